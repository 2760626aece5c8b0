/*
 * mk.h -- C ABI of the MI355X batched executor for Misaka Net TIS networks.
 *
 * Drop-in boundary (SURVEY.md section 8 row b).  The reference has no FFI; the
 * path sits behind the master's HTTP surface and the Go-internal node types.
 * Each entry point below names the reference interface it replaces.  Plain C:
 * no C++ types, caller-owned arrays, the library never retains a caller
 * pointer after return (cgo pointer-passing rules), never exits or aborts.
 *
 * Thread safety: every call is safe to make concurrently on one mk_net
 * (Go net/http runs /compute handlers concurrently, master.go:197).  The host
 * API serialises per handle.  Launches of one handle on one device share its
 * scratch (stack slots, counters), so the library orders them across
 * streams: work enqueued on a stream other than the previous launch's waits
 * for that launch (the host API's internal stream included).  Callers that
 * never change stream pay nothing for it.
 */
#ifndef MK_H
#define MK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (negative returns) ---------------------------------- */
#define MK_OK 0
#define MK_EINVAL (-1)  /* bad argument                                   */
#define MK_EPARSE (-2)  /* program text rejected (Go error text in err)   */
#define MK_ELIMIT (-3)  /* network exceeds executor limits                */
#define MK_EDEVICE (-4) /* HIP runtime error / no usable GPU              */
#define MK_ENOMEM (-5)  /* allocation failed                              */
#define MK_EBUSY (-6)   /* would block: port full / stack empty (retry)  */

/* ---- limits ------------------------------------------------------------ */
#define MK_MAX_PROGRAM_NODES 16
#define MK_MAX_STACK_NODES 32
#define MK_MAX_LINES 65535

/* ---- per-lane status byte ---------------------------------------------- */
#define MK_ST_QUIESCENT 1      /* every node blocked (reference: /compute hangs if no output) */
#define MK_ST_BUDGET 2         /* retired-instruction budget reached at a round end           */
#define MK_ST_STACK_OVERFLOW 3 /* a PUSH exceeded stack_cap (reference stacks are unbounded)  */
#define MK_ST_OUTPUT_STOP 4    /* stopped at the first OUT (MK_FLAG_STOP_ON_OUTPUT)           */
#define MK_ST_REMOTE_WAIT 5    /* session call parked on remote peers / inbound RPCs (row f4)  */
#define MK_ST_CALL_OPEN 6      /* session: a call is still open; this new one did nothing      */
#define MK_ST_REASON_MASK 0x0f
#define MK_ST_HAS_OUTPUT 0x10  /* lane produced a /compute result                              */

/* ---- node kinds ----------------------------------------------------------
 * NODE_INFO types (master.go:431-438, docker-compose.yml:16-21) plus the
 * master's own name (MASTER_URI, cmd/app.go:20): a program that addresses the
 * master with MOV/PUSH/POP gets the reference's Unimplemented-and-retry
 * behaviour instead of the unknown-host hang. */
#define MK_NODE_PROGRAM 0
#define MK_NODE_STACK 1
#define MK_NODE_MASTER 2
/* Peers served outside this executor -- reference nodes of a mixed
 * deployment (row f4): MOV to a remote program's port, PUSH / POP on a
 * remote stack become requests a stateful session hands to its host, which
 * makes the reference's RPC (Program.Send, Stack.Push / Stack.Pop,
 * messenger.proto:9-28; see mk_session_remote_*).  Batch lanes have no
 * peers: such an instruction blocks there forever. */
#define MK_NODE_REMOTE_PROGRAM 3
#define MK_NODE_REMOTE_STACK 4

typedef struct mk_net mk_net;

typedef struct {
    const char *name;    /* service name other nodes address it by          */
    int kind;            /* MK_NODE_*                                        */
    const char *program; /* TIS source for MK_NODE_PROGRAM (NULL = "")     */
} mk_node_desc;

#define MK_FLAG_STOP_ON_OUTPUT 1u
/* Skip the schedule compiler and run the direct bytecode interpreter
 * (tier 1).  By default a network is first compiled into superblocks of
 * micro-ops (tier 2); networks the compiler cannot bound fall back to
 * tier 1 automatically.  Both tiers give identical results. */
#define MK_FLAG_FORCE_INTERP 2u
/* Select the tier-2 superblock interpreter with the given lane scheduling
 * (results are identical either way; tier 2's default is TILE).  TILE: every
 * thread owns K contiguous inputs of a tile and the tile is written back with
 * vector stores once all of its lanes finished.  REFILL: a finished slot
 * immediately takes the next input. */
#define MK_FLAG_TILE 4u
#define MK_FLAG_REFILL 8u
/* Tier 3: the compiled schedule as a native gfx950 kernel generated and
 * compiled (hiprtc) once per network and option set.  Used by default when
 * the schedule fits its limits; MK_FLAG_JIT demands it (MK_ELIMIT when it is
 * unavailable -- mk_net_plan gives the reason), MK_FLAG_TILE / MK_FLAG_REFILL
 * select the tier-2 superblock interpreter, MK_FLAG_FORCE_INTERP tier 1.
 * MK_JIT=0 in the environment disables tier 3. */
#define MK_FLAG_JIT 16u
/* Device API: gather the counters of this launch without folding them into
 * d_stats yet (d_stats may be NULL).  Counters of deferred launches on one
 * handle and device accumulate on the device until mk_stats_fold (or the
 * next launch that folds); launches that defer must be stream-ordered with
 * each other and with the fold. */
#define MK_FLAG_DEFER_STATS 32u

typedef struct {
    uint32_t budget;      /* retired node-instructions per lane; 0 = 1<<20          */
    uint32_t stack_cap;   /* values per stack per lane; 0 = 1024                     */
    uint32_t flags;       /* MK_FLAG_*                                               */
    uint32_t device_mask; /* host API: GPUs to shard the batch over; 0 = GPU 0 only */
} mk_opts;

/* Parse + lower every program node and wire ports/stacks.
 * Replaces: ProgramNode.LoadProgram (internal/nodes/program.go:178-193) ->
 * tis.GenerateLabelMap / tis.Tokenize (internal/tis/tokenizer.go:11-106) for
 * every node of NODE_INFO (cmd/app.go:31), plus the name resolution that the
 * reference does per call with grpc.Dial (program.go:492,510,525).
 * Parse errors return MK_EPARSE with "node <name>: <Go error text>" in err,
 * where the Go text is byte-identical to the reference's
 * ("Cannot repeat label", "line N, label 'L' was not declared",
 *  "line N, '<instr>' not a valid instruction"). */
int mk_net_load(const mk_node_desc *nodes, int n, mk_net **out, char *err, size_t err_len);

void mk_net_free(mk_net *net);

/* Evaluate n independent /compute inputs (host arrays).
 * Replaces: the /compute handler (master.go:197-224) + GetInput/SendOutput
 * (master.go:233-249) + the program/stack node loops (program.go:80-92,
 * stack.go:95-155) for a batch.  in[i] is the strconv.Atoi value of the form
 * field; it is truncated to int32 inside, as GetInput does (master.go:237).
 * out[i] is the first OUT value (what /compute returns), status[i] the
 * MK_ST_* byte, steps[i] (nullable) the retired node-instructions. */
int mk_compute_batch(mk_net *net, const int64_t *in, size_t n, int32_t *out, uint8_t *status,
                     uint32_t *steps, const mk_opts *opts);

/* ---- device API (inputs/outputs already in HBM) ------------------------- */
#define MK_IN_I64 0 /* data: const int64_t*                                   */
#define MK_IN_I32 1 /* data: const int32_t*                                   */
#define MK_IN_GEN 2 /* synthetic: x_i = gen(seed, offset + i), no input bytes */

#define MK_GEN_FULL 0   /* (int32)splitmix64(seed^i); lanes i%16==15 take int32 edge values */
#define MK_GEN_MASKED 1 /* splitmix64(seed^i) & mask                                          */

typedef struct {
    int kind;          /* MK_IN_*                               */
    const void *data;  /* device pointer (MK_IN_I64 / MK_IN_I32) */
    uint64_t seed;     /* MK_IN_GEN                             */
    uint32_t gen_kind; /* MK_GEN_*                              */
    uint32_t gen_mask;
    uint64_t offset;   /* global lane index of element 0        */
} mk_input;

/* stats (nullable, device uint64[8], accumulated, caller zeroes):
 * [0] retired node-instructions  [1] lanes with output  [2] lanes finished
 * [3] quiescent  [4] budget  [5] stack overflow  [6] output-stop  [7] reserved */
#define MK_STATS_LEN 8

/* Launch the executor on `device` on HIP stream `stream` (NULL = default).
 * d_out / d_status are required, d_steps / d_stats nullable.  Asynchronous. */
int mk_compute_device(mk_net *net, int device, const mk_input *in, size_t n, int32_t *d_out,
                      uint8_t *d_status, uint32_t *d_steps, uint64_t *d_stats,
                      const mk_opts *opts, void *stream);

/* ---- stateful sessions ------------------------
 * The reference's nodes keep running between /compute calls
 * (program.go:80-92): ACC, BAK, ptr, ports, stacks and the master's inChan /
 * outChan (capacity 1, master.go:58-59) persist from one call to the next.
 * A session set holds n such network instances in HBM, in the post-/reset,
 * post-/run state; one compute call performs one /compute (master.go:
 * 216-219) on every session at once: deposit in[i] once inChan is empty,
 * run until outChan holds a value and take it.  status[i] is
 * MK_ST_HAS_OUTPUT with out[i] the value, or why the call has no result:
 *   MK_ST_BUDGET: this slice of the call retired opts->budget instructions.
 *     The call stays OPEN -- the reference's handler keeps waiting while its
 *     nodes run on (program.go:80-92) -- and mk_session_step(in = NULL)
 *     continues it with a fresh budget; mk_session_cancel abandons it.
 *   MK_ST_QUIESCENT: nothing can change without another input (the
 *     reference's handler would block forever).  The call closes; the
 *     instance keeps its state and takes the next call's input.
 *   MK_ST_STACK_OVERFLOW: a PUSH beyond stack_cap (the reference's stacks
 *     are unbounded): the session stays ended (same status, no output) until
 *     mk_session_reset.
 *   MK_ST_CALL_OPEN: the session already had an open call; this call did
 *     nothing and its input was not taken.  The host calls return MK_EBUSY
 *     when any session had a call open as the launch began (a burst's later
 *     calls behind a call that stayed open in the same launch report it too,
 *     without MK_EBUSY).
 * steps[i] (nullable): instructions retired by the call so far, over all
 * its slices (mod 2^32).  The mk_net must outlive its sessions. */
typedef struct mk_session mk_session;

int mk_session_create(mk_net *net, int device, size_t n, const mk_opts *opts, mk_session **out);

/* One /compute call on every session (host arrays; synchronous). */
int mk_session_compute(mk_session *s, const int64_t *in, int32_t *out, uint8_t *status, uint32_t *steps);

/* ncalls sequential /compute calls on every session in one launch (host
 * arrays laid out [call][session]; synchronous): call c of session i takes
 * in[c*n + i] and reports out/status/steps[c*n + i], exactly as ncalls
 * mk_session_compute calls in a row would.  Replaces a burst of concurrent
 * /compute requests on the reference's one network (master.go:197-224 served
 * one at a time through inChan/outChan, :216-219); the master coalesces such
 * bursts into one call (misaka_net_amd.master). */
int mk_session_compute_seq(mk_session *s, const int64_t *in, size_t ncalls, int32_t *out, uint8_t *status,
                           uint32_t *steps);

/* One call on device arrays, asynchronous on `stream` (NULL = the session's
 * own stream); calls on one session are ordered device-side, with no host
 * synchronisation: a call waits on an event recorded after the previous
 * launch when that ran on another stream (calls on one stream follow stream
 * order), and the session's synchronous calls below wait on it too.  The
 * event is the completion event of the launch's last kernel (no separate
 * marker on the stream: ~3 us per call less).  A
 * caller stream must outlive the session work queued on it; mk_session_free
 * waits for the last launch on any stream. */
int mk_session_compute_device(mk_session *s, const int64_t *d_in, int32_t *d_out, uint8_t *d_status,
                              uint32_t *d_steps, void *stream);

/* mk_session_compute_seq on device arrays ([call][session], d_steps
 * nullable), asynchronous on `stream` like mk_session_compute_device: a burst
 * of ncalls sequential /compute calls per instance in one launch, the state
 * loaded from HBM once and stored once.  Statuses report MK_ST_CALL_OPEN as
 * the host call does; nothing here returns MK_EBUSY (the statuses stay on the
 * device). */
int mk_session_compute_seq_device(mk_session *s, const int64_t *d_in, size_t ncalls, int32_t *d_out,
                                  uint8_t *d_status, uint32_t *d_steps, void *stream);

/* ---- mixed deployments (row f4): sessions of a network with remote peers --
 * A call on such a session runs until it has its output or nothing more can
 * happen without the peers; then it is PARKED: status MK_ST_REMOTE_WAIT,
 * no output, the call still open.  The host then
 *   - makes the RPC of every outstanding request (mk_session_remote_poll:
 *     Program.Send to a remote port, Stack.Push / Stack.Pop on a remote stack,
 *     program.go:475-536) and reports each completion (mk_session_remote_done,
 *     with the popped value for a pop);
 *   - serves the peers' RPCs to this instance's nodes: Program.Send into a
 *     local port (mk_session_port_put, MK_EBUSY while full: program.go:163),
 *     Stack.Push / Stack.Pop on a local stack (mk_session_stack_push / _pop,
 *     MK_EBUSY while empty: stack.go:133-155), and Master.GetInput /
 *     SendOutput on the master's channels (mk_session_input_take /
 *     _output_put);
 *   - resumes the call (mk_session_step with in = NULL).
 * All of these are ordered on the session's stream and synchronous. */
#define MK_REMOTE_SEND 0
#define MK_REMOTE_PUSH 1
#define MK_REMOTE_POP 2
typedef struct {
    uint32_t node;   /* local program node (sorted-name index) making the request */
    uint32_t op;     /* MK_REMOTE_*                                              */
    uint32_t remote; /* index of the peer among the network's MK_NODE_REMOTE_* nodes */
    uint32_t reg;    /* MK_REMOTE_SEND: the peer's port R0..R3                   */
    int32_t value;   /* SEND / PUSH: int32 value                                 */
} mk_remote_req;

/* One call step on every session: a new /compute call with in[i] (host
 * arrays), or, with in == NULL, resume each session's open call (parked on
 * peers, or out of budget); sessions without one report status 0. */
int mk_session_step(mk_session *s, const int64_t *in, int32_t *out, uint8_t *status, uint32_t *steps);
int mk_session_remote_poll(mk_session *s, size_t inst, mk_remote_req *reqs, int max, int *count);
int mk_session_remote_done(mk_session *s, size_t inst, uint32_t node, int32_t value);
int mk_session_port_put(mk_session *s, size_t inst, uint32_t node, uint32_t reg, int32_t value);
int mk_session_stack_push(mk_session *s, size_t inst, uint32_t stack, int32_t value);
int mk_session_stack_pop(mk_session *s, size_t inst, uint32_t stack, int32_t *value);
/* The master's side for remote program nodes that do IN / OUT: their
 * Master.GetInput takes from this instance's inChan (master.go:233-242;
 * MK_EBUSY while it is empty and no open call holds an input to deposit --
 * the reference's receive blocks), their Master.SendOutput deposits into its
 * outChan (master.go:245-249; MK_EBUSY while full).  The open call takes
 * that output when it resumes. */
int mk_session_input_take(mk_session *s, size_t inst, int32_t *value);
int mk_session_output_put(mk_session *s, size_t inst, int32_t value);

/* Kind (MK_NODE_*) and index of a node by name: program and stack nodes in
 * sorted-name order (the canonical schedule), remote peers in declaration
 * order. */
int mk_net_node_index(const mk_net *net, const char *name, int *kind, int *index);

/* Abandon every session's open call (the master answered it 504).  What it
 * set in motion stays: an input it deposited in inChan, the nodes' progress;
 * an input not deposited yet is dropped.  Synchronous. */
int mk_session_cancel(mk_session *s);

/* Which tier runs the sessions, as one line of text: "tier=native ..." --
 * the network's session schedule compiled to a kernel (one thread per
 * session, state in HBM; a call whose budget slice ends inside a superblock
 * is handed to the interpreter, which keeps that session) -- or
 * "tier=interp reason=..." (the bytecode interpreter for every session:
 * mixed deployments, networks the compiler declines, MK_SESSION_NATIVE=0).
 * Host-side state access (mk_session_port_put, _stack_*, _input_take,
 * _output_put) is for interpreter sessions: MK_EINVAL on the native tier. */
int mk_session_plan(const mk_session *s, char *out, size_t out_len);

/* /reset (master.go:126-143): every session back to the initial state. */
int mk_session_reset(mk_session *s);

/* ---- indexed forms: calls, resumes and resets on a chosen subset -----------
 * An index list sel[0..m) names the sessions a launch acts on: uint32_t,
 * strictly increasing, every entry < n (so m <= n).  Entry t of the launch is
 * session sel[t]: the I/O arrays have m columns, not n -- call c of entry t
 * takes in[c*m + t] and reports out/status/steps[c*m + t].  A session outside
 * the list is not touched: its registers, ports, stacks, inChan / outChan,
 * its open call and the tier that holds it stay as they were -- frozen, as
 * every session is between calls.  Indexed and plain launches on one set are
 * ordered against each other like the plain ones, whatever they select.
 * m == 0 is MK_OK and launches nothing.
 *
 * The host forms (host arrays, synchronous) check the list and return
 * MK_EINVAL for a bad one before anything is queued; they return MK_EBUSY
 * when a LISTED session reported MK_ST_CALL_OPEN on a new call. */
int mk_session_compute_indexed(mk_session *s, const uint32_t *sel, size_t m, const int64_t *in, size_t ncalls,
                               int32_t *out, uint8_t *status, uint32_t *steps);
/* mk_session_step on the listed sessions; in NULL: resume their open calls. */
int mk_session_step_indexed(mk_session *s, const uint32_t *sel, size_t m, const int64_t *in, int32_t *out,
                            uint8_t *status, uint32_t *steps);
/* mk_session_compute_seq_device on the listed sessions.  d_sel is a device
 * array taken ON TRUST: the caller guarantees that it is strictly increasing
 * with every entry < n (two entries naming one session would race on its
 * state), and keeps it valid and unchanged until the launch completes.  The
 * only net below that contract: an entry >= n touches no session and reports
 * out 0 / status 0. */
int mk_session_compute_indexed_device(mk_session *s, const uint32_t *d_sel, size_t m, const int64_t *d_in,
                                      size_t ncalls, int32_t *d_out, uint8_t *d_status, uint32_t *d_steps,
                                      void *stream);
/* mk_session_cancel / mk_session_reset for the listed sessions only.  A
 * reset clears the set's MK_EDEVICE-after-a-failed-launch condition only when
 * the list covers every session. */
int mk_session_cancel_indexed(mk_session *s, const uint32_t *sel, size_t m);
int mk_session_reset_indexed(mk_session *s, const uint32_t *sel, size_t m);
/* open[t] = 1 when session sel[t] has a call open (MK_ST_BUDGET or
 * MK_ST_REMOTE_WAIT was its last word), else 0.  sel NULL with m == n: every
 * session.  Synchronous. */
int mk_session_call_open(mk_session *s, const uint32_t *sel, size_t m, uint8_t *open);

/* ---- open calls: the list, the device resume and the drain -------------------
 * A call that outlives its budget slice stays open (MK_ST_BUDGET) until
 * resumes finish it.  These forms find and finish open calls on the GPU.
 * sel[0..m) as in the indexed forms; sel NULL with m == n: every session.  The
 * host forms check the list and return MK_EINVAL before anything is queued; the
 * device forms take it ON TRUST under the contract of
 * mk_session_compute_indexed_device, and an entry >= n touches nothing.
 * m == 0 is MK_OK and launches nothing.  All of them are ordered against every
 * other launch of the set like the indexed forms.  Their scratch belongs to the
 * set and grows on demand: a call synchronises only when it has to grow (it
 * never shrinks), and MK_ENOMEM leaves the set usable.
 *
 * The open list: list[0..*count) holds the listed sessions that have a call
 * open (what mk_session_call_open reports), in increasing order, and pos[k]
 * (nullable) the t with sel[t] == list[k] -- list[k] itself for a null sel.
 * list[*count..m) is 0xffffffff and pos[*count..m) is 0, the padding of
 * mk_requests_group_device: the list is a valid d_sel of the indexed and ragged
 * device forms over m entries with no read-back of the count.  list and pos
 * have m words and must not overlap sel. */
int mk_session_open_list(mk_session *s, const uint32_t *sel, size_t m, uint32_t *list, uint32_t *pos /* nullable */,
                         size_t *count);
/* Device form, asynchronous on `stream`; *d_count is one word. */
int mk_session_open_list_device(mk_session *s, const uint32_t *d_sel, size_t m, uint32_t *d_list,
                                uint32_t *d_pos /* nullable */, uint32_t *d_count, void *stream);
/* mk_session_step_indexed(in = NULL) on device arrays of m columns,
 * asynchronous on `stream`: one more budget slice of the listed sessions' open
 * calls.  A listed session without one reports out 0, steps 0 and status 0, or
 * MK_ST_STACK_OVERFLOW if it has ended, as the host form does. */
int mk_session_resume_device(mk_session *s, const uint32_t *d_sel, size_t m, int32_t *d_out, uint8_t *d_status,
                             uint32_t *d_steps /* nullable */, void *stream);
/* The drain: resumes the listed sessions' open calls slice after slice until
 * they answer or max_slices slices have run.  Its result is that of
 *   slice 1                mk_session_step_indexed(sel, in = NULL)
 *   slices 2..max_slices   the same on exactly the entries whose last status
 *                          was MK_ST_BUDGET
 * with entry t reporting, at column t of m, the out, status and steps of the
 * last slice that ran it (steps accumulate over a call's slices, as a resume
 * reports them); an entry with no call open at the start reports what
 * mk_session_resume_device does.  *still_open (nullable) is the number of
 * entries whose final status is MK_ST_BUDGET; MK_OK whether or not calls stay
 * open.  On the GPU the open calls are packed into a list (above) and each
 * slice runs over the list alone, repacked after it, so a slice costs what the
 * calls still open cost, not the whole set.  MK_EINVAL for max_slices == 0 and
 * for sets of a network with remote peers: there the host serves the peers
 * between slices.  The host form is synchronous and stops at the first slice
 * that leaves nothing open. */
int mk_session_drain(mk_session *s, const uint32_t *sel, size_t m, uint32_t max_slices, int32_t *out,
                     uint8_t *status, uint32_t *steps /* nullable */, size_t *still_open /* nullable */);
/* Device form, asynchronous on `stream` and without any read-back: all
 * max_slices slices are queued over m entries, those past the last open call
 * over padding that the `>= n` guard drops.  *d_still_open is one word. */
int mk_session_drain_device(mk_session *s, const uint32_t *d_sel, size_t m, uint32_t max_slices, int32_t *d_out,
                            uint8_t *d_status, uint32_t *d_steps /* nullable */,
                            uint32_t *d_still_open /* nullable */, void *stream);

/* ---- ragged bursts: each listed session its own number of calls -------------
 * sel[0..m) as in the indexed forms; sel NULL with m == n: every session.
 * off[0..m] (uint32_t) gives each entry's place in the I/O arrays: off[0] == 0,
 * non-decreasing, off[m] == total < 2^32.  Entry t makes cnt = off[t+1] - off[t]
 * sequential /compute calls on session sel[t], exactly as that many
 * mk_session_compute_indexed calls on {sel[t]} would: call c of entry t takes
 * in[off[t] + c] and reports out/status/steps[off[t] + c] -- the arrays are
 * entry-major and compact, of length total (with every cnt 1, the indexed
 * layout).  An entry with cnt 0 is not touched, like a session outside the
 * list.  Within an entry the rules of a uniform burst hold: after a call that
 * stays open (MK_ST_BUDGET) the later ones report MK_ST_CALL_OPEN and their
 * inputs are not taken; after a stack overflow they report
 * MK_ST_STACK_OVERFLOW with out 0.  m == 0 or total == 0 is MK_OK and
 * launches nothing.  Resumes stay with mk_session_step_indexed.
 *
 * The host form checks the list and the offsets and returns MK_EINVAL for bad
 * ones before anything is queued; it returns MK_EBUSY when a listed session
 * with cnt >= 1 reported MK_ST_CALL_OPEN on its first call. */
int mk_session_compute_ragged(mk_session *s, const uint32_t *sel, size_t m, const uint32_t *off, const int64_t *in,
                              int32_t *out, uint8_t *status, uint32_t *steps);
/* Device form, asynchronous on `stream`: d_sel and d_off (m + 1 words) are
 * taken ON TRUST under the contract of mk_session_compute_indexed_device, and
 * the arrays hold `total` words.  The only net below that contract: entry t
 * is served only if d_sel[t] < n and d_off[t] <= d_off[t+1] <= total; one that
 * is not loads nothing, stores nothing and writes no I/O word. */
int mk_session_compute_ragged_device(mk_session *s, const uint32_t *d_sel, size_t m, const uint32_t *d_off,
                                     size_t total, const int64_t *d_in, int32_t *d_out, uint8_t *d_status,
                                     uint32_t *d_steps, void *stream);

/* ---- request queues: arrival order in, grouped on the GPU --------------------
 * A queue is `total` < 2^32 requests in arrival order: request j is for
 * session ids[j] (any order, repeats allowed), carries in[j] and is answered
 * at out[j], status[j], steps[j].  The launch behaves exactly as if the
 * requests were served one at a time in arrival order, each as a one-entry
 * mk_session_compute_indexed call on {ids[j]}: sessions are independent, the
 * requests of one session run in arrival order, every answer returns to its
 * own position.  Within one session the rules of a burst hold, as in a ragged
 * entry (MK_ST_CALL_OPEN after a call that stays open, its input not taken;
 * MK_ST_STACK_OVERFLOW with out 0 after an overflow).  A session with no
 * request is not touched.  total == 0 is MK_OK and launches nothing.  The
 * grouping -- a stable sort by session and a compaction -- runs on the GPU and
 * feeds one ragged launch: whatever mk_session_compute_ragged accepts or
 * refuses for a set the queue forms do likewise, and they order against every
 * other launch of the set as the ragged forms do.
 *
 * The host form returns MK_EINVAL for any ids[j] >= n before anything is
 * queued, and MK_EBUSY when a request that is the first of its session in
 * this queue reported MK_ST_CALL_OPEN. */
int mk_session_compute_queue(mk_session *s, const uint32_t *ids, const int64_t *in, size_t total, int32_t *out,
                             uint8_t *status, uint32_t *steps /* nullable */);
/* Device form, asynchronous on `stream`, no host synchronisation unless the
 * set's queue scratch has to grow (it never shrinks; MK_ENOMEM leaves the set
 * usable).  d_ids is taken ON TRUST; the net: a request with d_ids[j] >= n
 * touches no session -- whatever its low bits -- and reports out 0, status 0,
 * steps 0. */
int mk_session_compute_queue_device(mk_session *s, const uint32_t *d_ids, const int64_t *d_in, size_t total,
                                    int32_t *d_out, uint8_t *d_status, uint32_t *d_steps, void *stream);
/* The grouping alone, for any n in [1, 2^32 - 1], on `device`, asynchronous on
 * `stream`.  With key[j] = min(d_ids[j], n) and M = min(total, n):
 *   d_perm[0..total)  the stable order of the keys: key[perm[k]] non-decreasing,
 *                     ties in increasing j (numpy argsort, kind="stable")
 *   *d_m              the number of distinct keys below n
 *   d_sel[0..M)       those m keys, increasing, then 0xffffffff
 *   d_off[0..M]       for t < m the first k with key[perm[k]] == sel[t]; for
 *                     m <= t <= M the number of requests with an id below n
 * so that (d_sel, M, d_off, total) is a ragged launch over the requests in
 * perm order whose padded entries the ragged guard drops.  d_tmp: scratch of
 * at least the bytes mk_requests_group_tmp_bytes reports, 4-byte aligned.
 * MK_EINVAL for n == 0, total >= 2^32, a null pointer with total > 0 or a
 * scratch too small; total == 0 writes *d_m = 0 and d_off[0] = 0. */
int mk_requests_group_tmp_bytes(uint32_t n, size_t total, size_t *bytes);
int mk_requests_group_device(int device, uint32_t n, const uint32_t *d_ids, size_t total, uint32_t *d_perm,
                             uint32_t *d_sel, uint32_t *d_off, uint32_t *d_m, void *d_tmp, size_t tmp_bytes,
                             void *stream);

/* ---- served queues: a request queue answered to completion -------------------
 * A queue as above (`total` < 2^32 requests, request j for session ids[j] with
 * in[j], answered at position j), served until every call has answered or
 * used up its slices.  The result is that of this sequence, the requests taken
 * in arrival order:
 *   (out, status, steps)[j] = mk_session_compute_indexed({ids[j]}, in[j])
 *   up to max_slices times while status[j] == MK_ST_BUDGET:
 *   (out, status, steps)[j] = mk_session_step_indexed({ids[j]}, in = NULL)
 * so a call gets its own slice and at most max_slices resume slices -- what
 * mk_session_drain(max_slices) gives it -- and steps accumulate over them as a
 * resume reports them.  A call still at MK_ST_BUDGET after that stays open: the
 * later requests of its session report MK_ST_CALL_OPEN and their inputs are not
 * taken.  A session whose call was open before the serve is never resumed by
 * it: all its requests report MK_ST_CALL_OPEN and the open call is left exactly
 * as it was.  After a stack overflow the later requests report
 * MK_ST_STACK_OVERFLOW with out 0, as in any burst.  A session with no request
 * is not touched.  total == 0 is MK_OK and launches nothing.
 *
 * On the GPU the queue is grouped once and served in rounds: one ragged launch
 * over the sessions that still have requests to run, the drain over those
 * whose call hit the budget in it, and the sessions whose drained call
 * answered go into the next round with the requests behind that call.  Both
 * forms are ordered against every other launch of the set like the queue
 * forms.  Their scratch belongs to the set and grows on demand: a call
 * synchronises only when it has to grow (it never shrinks), and MK_ENOMEM
 * leaves the set usable.  MK_EDEVICE on a set broken by a failed launch;
 * MK_EINVAL for max_slices == 0 and for sets of a network with remote peers:
 * there the host serves the peers between slices, as for the drain.
 *
 * The host form is synchronous and runs rounds until no request is left to
 * run, reading the next round's size back after each, so that a round after
 * the first costs what the sessions and requests still to run cost, not the
 * whole queue.  *still_open (nullable) is the number of requests whose final
 * status is MK_ST_BUDGET, *rounds (nullable) the number of ragged launches
 * made.  MK_EINVAL for any ids[j] >= n before anything is queued; MK_EBUSY,
 * like the queue form, when a request that is the first of its session
 * reported MK_ST_CALL_OPEN. */
int mk_session_serve(mk_session *s, const uint32_t *ids, const int64_t *in, size_t total, uint32_t max_slices,
                     int32_t *out, uint8_t *status, uint32_t *steps /* nullable */,
                     size_t *still_open /* nullable */, size_t *rounds /* nullable */);
/* Device form, asynchronous on `stream` and without any read-back: exactly
 * max_rounds >= 1 rounds are queued, every one over the padded full length, as
 * mk_session_drain_device queues its slices.  A request that no round reached
 * is unserved: out 0, status 0, steps 0, its input not taken.  The unserved
 * requests of one session are always a suffix of its requests in arrival
 * order, so serving the unserved requests again, in their original order,
 * gives what one serve with enough rounds gives.  d_left (nullable, 2 words):
 * d_left[0] the number of requests left open, d_left[1] the number unserved.
 * d_ids is taken ON TRUST; the net: a request with d_ids[j] >= n touches no
 * session, reports out 0, status 0, steps 0 and is not counted as unserved. */
int mk_session_serve_device(mk_session *s, const uint32_t *d_ids, const int64_t *d_in, size_t total,
                            uint32_t max_slices, uint32_t max_rounds, int32_t *d_out, uint8_t *d_status,
                            uint32_t *d_steps /* nullable */, uint32_t *d_left /* nullable, 2 words */, void *stream);

/* ---- client keys: a directory from 64-bit keys to instances ------------------
 * A server names its clients by connection ids, user ids or hashes, not by
 * instance numbers.  A set has at most one directory: a partial injective map
 * from uint64_t keys to the set's instances, and a FIFO of the free instances,
 * both on the GPU.  MK_KEY_NONE is never bound; every other key is valid.
 *
 *   open     the set is reset as mk_session_reset resets it, every instance is
 *            free, and the FIFO is 0, 1, ..., n-1.
 *   bind     keys[0..total) in arrival order to ids[0..total).  A key bound
 *            before the call gives its instance.  The distinct keys that are not
 *            bound are the new keys, in the order of their first occurrence in
 *            this queue: the k-th of them takes the k-th instance from the front
 *            of the FIFO.  When the FIFO runs out the remaining new keys are
 *            rejected: they stay unbound and every one of their requests gets
 *            0xffffffff.  A MK_KEY_NONE request gets 0xffffffff and is counted
 *            nowhere.  counts = {keys admitted, keys rejected, requests of
 *            rejected keys}.  An admitted instance is in the post-/reset state:
 *            open and release keep every free instance there.  0xffffffff is
 *            what the queue and serve forms treat as "touches no session".
 *   lookup   as bind, but nothing is admitted: an unbound key gives 0xffffffff.
 *   release  every listed key that is bound loses its binding; its instance is
 *            reset as mk_session_reset_indexed resets it, once, and goes to the
 *            back of the FIFO, the instances of one release in increasing
 *            order.  Unbound keys, MK_KEY_NONE and repeats are ignored.
 *   export   owner[i] = the key of instance i, MK_KEY_NONE for a free one.
 *   import   replaces the whole directory by such an array and resets nothing;
 *            the FIFO is then the free instances in increasing order.
 *            MK_EINVAL, and nothing changes, when a key occurs twice.  With
 *            snapshot and restore this carries a keyed set to another set or
 *            process.
 *
 * The directory never looks at instance state, and mk_session_reset leaves the
 * bindings in place.  The ids depend on nothing but the contract above: not on
 * the order in which the GPU's threads run.  Bind and lookup cost what `total`
 * requests cost and never pass over the n instances; a release costs what its
 * m listed keys cost, and now and then -- after releases that listed a quarter
 * of the table's slots in all, bound or not -- a rebuild of the table over the n instances, so deletions
 * never degrade it (info.tombstones <= info.slots / 4 after every release).
 * The table is open addressing with linear probing in mk_session_dir_slots(n)
 * slots of 12 bytes, the power of two that is at least 2n; with the owner
 * array and the FIFO that is 36 to 60 bytes an instance.  MK_ELIMIT for sets
 * of more than 2^30 instances.
 *
 * Every operation is ordered against every other launch of the set like the
 * indexed forms.  MK_EINVAL without a directory (and for a second open), for
 * total or m >= 2^32 and for null arrays; MK_EDEVICE on a set broken by a failed
 * launch; total == 0 and m == 0 are MK_OK and launch nothing.  The scratch
 * belongs to the set and grows on demand: a call synchronises only when it has
 * to grow (it never shrinks), and MK_ENOMEM leaves the set usable.  The host
 * forms are synchronous; the device forms are asynchronous on `stream`, read
 * nothing back and take their arrays ON TRUST. */
#define MK_KEY_NONE 0xffffffffffffffffull
typedef struct {
    uint32_t slots, live, free, tombstones;
} mk_session_dir_info;

int mk_session_dir_open(mk_session *s);
int mk_session_dir_close(mk_session *s); /* also freed with the set */
int mk_session_dir_info_get(mk_session *s, mk_session_dir_info *out);
int mk_session_dir_export(mk_session *s, uint64_t *owner /* n */);
int mk_session_dir_import(mk_session *s, const uint64_t *owner /* n */);

int mk_session_bind(mk_session *s, const uint64_t *keys, size_t total, uint32_t *ids,
                    size_t counts[3] /* nullable */);
int mk_session_bind_device(mk_session *s, const uint64_t *d_keys, size_t total, uint32_t *d_ids,
                           uint32_t *d_counts /* nullable, 3 words */, void *stream);
int mk_session_lookup(mk_session *s, const uint64_t *keys, size_t total, uint32_t *ids);
int mk_session_lookup_device(mk_session *s, const uint64_t *d_keys, size_t total, uint32_t *d_ids, void *stream);
int mk_session_release(mk_session *s, const uint64_t *keys, size_t m, size_t *released /* nullable */);
int mk_session_release_device(mk_session *s, const uint64_t *d_keys, size_t m,
                              uint32_t *d_released /* nullable */, void *stream);

/* Bind, then the queue / the serve on the ids, the keys staged once; ids
 * (nullable) returns the assignment.  Rejected and MK_KEY_NONE requests are
 * unserved (out 0, status 0, steps 0), not MK_EINVAL; everything else as the
 * unkeyed host forms, MK_EBUSY included.  On the device the same is
 * mk_session_bind_device followed by mk_session_compute_queue_device or
 * mk_session_serve_device on the ids. */
int mk_session_compute_queue_keyed(mk_session *s, const uint64_t *keys, const int64_t *in, size_t total,
                                   int32_t *out, uint8_t *status, uint32_t *steps /* nullable */,
                                   uint32_t *ids /* nullable */, size_t counts[3] /* nullable */);
int mk_session_serve_keyed(mk_session *s, const uint64_t *keys, const int64_t *in, size_t total,
                           uint32_t max_slices, int32_t *out, uint8_t *status, uint32_t *steps /* nullable */,
                           uint32_t *ids /* nullable */, size_t counts[3] /* nullable */,
                           size_t *still_open /* nullable */, size_t *rounds /* nullable */);

/* ---- idle clients: use stamps, selection and eviction ------------------------
 * A full directory rejects new keys.  A tracked one knows when each client was
 * last seen, so that the clients silent longest can make room, or be parked on
 * the host (snapshot, then release) before they have to.
 *
 *   track    turns tracking on: a 64-bit use stamp per instance on the device
 *            and a 64-bit clock on the host, the number of binds queued since
 *            (a bind of total == 0 launches nothing and does not tick).  Every
 *            instance bound at that moment gets stamp 0.  From then on every
 *            bind (mk_session_bind, _device, the keyed forms, bind_evict)
 *            stamps every instance its requests resolve to, hits and admissions
 *            alike, with the clock after its tick.  Lookup and release stamp
 *            nothing; mk_session_dir_import stamps every instance it binds with
 *            the current clock.  An untracked directory runs the same kernels,
 *            which skip the store.
 *   age(i)   min(clock - stamp[i], 2^32 - 1)
 *   eligible instance i for min_idle: bound, age(i) >= max(min_idle, 1), and no
 *            call open.
 *   the k most idle: the first k of the eligible instances ordered by (age
 *            descending, instance ascending).  Every list of victims is
 *            reported in increasing instance order, min(want, n) entries (for
 *            bind_evict min(max_evict, n)), padded with MK_KEY_NONE /
 *            0xffffffff: a valid list for the indexed, snapshot and reset
 *            forms.  Nothing depends on the order in which the GPU's threads run.
 *   idle_select  reports the min(want, eligible) most idle: keys, instances and
 *            their number.  Changes nothing and ticks nothing.
 *   evict    the same selection, then the victims are released as
 *            mk_session_release releases them (reset, to the back of the FIFO
 *            in increasing order).  keys and ids are nullable.
 *   bind_evict  a bind that makes room: need = max(0, new keys - free), and the
 *            k = min(need, max_evict, eligible) most idle are evicted before
 *            the new keys are admitted -- from the instances that were free
 *            first, then from the victims in increasing order.  What this bind's
 *            requests resolve to has age 0 and is never evicted.  What still
 *            finds no instance is rejected as by bind.  counts = {admitted,
 *            rejected keys, requests of rejected keys, evicted}.  With
 *            max_evict == 0 it is mk_session_bind in every output.
 *   use_export  stamp[i] (0 for a free instance) and the clock; use_import
 *            replaces both, beside mk_session_dir_export / _import (import the
 *            directory first).  MK_EINVAL, and nothing changes, when a bound
 *            instance has a stamp above the clock.
 *
 * A selection passes over the n instances a few times (sess_evict.h); a
 * bind_evict that lacks nothing pays the launches only.  The host cannot know
 * how many an eviction evicted on the device, so its bound on the tombstones
 * grows by min(want, n) (min(max_evict, n)) per evicting call, and the table is
 * rebuilt behind the call that takes the bound past slots / 4:
 * info.tombstones <= info.slots / 4 holds after every call.  Ask for no more
 * evictions than a call may need.
 *
 * MK_EINVAL on an untracked directory (track: without a directory and on a
 * second call), for null required arrays and for want or max_evict >= 2^32;
 * want == 0 is MK_OK and launches nothing.  Ordering, host and device forms as
 * for the directory above. */
typedef struct {
    uint64_t clock;    /* binds queued since tracking began */
    uint32_t tracking; /* 1 when mk_session_dir_track has been called */
    uint32_t reserved;
} mk_session_dir_use_info;

int mk_session_dir_track(mk_session *s); /* undone by mk_session_dir_close */
int mk_session_dir_use_info_get(mk_session *s, mk_session_dir_use_info *out);
int mk_session_dir_use_export(mk_session *s, uint64_t *last /* n */, uint64_t *clock /* nullable */);
int mk_session_dir_use_import(mk_session *s, const uint64_t *last /* n */, uint64_t clock);

int mk_session_idle_select(mk_session *s, size_t want, uint32_t min_idle, uint64_t *keys, uint32_t *ids,
                           size_t *count /* nullable */);
int mk_session_idle_select_device(mk_session *s, size_t want, uint32_t min_idle, uint64_t *d_keys, uint32_t *d_ids,
                                  uint32_t *d_count /* nullable */, void *stream);
int mk_session_evict(mk_session *s, size_t want, uint32_t min_idle, uint64_t *keys /* nullable */,
                     uint32_t *ids /* nullable */, size_t *count /* nullable */);
int mk_session_evict_device(mk_session *s, size_t want, uint32_t min_idle, uint64_t *d_keys /* nullable */,
                            uint32_t *d_ids /* nullable */, uint32_t *d_count /* nullable */, void *stream);
int mk_session_bind_evict(mk_session *s, const uint64_t *keys, size_t total, uint32_t *ids, size_t max_evict,
                          uint32_t min_idle, uint64_t *ev_keys /* nullable */, uint32_t *ev_ids /* nullable */,
                          size_t counts[4] /* nullable */);
int mk_session_bind_evict_device(mk_session *s, const uint64_t *d_keys, size_t total, uint32_t *d_ids,
                                 size_t max_evict, uint32_t min_idle, uint64_t *d_ev_keys /* nullable */,
                                 uint32_t *d_ev_ids /* nullable */, uint32_t *d_counts /* nullable, 4 words */,
                                 void *stream);

/* The device form of mk_session_reset_indexed, asynchronous on `stream`: d_sel
 * is taken ON TRUST (strictly increasing); an entry >= n touches nothing.
 * MK_EDEVICE on a set broken by a failed launch: only the host forms, which can
 * see that a list names all n sessions, mend such a set. */
int mk_session_reset_indexed_device(mk_session *s, const uint32_t *d_sel, size_t m, void *stream);

/* Pure host functions, usable without a GPU: the table size for n instances
 * (MK_EINVAL for n == 0, MK_ELIMIT above 2^30) and the slot each key's probe
 * starts at in a table of `slots` slots (a power of two), so that tests can
 * build colliding keys. */
int mk_session_dir_slots(size_t n, uint32_t *slots);
int mk_session_dir_home(const uint64_t *keys, size_t m, uint32_t slots, uint32_t *home);

/* ---- snapshots: a session's state out of the set and back -------------------
 * A session record is one session's whole state -- registers, ports, pending
 * sends, stacks, inChan / outChan, its open call, the tier that holds it --
 * as layout.rows 32-bit rows; an int64 takes two rows, low word first.  A
 * block of m records is laid out [row][m]: row r of entry t is rec[r*m + t].
 *   control    held io csteps pin in_val out_val bits pfull(2)
 *   per program node, sorted-name order
 *              acc(2) bak(2) ip pendv port[4]
 *   per stack  depth, then stack_cap entries (0 at and above the depth)
 *   native     sb, registers (2 rows each), stack slots: layout.native_rows
 *              rows, present only in blocks of a native-tier set, all zero for
 *              a record with held == 0
 * held: 1 when the native tier held the session, 0 when the interpreter did.
 * io: in_full | out_full << 1 | input not deposited << 2 | call open << 3 |
 * ended (MK_ST_STACK_OVERFLOW) << 4.  bits: pend | hung << 16, one bit per
 * program node.  Everything but the native section is the CANONICAL part, in
 * the bytecode interpreter's terms and always filled: a session the native
 * tier holds is between calls, so its record has the call closed.  The
 * canonical part of one history need not be word-identical between tiers (the
 * compiler drops dead values, the interpreter keeps stale ones in empty
 * ports); restored, it behaves identically.
 *
 * A restore overwrites the listed sessions completely.  A record with
 * held == 1 goes back to the native tier when the block's native_hash is the
 * set's own (and not 0); every other record is restored from its canonical
 * part, and in a native-tier set that session is the interpreter's until
 * promoted (mk_session_promote), as after a hand-off.  So a block can go to another set, another GPU or
 * another tier of the same network at the same stack_cap.
 *
 * Both operations are ordered against every other launch of the set like the
 * indexed forms; MK_EDEVICE on a set broken by a failed launch; MK_EINVAL for
 * sets of a network with remote peers (part of their state lives in the
 * peers).  sel NULL with m == n: every session.  m == 0 is MK_OK and
 * launches nothing. */
typedef struct {
    uint32_t magic;       /* "MKSR" */
    uint32_t version;
    uint64_t net_hash;    /* node names, kinds and the lowered bytecode */
    uint64_t native_hash; /* the session module's generated source; 0: interpreter-tier set */
    uint32_t nprog;
    uint32_t nstack;
    uint32_t stack_cap;
    uint32_t rows;        /* of one record, the native section included */
    uint32_t native_rows; /* 1 + 2 * registers + slots, or 0 */
    uint32_t reserved;
} mk_session_layout;

int mk_session_layout_get(const mk_session *s, mk_session_layout *out);
/* Host form, synchronous: rec is a host block [rows][m]; sel is checked as in
 * the indexed forms.  Staged through a temporary device block in chunks of
 * entries of at most 64 MiB of rows; MK_ENOMEM if one chunk cannot be had. */
int mk_session_snapshot(mk_session *s, const uint32_t *sel, size_t m, uint32_t *rec);
/* Device form, asynchronous on `stream`: d_sel as in
 * mk_session_compute_indexed_device (an entry >= n gives an all-zero record). */
int mk_session_snapshot_device(mk_session *s, const uint32_t *d_sel, size_t m, uint32_t *d_rec, void *stream);
/* Session sel[t] takes column col[t] (t with col NULL) of the block rec of
 * mcols columns described by `from`.  MK_EINVAL before anything is queued
 * when `from` disagrees with the set in magic, version, net_hash, nprog,
 * nstack or stack_cap, or its rows are not those of its sections.  The host
 * form also checks sel and every referenced record -- col[t] < mcols,
 * held <= 1, every ip inside its node's program, every depth <= stack_cap,
 * and for a record that goes back to the native tier an sb that is either
 * "ended" or a superblock a call starts at -- and returns MK_EINVAL for the
 * first bad one with no session changed. */
int mk_session_restore(mk_session *s, const uint32_t *sel, size_t m, const mk_session_layout *from,
                       const uint32_t *rec, size_t mcols, const uint32_t *col);
/* Device form: d_sel, d_rec and d_col are taken ON TRUST and kept valid and
 * unchanged until the launch completes.  The net below that contract is the
 * kernel's own guard: an entry that fails one of the checks above restores
 * nothing and leaves its session untouched. */
int mk_session_restore_device(mk_session *s, const uint32_t *d_sel, size_t m, const mk_session_layout *from,
                              const uint32_t *d_rec, size_t mcols, const uint32_t *d_col, void *stream);

/* ---- promotion: interpreter-held sessions back to the native tier ----------
 * In a native-tier set a session whose call ran out of its budget slice, or
 * that was restored from a record's canonical part, is the interpreter's; it
 * stays there until promoted.  A listed session is ELIGIBLE when the
 * interpreter holds it and its call is closed: none open, no hand-off of a
 * launch in flight, so no input or steps pending (io bits 2, 3 and 8-14
 * clear; pin and csteps count only while a call is open).  An eligible session
 * that has ended goes back as ended.
 * A live one goes back when its state is an instance of the entry state of a
 * superblock a call starts at: the control (every ip, pend, hung, pfull, the
 * channel bits, the ordinary stacks' depths) agrees exactly and every constant
 * the compiler built into that superblock's code has its value.  Where several
 * superblocks match, the one with the LOWEST INDEX is taken, so every build
 * and the CPU model agree session by session.  Every state that calls,
 * resumes, resets and restores of such states produce matches; a state left
 * by mk_session_cancel of an open call may match nothing, and that session
 * stays on the interpreter (flag 0).  Promotion changes no result: later calls
 * return what they would have returned, only on the faster tier.  Nothing
 * promotes by itself.
 *
 * Both forms are ordered against every other launch of the set like the
 * indexed forms; MK_EDEVICE on a set broken by a failed launch.  m == 0 is
 * MK_OK and launches nothing.  A set on the interpreter's tier (one with remote
 * peers included) has nowhere to promote to: MK_OK, all flags 0, nothing
 * launched. */
/* Host form, synchronous: sel as in the indexed forms (NULL with m == n: every session),
 * checked, MK_EINVAL before anything is queued.  promoted (nullable) has m bytes,
 * *count (nullable) the number promoted. */
int mk_session_promote(mk_session *s, const uint32_t *sel, size_t m, uint8_t *promoted, size_t *count);
/* Device form, asynchronous on `stream`: d_sel on trust under the indexed contract
 * (an entry >= n touches nothing and reports 0); d_promoted (nullable) has m bytes. */
int mk_session_promote_device(mk_session *s, const uint32_t *d_sel, size_t m, uint8_t *d_promoted, void *stream);

void mk_session_free(mk_session *s);

/* Add the counters accumulated by MK_FLAG_DEFER_STATS launches on `device`
 * into d_stats (device uint64[MK_STATS_LEN]) and clear them; asynchronous
 * on `stream`.  Replaces nothing in the reference (it has no counters). */
int mk_stats_fold(mk_net *net, int device, uint64_t *d_stats, void *stream);

/* Fill d_out[i] = gen(seed, offset + i) on device (same generator as MK_IN_GEN). */
int mk_generate_inputs_device(int device, uint64_t seed, uint32_t gen_kind, uint32_t gen_mask,
                              uint64_t offset, size_t n, int32_t *d_out, void *stream);

/* ---- lane trace -------------------------------------
 * The reference logs every instruction it executes (log.Printf of tokens,
 * ACC, BAK; program.go:222-223).  mk_trace_lane runs ONE /compute input
 * through the bytecode interpreter (tier 1, the tier that executes one TIS
 * instruction at a time) on `device` and returns its first max_entries
 * retired instructions in schedule order: round, program node (index in
 * sorted-name order), the ptr it executed at, ACC and BAK after it -- the
 * same records as the oracle's orc_trace_lane, so a lane whose result
 * differs can be diffed instruction by instruction.  *count = entries
 * written, *status = the lane's MK_ST_* byte.  Synchronous. */
typedef struct {
    uint32_t round;
    uint16_t node;
    uint16_t ip;
    int64_t acc;
    int64_t bak;
} mk_trace_entry;

int mk_trace_lane(mk_net *net, int device, int64_t input, const mk_opts *opts, mk_trace_entry *out,
                  uint32_t max_entries, uint32_t *count, uint8_t *status);

/* ---- introspection -------------------------------------------------------- */
/* Token dump of one program in the test format: lines joined by '\n', tokens
 * by '\x1f' (the [][]string of tis.Tokenize); on error the Go error text and
 * MK_EPARSE.  Replaces tis.Tokenize for parity tests. */
int mk_tokenize(const char *program, char *out, size_t out_len);

/* Lowered bytecode of a loaded network as text (one instruction per line). */
int mk_net_disasm(const mk_net *net, char *out, size_t out_len);

/* Which tier `opts` selects for this network and its shape, as one line of
 * text ("tier=native ..", "tier=compiled superblocks=.. regs=.. words=.." or
 * "tier=interp reason=.."); compiles the schedule (and the native kernel) if
 * not cached yet. */
int mk_net_plan(mk_net *net, const mk_opts *opts, char *out, size_t out_len);

/* Compile everything `opts` will use on `device` now (schedule, native
 * kernel, device tables) so the first mk_compute_* call does not pay for it.
 * Replaces nothing in the reference (its /load has no compile step); meant
 * for the master's /load and for benchmarks. */
int mk_net_prepare(mk_net *net, const mk_opts *opts, int device);

/* Generated source of the native (tier-3) kernel for `opts` (MK_ELIMIT with
 * the reason in `out` when the tier is unavailable). */
int mk_net_jit_source(mk_net *net, const mk_opts *opts, char *out, size_t out_len);

/* Micro-op listing of the compiled schedule for `opts` (MK_ELIMIT if the
 * network is not compilable). */
int mk_net_sched_disasm(mk_net *net, const mk_opts *opts, char *out, size_t out_len);

/* counts: [0] program nodes [1] stack nodes [2] total instructions */
int mk_net_info(const mk_net *net, int *counts3);

/* Integer-issue peak probe: launches a dependency-free v_add_u32 kernel doing
 * `iters` x 64 adds per lane over blocks x 256 lanes; returns the lane-op count
 * it performs in *lane_ops.  Caller times it with events on `stream`. */
int mk_valu_probe_device(int device, int blocks, int iters, uint64_t *lane_ops, void *stream);

const char *mk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MK_H */
