// sess_serve.h -- the bookkeeping of a served request queue
// (mk_session_serve, include/mk.h): a queue answered to completion, the calls
// that outlive their budget slice drained and the requests behind them run in
// the next round, all on the GPU.  The session kernels are the ones every other
// form launches; what is here chains them.
//
// The queue is grouped once (req_group.h): perm, and in sorted order the
// inputs, one entry per session with the run of its requests.  A round works on
// a round list of `len` slots, padded like every list here:
//   sel[k]          the slot's session (0xffffffff: padding)
//   beg[k]          the sorted position of its next unanswered request
//   off[k..k+1]     its place in the round's compact I/O arrays; off[len] is
//                   the number of requests the round holds
// The first round's list is the grouping itself (sel, off, off).  A round is
//   launch    one ragged session launch over the list
//   fold      sv_fold: every compact word back to the caller's position through
//             perm -- the MK_ST_CALL_OPEN words behind a MK_ST_BUDGET as
//             MK_ST_CALL_OPEN / 0 / 0, which holds unless a later round runs them
//             again and overwrites it -- and SvHit packs the slots that hit the
//             budget into the drain list (dr_compact), noting in hit[k] the
//             sorted position of the call that did
//   drain     the drain of sess_drain.h over that list into columns of its own
//   advance   sv_advance: a drained call's answer to its request's position;
//             SvNext packs the drained slots whose call answered and that have
//             requests left into the next round list, sv_next gives it beg and
//             the counts, rg_scan turns those into off, sv_gather fills the
//             next compact inputs
// A slot whose first word is MK_ST_CALL_OPEN had a call open before the serve:
// all its words are final and it is never in the drain list.  In a burst the
// statuses of a slot are monotone -- none is MK_ST_BUDGET or MK_ST_CALL_OPEN
// before the call that hit the budget, all are from it on -- so SvHit finds that
// call by bisection, and a request finds its slot by bisection over off
// (sv_slot): no kernel loops over a slot's requests, whatever the skew.
// sv_unserved ends the device form: the requests of the last list, which no
// round ran, back to 0 / 0 / 0, and the two counts.
//
// Every kernel writes with ordinary vector stores; a value one thread writes
// for the block is written under `if (threadIdx.x == ...)`.  Included by
// mk_exec.hip after sess_drain.h; everything here is static to it.
#pragma once

namespace mk {
namespace sv {

using rg::kRgBlock;

// the words of a serve's counters (ServeBufs::cnt)
enum { kPend = 0, kReq = 1, kOpen = 2, kStill = 3, kHit = 4, kCntWords = 8 };

struct SvList {
    const uint32_t *sel, *beg, *off;
};

// The slot of compact position q: the largest k < len with off[k] <= q.
// off[0] == 0, a slot with requests has off[k] < off[k + 1], and the padding
// behind them holds off[len], above every q there is.
__device__ __forceinline__ uint32_t sv_slot(const uint32_t *__restrict__ off, uint32_t len, uint32_t q)
{
    uint32_t lo = 0, hi = len;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool sv_stays(uint8_t st)
{
    return st == (uint8_t)MK_ST_BUDGET || st == (uint8_t)MK_ST_CALL_OPEN;
}

// Slot k of the round list the launch just ran over, kept when one of its calls
// hit the budget; the pass that emits writes hit[k], the sorted position of
// that call (of the slot's end without one).
struct SvHit {
    SvList l;
    uint32_t n, tot;         // sessions; requests of the queue
    const uint8_t *c_status; // the round's compact statuses
    uint32_t *hit;           // [len]

    __device__ __forceinline__ bool entry(uint32_t k, bool emit, uint32_t *id, uint32_t *col) const
    {
        const uint32_t i = l.sel[k], o0 = l.off[k], o1 = l.off[k + 1];
        const bool real = i < n && o0 < o1 && o1 <= tot;
        const uint32_t cnt = real ? o1 - o0 : 0u;
        uint32_t b = cnt;
        if (real && c_status[o0] != (uint8_t)MK_ST_CALL_OPEN) {
            uint32_t lo = 0, hi = cnt; // the first word that is MK_ST_BUDGET or behind one
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (sv_stays(c_status[o0 + mid])) hi = mid;
                else lo = mid + 1u;
            }
            b = lo;
        }
        *id = i;
        *col = k;
        if (emit) hit[k] = real ? l.beg[k] + b : 0u;
        return b < cnt;
    }
};

// Slot r of the drain list after the drain, kept when its call answered and
// its round slot has requests behind that call: the next round's slots.
struct SvNext {
    const uint32_t *dlist, *dpos; // the drain list and each slot's round slot
    uint32_t n;
    const uint8_t *d_status; // the drain's column
    const uint32_t *hit;
    SvList l;

    __device__ __forceinline__ bool entry(uint32_t r, bool, uint32_t *id, uint32_t *col) const
    {
        const uint32_t i = dlist[r];
        *id = i;
        *col = r;
        if (i >= n) return false;
        const uint32_t k = dpos[r];
        const uint32_t end = l.beg[k] + (l.off[k + 1] - l.off[k]);
        return d_status[r] != (uint8_t)MK_ST_BUDGET && hit[k] + 1u < end;
    }
};

// The round's compact words to the callers' positions; busy (when given) is set
// when the first request of a slot reports MK_ST_CALL_OPEN.
__global__ void __launch_bounds__(kRgBlock)
    sv_fold(SvList l, uint32_t len, const uint32_t *__restrict__ perm, uint32_t tot,
            const int32_t *__restrict__ c_out, const uint8_t *__restrict__ c_status,
            const uint32_t *__restrict__ c_steps, int32_t *__restrict__ out, uint8_t *__restrict__ status,
            uint32_t *__restrict__ steps, uint32_t *busy)
{
    const uint64_t q64 = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    const uint32_t R = l.off[len] < tot ? l.off[len] : tot;
    if (q64 >= R) return;
    const uint32_t q = (uint32_t)q64, k = sv_slot(l.off, len, q), o0 = l.off[k];
    const uint64_t sp = (uint64_t)l.beg[k] + (q - o0);
    if (sp >= tot) return; // holds for a list made here
    const uint32_t j = perm[sp];
    if (j >= tot) return;
    const uint8_t st = c_status[q];
    const bool first_open = c_status[o0] == (uint8_t)MK_ST_CALL_OPEN;
    const bool behind = st == (uint8_t)MK_ST_CALL_OPEN && !first_open; // not run: a later round may
    out[j] = behind ? 0 : c_out[q];
    status[j] = st;
    if (steps) steps[j] = behind ? 0u : c_steps[q];
    if (busy && first_open && q == o0) *busy = 1u;
}

// The drained calls' answers to their requests' positions, and the calls left
// open added to the serve's count.
__global__ void __launch_bounds__(kRgBlock)
    sv_advance(const uint32_t *__restrict__ dlist, const uint32_t *__restrict__ dpos, uint32_t dlen, uint32_t n,
               const uint32_t *__restrict__ hit, const uint32_t *__restrict__ perm, uint32_t tot,
               const int32_t *__restrict__ d_out, const uint8_t *__restrict__ d_status,
               const uint32_t *__restrict__ d_steps, int32_t *__restrict__ out, uint8_t *__restrict__ status,
               uint32_t *__restrict__ steps, uint32_t *cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[kOpen] += cnt[kStill];
    if (r >= dlen || dlist[r] >= n) return;
    const uint32_t sp = hit[dpos[r]];
    if (sp >= tot) return;
    const uint32_t j = perm[sp];
    if (j >= tot) return;
    out[j] = d_out[r];
    status[j] = d_status[r];
    if (steps) steps[j] = d_steps[r];
}

// beg and the request counts of the next round list (nsel, with npos[k] the
// drain slot it was taken from), nlen + 1 words: the last count is 0, so the
// scan of the counts leaves the number of requests in off[nlen].
__global__ void __launch_bounds__(kRgBlock)
    sv_next(const uint32_t *__restrict__ nsel, const uint32_t *__restrict__ npos, uint32_t nlen, uint32_t n,
            const uint32_t *__restrict__ dpos, const uint32_t *__restrict__ hit, SvList l,
            uint32_t *__restrict__ nbeg, uint32_t *__restrict__ noff)
{
    const uint64_t t = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (t > nlen) return;
    uint32_t b = 0, c = 0;
    if (t < nlen && nsel[t] < n) {
        const uint32_t k = dpos[npos[t]];
        b = hit[k] + 1u;
        c = l.beg[k] + (l.off[k + 1] - l.off[k]) - b;
    }
    noff[t] = c;
    if (t < nlen) nbeg[t] = b;
}

// the compact inputs of the round over l, out of the sorted ones
__global__ void __launch_bounds__(kRgBlock)
    sv_gather(SvList l, uint32_t len, const int64_t *__restrict__ in_sorted, uint32_t tot, int64_t *__restrict__ c_in)
{
    const uint64_t q64 = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    const uint32_t R = l.off[len] < tot ? l.off[len] : tot;
    if (q64 >= R) return;
    const uint32_t q = (uint32_t)q64, k = sv_slot(l.off, len, q);
    const uint64_t sp = (uint64_t)l.beg[k] + (q - l.off[k]);
    c_in[q] = sp < tot ? in_sorted[sp] : 0;
}

// The end of a device serve: the requests of the list no round ran report
// 0 / 0 / 0, and left[0..2) (when given) = the calls left open, the requests
// unserved.
__global__ void __launch_bounds__(kRgBlock)
    sv_unserved(SvList l, uint32_t len, const uint32_t *__restrict__ perm, uint32_t tot, int32_t *__restrict__ out,
                uint8_t *__restrict__ status, uint32_t *__restrict__ steps, const uint32_t *__restrict__ cnt,
                uint32_t *left)
{
    const uint64_t q64 = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    const uint32_t R = l.off[len] < tot ? l.off[len] : tot;
    if (left && blockIdx.x == 0 && threadIdx.x == 0) {
        left[0] = cnt[kOpen];
        left[1] = R;
    }
    if (q64 >= R) return;
    const uint32_t q = (uint32_t)q64, k = sv_slot(l.off, len, q);
    const uint64_t sp = (uint64_t)l.beg[k] + (q - l.off[k]);
    if (sp >= tot) return;
    const uint32_t j = perm[sp];
    if (j >= tot) return;
    out[j] = 0;
    status[j] = (uint8_t)0;
    if (steps) steps[j] = 0u;
}

inline unsigned sv_blocks(uint64_t threads) { return (unsigned)((threads + kRgBlock - 1) / kRgBlock); }

} // namespace sv
} // namespace mk
