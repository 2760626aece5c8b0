// sess_dir.h -- the directory of a session set: 64-bit client keys to
// instances, with admission and release (mk_session_dir_open and what follows
// it in include/mk.h).
//
//   tkey/tval  an open-addressing table of `slots` slots (a power of two, at
//              least 2n), linear probing from sd_home(key).  A slot whose key
//              is MK_KEY_NONE is free: never used since the last rebuild when
//              its value is kEmpty, a tombstone otherwise (a release leaves the
//              stale instance number there).  A probe for a key ends at the
//              key, at a never-used slot, or after `slots` steps.
//   owner[n]   the key of every instance, MK_KEY_NONE for a free one
//   fifo[n]    the free instances, a ring: w[kHead] its front, w[kFree] its length
//   w[]        the counters (the k... words below)
//
// A bind is kernels in a row, each one reading what the one before wrote:
//   sd_bind_find    a request whose key is bound gets its instance.  The others
//                   meet in a scratch table of at least 2 * total slots that
//                   holds only this queue's unbound keys: a 64-bit
//                   compare-and-swap claims a slot for a key, and an atomicMin
//                   leaves the arrival position of the key's first request there
//   sd_bind_flag    1 for the request that is the first of a new key; the
//                   exclusive scan of the flags (rg_scan) is the key's rank
//                   among the new keys, the sum their number
//   sd_bind_assign  the key of rank r takes fifo[head + r] while r < free: a
//                   slot of the directory is claimed for it (a never-used one
//                   or a tombstone: the key is known to be absent), owner[] and
//                   the scratch slot get the instance.  Past the FIFO's end the
//                   scratch slot gets "none", and the directory is not touched:
//                   a rejected key leaves no trace in it
//   sd_bind_answer  every request of a new key reads its key's scratch slot, and
//                   puts the slot back to empty: the scratch is clean between binds
//   sd_bind_finish  one thread: head, free, live and the three counts
// Which slot a key gets depends on the order the claims land in, in both tables;
// nothing else does: ranks come from arrival positions, instances from ranks.
//
// A release finds the listed keys (sd_rel_find; among repeats the one whose
// compare-and-swap clears owner[] wins), frees their slots (sd_rel_apply),
// brings the released instances into increasing order with the queue grouping
// (rg_group: distinct, sorted, padded), resets them with the indexed reset's
// kernel, appends them to the ring (sd_rel_push) and counts (sd_rel_finish).
// Tombstones only come from releases; the host keeps an upper bound of their
// number (the keys listed, bound or not) and queues a rebuild (sd_clear,
// sd_rebuild: every owner[] re-inserted into an empty table) behind the
// release that takes the bound past a quarter of the table, so that at most
// three quarters of the slots are ever in use and the rebuilds cost a constant
// per listed key.
//
// A tracked directory (mk_session_dir_track, sess_evict.h) also has last[n],
// the use stamps: sd_bind_find stores the bind's clock value for every hit and
// sd_bind_assign for every admission, the kernels that hold the instance
// anyway.  An untracked one passes a null `last` and the stores are skipped.
//
// Every kernel writes with ordinary vector stores and atomics.  Included by
// mk_exec.hip after req_group.h; everything here is static to it.
#pragma once

namespace mk {
namespace sd {

constexpr uint64_t kNone = MK_KEY_NONE;
constexpr uint32_t kEmpty = 0xffffffffu; // tval of a slot never used since the last rebuild
constexpr uint32_t kNoId = 0xffffffffu;  // "touches no session" (the queue forms' convention)
constexpr int kSdBlock = rg::kRgBlock;
constexpr uint64_t kMaxInstances = 1ull << 30; // 2n slots in 32 bits

// the counters of a directory, 32-bit words on the device
enum : int {
    kHead = 0, // front of the ring
    kFree,     // its length
    kLive,     // bound keys
    kTomb,     // tombstones in the table
    kNew,      // a bind: the queue's new keys (the scan's sum)
    kRejReq,   // a bind: requests of rejected keys; zero between binds
    kOut0,     // the last bind's counts[3]
    kOut1,
    kOut2,
    kRel,      // a release: instances released; zero between releases
    kRelOut,   // the last release's count
    kEvOut,    // the last selection's count (sess_evict.h)
    kWords = 16
};

// the finaliser of splitmix64: every input bit reaches every output bit
__host__ __device__ inline uint64_t sd_mix(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// where a key's probe starts; mask = slots - 1
__host__ __device__ inline uint32_t sd_home(uint64_t key, uint32_t mask) { return (uint32_t)(sd_mix(key) >> 32) & mask; }

// the table for n instances: the power of two that is at least 2n
inline bool sd_slots(uint64_t n, uint32_t *slots)
{
    if (n == 0 || n > kMaxInstances) return false;
    uint64_t s = 2;
    while (s < 2 * n) s <<= 1;
    *slots = (uint32_t)s;
    return true;
}

// the scratch table of a bind of `total` requests: at least 2 * total slots,
// and never more than 2^32 (which still leaves one free for any total < 2^32)
inline uint64_t sd_scratch_slots(uint64_t total)
{
    uint64_t s = 2;
    while (s < 2 * total && s < (1ull << 32)) s <<= 1;
    return s;
}

// The instance of key k (not kNone), or kNoId; *slot is where it sits.  For
// kernels in which nobody writes the table.
__device__ __forceinline__ uint32_t sd_find(const uint64_t *__restrict__ tkey, const uint32_t *__restrict__ tval,
                                            uint32_t mask, uint64_t k, uint32_t *slot)
{
    uint32_t s = sd_home(k, mask);
    for (uint64_t step = 0; step <= mask; ++step) {
        const uint64_t c = tkey[s];
        if (c == k) {
            *slot = s;
            return tval[s];
        }
        if (c == kNone && tval[s] == kEmpty) break;
        s = (s + 1u) & mask;
    }
    return kNoId;
}

// The slot of key k (not kNone) in a table it may or may not be in yet: the
// first free slot of its probe is claimed for it, unless a peer of the same
// key got there first.  Slots only go from free to taken while claims run, so
// every thread of one key ends at the same slot.  False: `mask + 1` steps
// found neither (a table with no free slot).
__device__ __forceinline__ bool sd_claim(uint64_t *tkey, uint32_t mask, uint64_t k, uint32_t *slot)
{
    uint32_t s = sd_home(k, mask);
    for (uint64_t step = 0; step <= mask; ++step) {
        uint64_t c = __hip_atomic_load(&tkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == kNone) {
            c = atomicCAS((unsigned long long *)&tkey[s], (unsigned long long)kNone, (unsigned long long)k);
            if (c == kNone) c = k;
        }
        if (c == k) {
            *slot = s;
            return true;
        }
        s = (s + 1u) & mask;
    }
    return false;
}

// key[i] = kNone, val[i] = all ones, for i < slots: an empty table
__global__ void __launch_bounds__(kSdBlock) sd_clear(uint64_t *__restrict__ key, uint32_t *__restrict__ val, uint64_t slots)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (i >= slots) return;
    key[i] = kNone;
    val[i] = 0xffffffffu;
}

// open: every instance free, the ring 0, 1, ..., n-1
__global__ void __launch_bounds__(kSdBlock)
    sd_open(uint64_t *__restrict__ owner, uint32_t *__restrict__ fifo, uint32_t n, uint32_t *__restrict__ w)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (i < (uint64_t)kWords) w[i] = i == (uint64_t)kFree ? n : 0u;
    if (i >= n) return;
    owner[i] = kNone;
    fifo[i] = (uint32_t)i;
}

// every bound instance into the (empty) table
__global__ void __launch_bounds__(kSdBlock)
    sd_rebuild(const uint64_t *__restrict__ owner, uint32_t n, uint64_t *tkey, uint32_t *__restrict__ tval, uint32_t mask,
               uint32_t *__restrict__ w)
{
    const uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (i == 0) w[kTomb] = 0u;
    if (i >= n) return;
    const uint64_t k = owner[i];
    uint32_t slot;
    if (k != kNone && sd_claim(tkey, mask, k, &slot)) tval[slot] = (uint32_t)i;
}

// ---- lookup ---------------------------------------------------------------------
__global__ void __launch_bounds__(kSdBlock)
    sd_lookup(const uint64_t *__restrict__ keys, uint32_t total, const uint64_t *__restrict__ tkey,
              const uint32_t *__restrict__ tval, uint32_t mask, uint32_t *__restrict__ ids)
{
    const uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (j >= total) return;
    const uint64_t k = keys[j];
    uint32_t slot;
    ids[j] = k == kNone ? kNoId : sd_find(tkey, tval, mask, k, &slot);
}

// ---- bind -----------------------------------------------------------------------
// The arrays of one bind; rslot and rank have `total` words each.
struct SdBind {
    const uint64_t *keys;
    uint32_t total;
    uint32_t *ids;
    uint32_t *rslot, *rank;                // a new key's request: its scratch slot; flag, then rank
    uint64_t *skey;                        // the scratch table
    uint32_t *sfirst, *sinst;
    uint32_t smask;
    uint64_t *tkey;                        // the directory
    uint32_t *tval;
    uint32_t mask;
    uint64_t *owner;
    const uint32_t *fifo;
    uint32_t n;
    uint32_t *w;
    uint64_t *last; // a tracked directory's use stamps (sess_evict.h), or null
    uint64_t now;   // what this bind stamps
};

// request j is one of a new key: not bound (sd_bind_find left kNoId) and not "no key"
__device__ __forceinline__ bool sd_is_new(const SdBind &b, uint64_t j) { return b.ids[j] == kNoId && b.keys[j] != kNone; }

__global__ void __launch_bounds__(kSdBlock) sd_bind_find(SdBind b)
{
    const uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (j >= b.total) return;
    const uint64_t k = b.keys[j];
    uint32_t id = kNoId, slot;
    if (k != kNone) {
        id = sd_find(b.tkey, b.tval, b.mask, k, &slot);
        // several requests of one key store the same value
        if (id < b.n && b.last) b.last[id] = b.now;
        if (id == kNoId) {
            // more slots than requests: the claim finds one
            (void)sd_claim(b.skey, b.smask, k, &slot);
            b.rslot[j] = slot;
            atomicMin(&b.sfirst[slot], (uint32_t)j);
        }
    }
    b.ids[j] = id;
}

__global__ void __launch_bounds__(kSdBlock) sd_bind_flag(SdBind b)
{
    const uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (j >= b.total) return;
    b.rank[j] = sd_is_new(b, j) && b.sfirst[b.rslot[j]] == (uint32_t)j ? 1u : 0u;
}

__global__ void __launch_bounds__(kSdBlock) sd_bind_assign(SdBind b)
{
    const uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool tomb = false;
    if (j < b.total && sd_is_new(b, j)) {
        const uint32_t rs = b.rslot[j];
        if (b.sfirst[rs] == (uint32_t)j) {
            const uint32_t r = b.rank[j];
            uint32_t inst = kNoId, slot;
            if (r < b.w[kFree]) {
                const uint32_t cand = b.fifo[((uint64_t)b.w[kHead] + r) % b.n];
                const uint64_t k = b.keys[j];
                // Live keys fill at most half the table, so a free slot is there, and
                // the ring holds instance numbers only.  sd_bind_finish relies on both:
                // it counts every key of rank < free as admitted and moves the head past
                // its instance without asking whether this branch was taken.
                if (cand < b.n && sd_claim(b.tkey, b.mask, k, &slot)) {
                    inst = cand;
                    tomb = b.tval[slot] != kEmpty;
                    b.tval[slot] = inst;
                    b.owner[inst] = k;
                    if (b.last) b.last[inst] = b.now;
                }
            }
            b.sinst[rs] = inst;
        }
    }
    // one subtraction per wave; counting needs no order
    const uint64_t used = __ballot(tomb);
    if (used && lane == __ffsll((unsigned long long)used) - 1) atomicSub(&b.w[kTomb], (uint32_t)__popcll(used));
}

__global__ void __launch_bounds__(kSdBlock) sd_bind_answer(SdBind b)
{
    __shared__ uint32_t wsum[rg::kRgWaves];
    const uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    uint32_t rej = 0;
    if (j < b.total && sd_is_new(b, j)) {
        const uint32_t rs = b.rslot[j];
        const uint32_t id = b.sinst[rs];
        b.ids[j] = id;
        rej = id == kNoId ? 1u : 0u;
        // every request of the key stores the same two values
        b.skey[rs] = kNone;
        b.sfirst[rs] = 0xffffffffu;
    }
    uint32_t all;
    (void)rg::rg_block_scan(rej, wsum, &all);
    if (threadIdx.x == 0 && all) atomicAdd(&b.w[kRejReq], all);
}

// one thread: the ring's front moves past the admitted keys' instances
__global__ void sd_bind_finish(uint32_t *__restrict__ w, uint32_t n, uint32_t *__restrict__ counts)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t fresh = w[kNew], avail = w[kFree];
    const uint32_t adm = fresh < avail ? fresh : avail;
    w[kHead] = (uint32_t)(((uint64_t)w[kHead] + adm) % n);
    w[kFree] = avail - adm;
    w[kLive] += adm;
    const uint32_t c0 = adm, c1 = fresh - adm, c2 = w[kRejReq];
    w[kRejReq] = 0u;
    w[kOut0] = c0;
    w[kOut1] = c1;
    w[kOut2] = c2;
    if (counts) {
        counts[0] = c0;
        counts[1] = c1;
        counts[2] = c2;
    }
}

inline unsigned sd_blocks(uint64_t count) { return (unsigned)((count + kSdBlock - 1) / kSdBlock); }
inline int sd_launched() { return hipGetLastError() == hipSuccess ? (int)MK_OK : (int)MK_EDEVICE; }

// the scratch of binds of up to `cap` requests
struct SdBindBufs {
    uint32_t *rslot, *rank, *sums;
    uint64_t *skey;
    uint32_t *sfirst, *sinst;
    uint64_t sslots;
    size_t bytes;
};

inline SdBindBufs sd_bind_layout(size_t cap, void *base)
{
    Carver k(base);
    SdBindBufs q{};
    q.sslots = sd_scratch_slots(cap);
    q.rslot = k.take<uint32_t>(cap);
    q.rank = k.take<uint32_t>(cap);
    q.sums = k.take<uint32_t>(rg::rg_scan_blocks(cap));
    q.skey = k.take<uint64_t>(q.sslots);
    q.sfirst = k.take<uint32_t>(q.sslots);
    q.sinst = k.take<uint32_t>(q.sslots);
    q.bytes = k.at;
    return q;
}

// The kernels of a bind on `st`; b complete, total in [1, 2^32).  The scratch
// table must be empty, and is again when all of this has run.  In two halves:
// after the first w[kNew] is known on the device, and a bind that makes room
// (sess_evict.h) frees instances between them.
inline int sd_bind_front(const SdBind &b, uint32_t *sums, hipStream_t st)
{
    const dim3 grid(sd_blocks(b.total)), blk(kSdBlock);
    hipLaunchKernelGGL(sd_bind_find, grid, blk, 0, st, b);
    hipLaunchKernelGGL(sd_bind_flag, grid, blk, 0, st, b);
    if (int rc = sd_launched()) return rc;
    return rg::rg_scan(b.rank, b.total, sums, b.w + kNew, st);
}

inline int sd_bind_back(const SdBind &b, uint32_t *d_counts, hipStream_t st)
{
    const dim3 grid(sd_blocks(b.total)), blk(kSdBlock);
    hipLaunchKernelGGL(sd_bind_assign, grid, blk, 0, st, b);
    hipLaunchKernelGGL(sd_bind_answer, grid, blk, 0, st, b);
    hipLaunchKernelGGL(sd_bind_finish, dim3(1), dim3(64), 0, st, b.w, b.n, d_counts);
    return sd_launched();
}

// ---- release --------------------------------------------------------------------
// rinst[t] = the instance key t frees, kNoId for no key, an unbound key and a
// repeat that lost; rslot[t] its slot
__global__ void __launch_bounds__(kSdBlock)
    sd_rel_find(const uint64_t *__restrict__ keys, uint32_t m, const uint64_t *__restrict__ tkey,
                const uint32_t *__restrict__ tval, uint32_t mask, uint64_t *owner, uint32_t n,
                uint32_t *__restrict__ rinst, uint32_t *__restrict__ rslot)
{
    const uint64_t t = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (t >= m) return;
    const uint64_t k = keys[t];
    uint32_t id = kNoId, slot = 0;
    if (k != kNone) {
        id = sd_find(tkey, tval, mask, k, &slot);
        if (id >= n) id = kNoId;
        else if (atomicCAS((unsigned long long *)&owner[id], (unsigned long long)k, (unsigned long long)kNone) != k)
            id = kNoId;
    }
    rinst[t] = id;
    rslot[t] = slot;
}

// the slots of the released keys become tombstones (tval keeps the stale instance)
__global__ void __launch_bounds__(kSdBlock)
    sd_rel_apply(const uint32_t *__restrict__ rinst, const uint32_t *__restrict__ rslot, uint32_t m,
                 uint64_t *__restrict__ tkey, uint32_t *__restrict__ w)
{
    __shared__ uint32_t wsum[rg::kRgWaves];
    const uint64_t t = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    const bool won = t < m && rinst[t] != kNoId;
    if (won) tkey[rslot[t]] = kNone;
    uint32_t all;
    (void)rg::rg_block_scan(won ? 1u : 0u, wsum, &all);
    if (threadIdx.x == 0 && all) atomicAdd(&w[kRel], all);
}

// sel[0..*count): the released instances, increasing, to the back of the ring
__global__ void __launch_bounds__(kSdBlock)
    sd_rel_push(const uint32_t *__restrict__ sel, const uint32_t *__restrict__ count, uint32_t cap,
                uint32_t *__restrict__ fifo, uint32_t n, const uint32_t *__restrict__ w)
{
    const uint64_t t = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (t >= cap || t >= *count) return;
    const uint32_t i = sel[t];
    if (i < n) fifo[((uint64_t)w[kHead] + w[kFree] + t) % n] = i;
}

__global__ void sd_rel_finish(uint32_t *__restrict__ w, uint32_t *__restrict__ released)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t r = w[kRel];
    w[kRel] = 0u;
    w[kFree] += r;
    w[kLive] -= r;
    w[kTomb] += r;
    w[kRelOut] = r;
    if (released) *released = r;
}

// the scratch of releases of up to `cap` keys from a set of n instances
struct SdRelBufs {
    uint32_t *rinst, *rslot, *perm, *sel, *off, *count;
    void *tmp;
    size_t bytes;
};

inline SdRelBufs sd_rel_layout(size_t n, size_t cap, void *base)
{
    const size_t M = cap < n ? cap : n;
    Carver k(base);
    SdRelBufs q{};
    q.rinst = k.take<uint32_t>(cap);
    q.rslot = k.take<uint32_t>(cap);
    q.perm = k.take<uint32_t>(cap);
    q.sel = k.take<uint32_t>(M);
    q.off = k.take<uint32_t>(M + 1);
    q.count = k.take<uint32_t>(1);
    q.tmp = k.take<char>(rg::rg_tmp_layout(cap).bytes);
    q.bytes = k.at;
    return q;
}

// ---- what a set holds of its directory (host) --------------------------------------
struct SdDir {
    uint32_t slots = 0;
    void *d_base = nullptr; // tkey, tval, owner, fifo and w, one allocation
    uint64_t *tkey = nullptr, *owner = nullptr;
    uint32_t *tval = nullptr, *fifo = nullptr, *w = nullptr;
    uint32_t *h_w = nullptr; // pinned: the words a host form reads back
    // the binds' and the releases' scratch, grown on demand
    void *d_bind = nullptr, *d_rel = nullptr;
    size_t bind_cap = 0, rel_cap = 0;
    bool bind_dirty = false; // a bind failed part way: its scratch table is cleared before the next
    uint64_t tomb_bound = 0; // no more tombstones than this are in the table
    // use stamps (mk_session_dir_track, sess_evict.h): null until tracked
    void *d_ev = nullptr;     // last[n] first, then the selection's scratch
    uint64_t *last = nullptr;
    uint64_t clock = 0;       // binds queued since tracking began
};

inline size_t sd_dir_carve(SdDir *d, size_t n, void *base)
{
    Carver k(base);
    d->tkey = k.take<uint64_t>(d->slots);
    d->tval = k.take<uint32_t>(d->slots);
    d->owner = k.take<uint64_t>(n);
    d->fifo = k.take<uint32_t>(n);
    d->w = k.take<uint32_t>(kWords);
    return k.at;
}

// Caller: device current, nothing of the directory in flight.
inline void sd_dir_free(SdDir *d)
{
    if (!d) return;
    (void)hipFree(d->d_base);
    (void)hipFree(d->d_bind);
    (void)hipFree(d->d_rel);
    (void)hipFree(d->d_ev);
    (void)hipHostFree(d->h_w);
    delete d;
}

} // namespace sd
} // namespace mk
