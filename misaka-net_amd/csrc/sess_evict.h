// sess_evict.h -- which clients of a tracked directory have been silent
// longest, and their eviction (mk_session_dir_track and what follows it in
// include/mk.h).
//
//   last[n]  the use stamp of every instance: the directory's clock (binds
//            queued since tracking began) as the last bind that resolved to it
//            ran.  sd_bind_find stamps hits, sd_bind_assign admissions.
//   age(i)   min(clock - last[i], 2^32 - 1)
//   eligible bound, age >= max(min_idle, 1), no call open (io bit 3)
//   the k most idle: the first k eligible by (age descending, instance
//            ascending), reported in increasing instance order
//
// The selection never sorts.  ev_begin puts k into ctl[] (for a bind that makes
// room: min(new - free, max_evict), both known on the device by then), and
// every kernel over the n instances reads that word first and returns when it
// is 0.  Then
//   ev_hist<true>  the eligible ages into age[] (0: not eligible), their top
//                  digit counted per block in LDS, one word per (digit, block)
//                  as rg_hist lays them out; the OR and the AND of the ages
//   ev_narrow      one block: the digits' totals, scanned from 255 down; the
//                  digit in which the k-th oldest falls joins the prefix, and
//                  k shrinks by the number above it.  The first one also caps
//                  k at the number eligible.
//   ev_hist<false> the next digit of the ages that share the prefix, and
//   ev_narrow      again, three times: after the fourth digit the prefix is
//                  the threshold age T and ctl[cLeft] how many of age T go.  A
//                  digit in which OR and AND agree is the same for every
//                  eligible age: both kernels of that pass return at once.
//   ev_count       per tile of 2048 instances, how many are older than T and
//                  how many are of age T; one scan (rg_scan) over both rows
//   ev_write       the stable compaction: an instance older than T goes to
//                  (older before it) + min(ties before it, left), one of age T
//                  with fewer than `left` ties before it to (older before it)
//                  + (ties before it).  Increasing instance order, ties broken
//                  by instance number, no atomics.
//   ev_tail        pads the lists to their capacity and reports the count
// An eviction goes on with ev_release (slot to tombstone, owner[] cleared, the
// instance to the back of the ring at head + free + its rank), the indexed
// reset's kernel over the list, and ev_finish (free, live, tombstones).
//
// Passes over the n instances: the first reads owner, last and io (20 bytes an
// instance) and writes age (4); each further pass reads age only.
//
// Every kernel writes with ordinary vector stores and atomics; a value one
// thread writes for the block is written under `if (threadIdx.x == ...)`.
// Included by mk_exec.hip after sess_dir.h; everything here is static to it.
#pragma once

namespace mk {
namespace ev {

using rg::kDigits;
using rg::kRgBlock;
using rg::kRgRounds;
using rg::kRgWaves;
using rg::kTile;

constexpr uint32_t kEvMaxGrid = 2048; // blocks of a kernel over n; the tiles beyond are strided
constexpr int kEvPasses = 4;          // 8-bit digits of a 32-bit age

// the words of a selection, on the device
enum : int {
    cK = 0,  // how many to select; 0: every kernel over n returns
    cPrefix, // the digits of the threshold age found so far
    cLeft,   // how many of the prefix's class are still to take
    cOr,     // the OR and the AND of the eligible ages
    cAnd,
    cElig,  // how many are eligible
    cCount, // how many are selected: min(k, eligible)
    cWords = 8
};

struct EvSrc {
    const uint64_t *owner, *last;
    const uint32_t *io;
    uint32_t n;
    uint64_t clock;
    uint32_t min_idle; // at least 1
};

// the age of instance i < n when it is eligible, 0 otherwise
__device__ __forceinline__ uint32_t ev_age(const EvSrc &s, uint64_t i)
{
    if (s.owner[i] == sd::kNone || ((s.io[i] >> 3) & 1u)) return 0u;
    const uint64_t l = s.last[i];
    if (l >= s.clock) return 0u;
    const uint64_t a = s.clock - l;
    const uint32_t a32 = a > 0xffffffffull ? 0xffffffffu : (uint32_t)a;
    return a32 >= s.min_idle ? a32 : 0u;
}

// every eligible age has the same digit at `shift`
__device__ __forceinline__ bool ev_uniform(uint32_t o, uint32_t a, uint32_t shift) { return (((o ^ a) >> shift) & (kDigits - 1u)) == 0u; }

// last[i] = value for a bound instance, 0 for a free one
__global__ void __launch_bounds__(kRgBlock)
    ev_stamp_bound(const uint64_t *__restrict__ owner, uint64_t *__restrict__ last, uint32_t n, uint64_t value)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kRgBlock)
        last[i] = owner[i] == sd::kNone ? 0ull : value;
}

// One thread: a selection begins.  from_bind: k is what the bind in progress
// lacks (w[kNew] is its scan's sum), at most `want`.
__global__ void ev_begin(uint32_t *__restrict__ ctl, const uint32_t *__restrict__ w, uint32_t want, int from_bind)
{
    if (blockIdx.x || threadIdx.x) return;
    uint32_t k = want;
    if (from_bind) {
        const uint32_t fresh = w[sd::kNew], avail = w[sd::kFree];
        const uint32_t need = fresh > avail ? fresh - avail : 0u;
        k = need < want ? need : want;
    }
    ctl[cK] = k;
    ctl[cPrefix] = 0u;
    ctl[cLeft] = 0u;
    ctl[cOr] = 0u;
    ctl[cAnd] = 0xffffffffu;
    ctl[cElig] = 0u;
    ctl[cCount] = 0u;
}

// table[d * gridDim.x + block] = how many of the block's tiles' eligible ages
// in the prefix's class have digit d at pass `pass` (0: the top one)
template <bool FIRST>
__global__ void __launch_bounds__(kRgBlock)
    ev_hist(EvSrc s, uint32_t *__restrict__ age, uint32_t pass, uint32_t ntiles, uint32_t *__restrict__ table,
            uint32_t *__restrict__ ctl)
{
    __shared__ uint32_t hist[kDigits];
    __shared__ uint32_t s_or, s_and;
    if (ctl[cK] == 0u) return;
    const uint32_t shift = 24u - 8u * pass;
    if (!FIRST && ev_uniform(ctl[cOr], ctl[cAnd], shift)) return;
    const uint32_t prefix = ctl[cPrefix];
    const int tid = threadIdx.x, lane = tid & 63;
    hist[tid] = 0u;
    if (tid == 0) {
        s_or = 0u;
        s_and = 0xffffffffu;
    }
    __syncthreads();
    uint32_t vo = 0u, va = 0xffffffffu;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int r = 0; r < kRgRounds; ++r) {
            const uint64_t i = (uint64_t)tile * kTile + (uint32_t)(r * kRgBlock + tid);
            const bool act = i < s.n;
            uint32_t a = 0u;
            if (act) {
                if (FIRST) {
                    a = ev_age(s, i);
                    age[i] = a;
                } else {
                    a = age[i];
                }
            }
            // FIRST: shift + 8 is 32, and every eligible age is in the class
            const bool in = a != 0u && (FIRST || (a >> (shift + 8u)) == (prefix >> (shift + 8u)));
            const uint32_t d = (a >> shift) & (kDigits - 1u);
            const uint64_t peers = rg::rg_peers(d, in);
            // one add per wave and digit; counting needs no order
            if (in && (peers & rg::rg_below(lane)) == 0u) atomicAdd(&hist[d], (uint32_t)__popcll(peers));
            if (FIRST && in) {
                vo |= a;
                va &= a;
            }
        }
    }
    if (FIRST) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            vo |= __shfl_xor(vo, d, 64);
            va &= __shfl_xor(va, d, 64);
        }
        if (lane == 0) {
            atomicOr(&s_or, vo);
            atomicAnd(&s_and, va);
        }
    }
    __syncthreads();
    table[(uint64_t)tid * gridDim.x + blockIdx.x] = hist[tid];
    if (FIRST && tid == 0 && s_or) { // OR and AND commute: no order matters
        atomicOr(&ctl[cOr], s_or);
        atomicAnd(&ctl[cAnd], s_and);
    }
}

// One block: thread t owns digit 255 - t, so that the block's scan counts the
// ages above a digit.
__global__ void __launch_bounds__(kRgBlock)
    ev_narrow(const uint32_t *__restrict__ table, uint32_t grid, uint32_t pass, uint32_t *__restrict__ ctl)
{
    __shared__ uint32_t wsum[kRgWaves];
    __shared__ uint32_t s_digit, s_left;
    const uint32_t k0 = ctl[cK];
    if (k0 == 0u) return;
    const uint32_t shift = 24u - 8u * pass;
    const uint32_t prefix = ctl[cPrefix], left = ctl[cLeft], o = ctl[cOr], a = ctl[cAnd];
    if (pass && ev_uniform(o, a, shift)) {
        __syncthreads(); // every thread has read the prefix
        if (threadIdx.x == 0) ctl[cPrefix] = prefix | (o & ((kDigits - 1u) << shift));
        return;
    }
    const uint32_t d = kDigits - 1u - (uint32_t)threadIdx.x;
    uint32_t tot = 0;
    for (uint32_t b = 0; b < grid; ++b) tot += table[(uint64_t)d * grid + b];
    uint32_t all;
    const uint32_t above = rg::rg_block_scan(tot, wsum, &all); // its barriers: every thread has read ctl
    const uint32_t k = pass ? left : (k0 < all ? k0 : all);
    // exactly one digit holds the k-th oldest (none when k is 0)
    if (k && above < k && k <= above + tot) {
        s_digit = d;
        s_left = k - above;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (pass == 0u) {
            ctl[cElig] = all;
            ctl[cK] = k;
            ctl[cCount] = k;
        }
        if (k) {
            ctl[cPrefix] = prefix | (s_digit << shift);
            ctl[cLeft] = s_left;
        }
    }
}

// cnt[tile] = the tile's instances older than the threshold, cnt[ntiles + tile]
// = those at it
__global__ void __launch_bounds__(kRgBlock)
    ev_count(const uint32_t *__restrict__ age, uint32_t n, uint32_t ntiles, const uint32_t *__restrict__ ctl,
             uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t wsum[kRgWaves];
    if (ctl[cK] == 0u) return;
    const uint32_t T = ctl[cPrefix];
    const int tid = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint32_t v = 0; // older in the low half, ties in the high: at most kTile of each
        for (int r = 0; r < kRgRounds; ++r) {
            const uint64_t i = (uint64_t)tile * kTile + (uint32_t)(r * kRgBlock + tid);
            const uint32_t a = i < n ? age[i] : 0u;
            v += a > T ? 1u : (a == T ? 0x10000u : 0u);
        }
        uint32_t all;
        (void)rg::rg_block_scan(v, wsum, &all);
        if (tid == 0) {
            cnt[tile] = all & 0xffffu;
            cnt[ntiles + tile] = all >> 16;
        }
    }
}

// cnt scanned as one array: cnt[ntiles] is the number older than the threshold
__global__ void __launch_bounds__(kRgBlock)
    ev_write(const uint64_t *__restrict__ owner, const uint32_t *__restrict__ age, uint32_t n, uint32_t ntiles,
             const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ cnt, uint32_t cap,
             uint32_t *__restrict__ sel, uint32_t *__restrict__ ids, uint64_t *__restrict__ keys)
{
    __shared__ uint32_t wsum[kRgWaves];
    if (ctl[cK] == 0u) return;
    const uint32_t T = ctl[cPrefix], left = ctl[cLeft], older_all = cnt[ntiles];
    const int tid = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint32_t bo = cnt[tile], bt = cnt[ntiles + tile] - older_all;
        for (int r = 0; r < kRgRounds; ++r) {
            const uint64_t i = (uint64_t)tile * kTile + (uint32_t)(r * kRgBlock + tid);
            const uint32_t a = i < n ? age[i] : 0u;
            const bool older = a > T, tie = a == T; // T >= 1: a free or busy instance is neither
            uint32_t all;
            const uint32_t x = rg::rg_block_scan(older ? 1u : (tie ? 0x10000u : 0u), wsum, &all);
            const uint32_t o_r = bo + (x & 0xffffu), t_r = bt + (x >> 16);
            if (older || (tie && t_r < left)) {
                const uint32_t pos = o_r + (t_r < left ? t_r : left);
                if (pos < cap) { // holds: older_all + left is the count, at most cap
                    sel[pos] = (uint32_t)i;
                    if (ids) ids[pos] = (uint32_t)i;
                    if (keys) keys[pos] = owner[i];
                }
            }
            bo += all & 0xffffu;
            bt += all >> 16;
        }
    }
}

// the padded tails of the lists, and the count where it is read
__global__ void __launch_bounds__(kRgBlock)
    ev_tail(const uint32_t *__restrict__ ctl, uint32_t cap, uint32_t *__restrict__ sel, uint32_t *__restrict__ ids,
            uint64_t *__restrict__ keys, uint32_t *__restrict__ w, uint32_t *__restrict__ count_out)
{
    const uint64_t t = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    const uint32_t c = ctl[cCount];
    if (t == 0) {
        w[sd::kEvOut] = c;
        if (count_out) *count_out = c;
    }
    if (t >= cap || t < c) return;
    sel[t] = sd::kNoId;
    if (ids) ids[t] = sd::kNoId;
    if (keys) keys[t] = sd::kNone;
}

// The slot of key k, which is in the table.  Other threads turn other keys'
// slots into tombstones meanwhile: a probe passes those either way.
__device__ __forceinline__ bool ev_slot_of(uint64_t *tkey, const uint32_t *tval, uint32_t mask, uint64_t k, uint32_t *slot)
{
    uint32_t s = sd::sd_home(k, mask);
    for (uint64_t step = 0; step <= mask; ++step) {
        const uint64_t c = __hip_atomic_load(&tkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == k) {
            *slot = s;
            return true;
        }
        if (c == sd::kNone && tval[s] == sd::kEmpty) break;
        s = (s + 1u) & mask;
    }
    return false;
}

// sel[0..count): distinct and increasing.  Each one's slot becomes a tombstone,
// its owner[] is cleared, and it goes to the back of the ring.
__global__ void __launch_bounds__(kRgBlock)
    ev_release(const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ sel, uint32_t cap, uint64_t *tkey,
               const uint32_t *__restrict__ tval, uint32_t mask, uint64_t *__restrict__ owner,
               uint32_t *__restrict__ fifo, uint32_t n, const uint32_t *__restrict__ w)
{
    const uint64_t t = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (t >= cap || t >= ctl[cCount]) return;
    const uint32_t i = sel[t];
    if (i >= n) return;
    const uint64_t k = owner[i];
    uint32_t slot;
    if (k != sd::kNone && ev_slot_of(tkey, tval, mask, k, &slot)) tkey[slot] = sd::kNone;
    owner[i] = sd::kNone;
    fifo[((uint64_t)w[sd::kHead] + w[sd::kFree] + t) % n] = i;
}

__global__ void ev_finish(const uint32_t *__restrict__ ctl, uint32_t *__restrict__ w)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t c = ctl[cCount];
    w[sd::kFree] += c;
    w[sd::kLive] -= c;
    w[sd::kTomb] += c;
}

// what a tracked directory of n instances holds on the device, one allocation
struct EvBufs {
    uint64_t *last;
    uint32_t *age, *table, *cnt, *sums, *sel, *ctl;
    uint32_t ntiles, grid;
    size_t bytes;
};

inline EvBufs ev_layout(size_t n, void *base)
{
    Carver k(base);
    EvBufs q{};
    q.ntiles = (uint32_t)((n + kTile - 1) / kTile);
    q.grid = q.ntiles < kEvMaxGrid ? q.ntiles : kEvMaxGrid;
    q.last = k.take<uint64_t>(n);
    q.age = k.take<uint32_t>(n);
    q.table = k.take<uint32_t>((size_t)kDigits * q.grid);
    q.cnt = k.take<uint32_t>((size_t)2 * q.ntiles);
    q.sums = k.take<uint32_t>(rg::rg_scan_blocks((uint64_t)2 * q.ntiles));
    q.sel = k.take<uint32_t>(n);
    q.ctl = k.take<uint32_t>(cWords);
    q.bytes = k.at;
    return q;
}

// The selection on `st`: q.sel (and ids and keys, nullable) take the victims,
// cap entries each, padded; w[kEvOut] and *count_out (nullable) their number.
// cap in [1, n]: the most to select.  from_bind: see ev_begin.
inline int ev_select(const EvSrc &s, const EvBufs &q, uint32_t cap, bool from_bind, uint32_t *ids, uint64_t *keys,
                     uint32_t *w, uint32_t *count_out, hipStream_t st)
{
    const dim3 grid(q.grid), blk(kRgBlock);
    hipLaunchKernelGGL(ev_begin, dim3(1), dim3(64), 0, st, q.ctl, (const uint32_t *)w, cap, from_bind ? 1 : 0);
    for (uint32_t p = 0; p < (uint32_t)kEvPasses; ++p) {
        if (p == 0) hipLaunchKernelGGL(ev_hist<true>, grid, blk, 0, st, s, q.age, p, q.ntiles, q.table, q.ctl);
        else hipLaunchKernelGGL(ev_hist<false>, grid, blk, 0, st, s, q.age, p, q.ntiles, q.table, q.ctl);
        hipLaunchKernelGGL(ev_narrow, dim3(1), blk, 0, st, (const uint32_t *)q.table, q.grid, p, q.ctl);
    }
    hipLaunchKernelGGL(ev_count, grid, blk, 0, st, (const uint32_t *)q.age, s.n, q.ntiles, (const uint32_t *)q.ctl,
                       q.cnt);
    if (int rc = sd::sd_launched()) return rc;
    if (int rc = rg::rg_scan(q.cnt, (uint64_t)2 * q.ntiles, q.sums, nullptr, st)) return rc;
    hipLaunchKernelGGL(ev_write, grid, blk, 0, st, s.owner, (const uint32_t *)q.age, s.n, q.ntiles,
                       (const uint32_t *)q.ctl, (const uint32_t *)q.cnt, cap, q.sel, ids, keys);
    hipLaunchKernelGGL(ev_tail, dim3(sd::sd_blocks(cap)), blk, 0, st, (const uint32_t *)q.ctl, cap, q.sel, ids, keys,
                       w, count_out);
    return sd::sd_launched();
}

} // namespace ev
} // namespace mk
