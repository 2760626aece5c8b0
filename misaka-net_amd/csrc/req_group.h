// req_group.h -- grouping a request queue on the GPU: `total` requests in
// arrival order, request j for session ids[j], become the shape a ragged
// session launch takes (mk_requests_group_device, include/mk.h).
//
//   key[j]  = min(ids[j], n)            every id that names no session is n
//   perm    = the stable order of the keys (numpy argsort, kind="stable")
//   sel/off = the distinct keys below n and where each one's run starts
//
// The sort is an LSD radix sort over the bits n has, 8 bits a pass, payload
// j (implicit on the first pass).  A tile is kTile consecutive elements, one
// block; a pass is
//   rg_hist     the tile's digit counts into table[digit][tile]
//   rg_scan_*   an exclusive scan of the whole table, in place
//   rg_scatter  every element to table[digit][tile] + its rank in the tile
// The rank of an element among its tile's equal digits orders nothing by
// atomics: the tile goes by in rounds of one block's width; in a round each
// wave finds, by eight ballots over the digit's bits, the mask of its lanes
// that hold the same digit (rg_peers) -- the rank in the wave is the popcount
// below the lane -- the waves' counts per digit meet in LDS, and a running
// per-digit base carries the rounds.  Stable: round, wave, lane is element
// order.  After the last pass rg_head_count / rg_head_write flag the first
// element of every run of the sorted keys, scan the flags the same way and
// write sel and off; rg_tail pads both to M = min(total, n) entries so that
// a launch over M entries needs no read-back of m.  A queue of one tile takes
// one launch for all of it (rg_one_tile).
//
// Every kernel writes with ordinary vector stores; a value one thread writes
// for the block is written under `if (threadIdx.x == ...)`.  Included by
// mk_exec.hip after mk.h; everything here is static to it.
#pragma once

namespace mk {
namespace rg {

constexpr int kRgBlock = 256;                  // threads of every kernel here: 4 waves of 64
constexpr int kRgWaves = kRgBlock / 64;
constexpr int kRgRounds = 8;                   // elements per thread of a tile
constexpr uint32_t kTile = kRgBlock * kRgRounds; // 2048
constexpr int kDigitBits = 8;
constexpr uint32_t kDigits = 1u << kDigitBits; // == kRgBlock: thread d owns digit d's counters
constexpr uint32_t kScanTile = kTile;          // words one block of the scan kernels covers
static_assert(kDigits == (uint32_t)kRgBlock, "thread d owns digit d");

__host__ __device__ inline uint32_t rg_bitlen(uint32_t n)
{
    uint32_t b = 0;
    while (n) {
        ++b;
        n >>= 1;
    }
    return b;
}

// The lanes of this wave that are active and hold digit d.  Called by every
// lane of the wave (inactive elements pass act false), never under divergence.
__device__ __forceinline__ uint64_t rg_peers(uint32_t d, bool act)
{
    uint64_t mask = __ballot(act);
#pragma unroll
    for (int b = 0; b < kDigitBits; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        mask &= bit ? bal : ~bal;
    }
    return mask;
}

__device__ __forceinline__ uint64_t rg_below(int lane) { return ((uint64_t)1 << lane) - 1u; }

// Exclusive prefix of v over the block's threads and, in *sum, the block's
// total.  wsum: kRgWaves words of LDS; safe to call again right away.
__device__ __forceinline__ uint32_t rg_block_scan(uint32_t v, uint32_t *wsum, uint32_t *sum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads(); // the previous call's readers are done with wsum
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kRgWaves; ++w) {
        const uint32_t s = wsum[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    *sum = all;
    return before + inc - v;
}

// Element idx of a pass's input as its key: the first pass clamps the ids.
template <bool FIRST> __device__ __forceinline__ uint32_t rg_key(const uint32_t *src, uint64_t idx, uint32_t n)
{
    const uint32_t k = src[idx];
    return FIRST ? (k < n ? k : n) : k;
}

// table[d * ntiles + tile] = how many of the tile's elements have digit d
template <bool FIRST>
__global__ void __launch_bounds__(kRgBlock)
    rg_hist(const uint32_t *__restrict__ src, uint32_t n, uint32_t total, uint32_t shift, uint32_t ntiles,
            uint32_t *__restrict__ table)
{
    __shared__ uint32_t hist[kDigits];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t tile = blockIdx.x;
    hist[tid] = 0u;
    __syncthreads();
    for (int r = 0; r < kRgRounds; ++r) {
        const uint64_t idx = (uint64_t)tile * kTile + (uint32_t)(r * kRgBlock + tid);
        const bool act = idx < total;
        const uint32_t d = act ? (rg_key<FIRST>(src, idx, n) >> shift) & (kDigits - 1u) : 0u;
        const uint64_t peers = rg_peers(d, act);
        // one add per wave and digit; counting needs no order
        if (act && (peers & rg_below(lane)) == 0u) atomicAdd(&hist[d], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    table[(uint64_t)tid * ntiles + tile] = hist[tid];
}

// ---- exclusive scan of a[0..len), in place, any len < 2^32 ------------------
// sums[b] = the sum of block b's kScanTile words
__global__ void __launch_bounds__(kRgBlock)
    rg_scan_reduce(const uint32_t *__restrict__ a, uint32_t len, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wsum[kRgWaves];
    const uint64_t at = (uint64_t)blockIdx.x * kScanTile + (uint32_t)threadIdx.x * kRgRounds;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < kRgRounds; ++i) v += at + i < len ? a[at + i] : 0u;
    uint32_t all;
    (void)rg_block_scan(v, wsum, &all);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// One chunk of kScanTile words at `base`, scanned by the block; returns the
// chunk's sum.
__device__ __forceinline__ uint32_t rg_scan_chunk(uint32_t *a, uint64_t base, uint32_t len, uint32_t carry,
                                                  uint32_t *wsum)
{
    const uint64_t at = base + (uint32_t)threadIdx.x * kRgRounds;
    uint32_t x[kRgRounds], v = 0;
#pragma unroll
    for (int i = 0; i < kRgRounds; ++i) {
        x[i] = at + i < len ? a[at + i] : 0u;
        v += x[i];
    }
    uint32_t all;
    uint32_t run = carry + rg_block_scan(v, wsum, &all);
#pragma unroll
    for (int i = 0; i < kRgRounds; ++i) {
        if (at + i < len) a[at + i] = run;
        run += x[i];
    }
    return all;
}

// one block over the whole of a[0..len), chunk after chunk with a carry;
// *sum_out (when given) = the sum of all
__global__ void __launch_bounds__(kRgBlock) rg_scan_serial(uint32_t *a, uint32_t len, uint32_t *sum_out)
{
    __shared__ uint32_t wsum[kRgWaves];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < len; base += kScanTile) carry += rg_scan_chunk(a, base, len, carry, wsum);
    if (sum_out && threadIdx.x == 0) *sum_out = carry;
}

// block b scans its chunk on top of sums[b] (already scanned)
__global__ void __launch_bounds__(kRgBlock) rg_scan_apply(uint32_t *a, uint32_t len, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wsum[kRgWaves];
    (void)rg_scan_chunk(a, (uint64_t)blockIdx.x * kScanTile, len, sums[blockIdx.x], wsum);
}

inline uint32_t rg_scan_blocks(uint64_t len) { return (uint32_t)((len + kScanTile - 1) / kScanTile); }

// Up to this many chunks one block scans alone, in one launch; more go
// through the three kernels.
constexpr uint32_t kSerialChunks = 4;

// a[0..len) scanned in place on `st`; sums: rg_scan_blocks(len) words
inline int rg_scan(uint32_t *a, uint64_t len, uint32_t *sums, uint32_t *sum_out, hipStream_t st)
{
    const uint32_t nb = rg_scan_blocks(len);
    if (nb <= kSerialChunks) {
        hipLaunchKernelGGL(rg_scan_serial, dim3(1), dim3(kRgBlock), 0, st, a, (uint32_t)len, sum_out);
    } else {
        hipLaunchKernelGGL(rg_scan_reduce, dim3(nb), dim3(kRgBlock), 0, st, a, (uint32_t)len, sums);
        hipLaunchKernelGGL(rg_scan_serial, dim3(1), dim3(kRgBlock), 0, st, sums, nb, sum_out);
        hipLaunchKernelGGL(rg_scan_apply, dim3(nb), dim3(kRgBlock), 0, st, a, (uint32_t)len, sums);
    }
    return hipGetLastError() == hipSuccess ? MK_OK : MK_EDEVICE;
}

// Every element of the tile to its place: table[digit][tile] (scanned) plus
// its rank among the tile's elements of the same digit.
template <bool FIRST>
__global__ void __launch_bounds__(kRgBlock)
    rg_scatter(const uint32_t *__restrict__ src_key, const uint32_t *__restrict__ src_perm, uint32_t n, uint32_t total,
               uint32_t shift, uint32_t ntiles, const uint32_t *__restrict__ table, uint32_t *__restrict__ dst_key,
               uint32_t *__restrict__ dst_perm)
{
    __shared__ uint32_t base[kDigits];
    __shared__ uint32_t wcnt[kRgWaves][kDigits];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = blockIdx.x;
    base[tid] = table[(uint64_t)tid * ntiles + tile];
#pragma unroll
    for (int w = 0; w < kRgWaves; ++w) wcnt[w][tid] = 0u;
    __syncthreads();
    for (int r = 0; r < kRgRounds; ++r) {
        const uint64_t idx = (uint64_t)tile * kTile + (uint32_t)(r * kRgBlock + tid);
        const bool act = idx < total;
        const uint32_t key = act ? rg_key<FIRST>(src_key, idx, n) : 0u;
        const uint32_t d = (key >> shift) & (kDigits - 1u);
        const uint64_t peers = rg_peers(d, act);
        const uint32_t rank = (uint32_t)__popcll(peers & rg_below(lane));
        if (act && rank == 0u) wcnt[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (act) {
            uint32_t pos = base[d] + rank;
#pragma unroll
            for (int w = 0; w < kRgWaves; ++w) pos += w < wave ? wcnt[w][d] : 0u;
            if (pos < total) { // holds for a table that counted these keys
                dst_key[pos] = key;
                dst_perm[pos] = FIRST ? (uint32_t)idx : src_perm[idx];
            }
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int w = 0; w < kRgWaves; ++w) {
            add += wcnt[w][tid];
            wcnt[w][tid] = 0u;
        }
        base[tid] += add;
        __syncthreads();
    }
}

// ---- sel, off and m from the sorted keys ------------------------------------
__device__ __forceinline__ bool rg_is_head(const uint32_t *key, uint64_t k, uint32_t n, uint32_t total)
{
    if (k >= total) return false;
    const uint32_t x = key[k];
    return x < n && (k == 0 || key[k - 1] != x);
}

// cnt[tile] = the tile's run starts; *valid = how many keys are below n
__global__ void __launch_bounds__(kRgBlock)
    rg_head_count(const uint32_t *__restrict__ key, uint32_t n, uint32_t total, uint32_t *__restrict__ cnt,
                  uint32_t *__restrict__ valid)
{
    __shared__ uint32_t wsum[kRgWaves];
    const int tid = threadIdx.x;
    uint32_t c = 0;
    for (int r = 0; r < kRgRounds; ++r) {
        const uint64_t k = (uint64_t)blockIdx.x * kTile + (uint32_t)(r * kRgBlock + tid);
        c += rg_is_head(key, k, n, total) ? 1u : 0u;
        if (k < total) {
            // sorted: the keys below n are a prefix, and exactly one k ends it
            const bool in = key[k] < n;
            if (in && (k + 1 == total || key[k + 1] >= n)) *valid = (uint32_t)k + 1u;
            if (!in && k == 0) *valid = 0u;
        }
    }
    uint32_t all;
    (void)rg_block_scan(c, wsum, &all);
    if (tid == 0) cnt[blockIdx.x] = all;
}

// sel[t] and off[t] for the tile's run starts, t from cnt[tile] (scanned) on
__global__ void __launch_bounds__(kRgBlock)
    rg_head_write(const uint32_t *__restrict__ key, uint32_t n, uint32_t total, const uint32_t *__restrict__ cnt,
                  uint32_t cap, uint32_t *__restrict__ sel, uint32_t *__restrict__ off)
{
    __shared__ uint32_t wsum[kRgWaves];
    const int tid = threadIdx.x;
    uint32_t t0 = cnt[blockIdx.x];
    for (int r = 0; r < kRgRounds; ++r) {
        const uint64_t k = (uint64_t)blockIdx.x * kTile + (uint32_t)(r * kRgBlock + tid);
        const bool head = rg_is_head(key, k, n, total);
        uint32_t all;
        const uint32_t t = t0 + rg_block_scan(head ? 1u : 0u, wsum, &all);
        if (head && t < cap) { // distinct keys below n: at most min(total, n)
            sel[t] = key[k];
            off[t] = (uint32_t)k;
        }
        t0 += all;
    }
}

// the padded tails: sel[t] = ~0 for m <= t < cap, off[t] = valid for m <= t <= cap
__global__ void __launch_bounds__(kRgBlock)
    rg_tail(const uint32_t *__restrict__ m, const uint32_t *__restrict__ valid, uint32_t cap,
            uint32_t *__restrict__ sel, uint32_t *__restrict__ off)
{
    const uint64_t t = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (t > cap || t < *m) return;
    off[t] = *valid;
    if (t < cap) sel[t] = 0xffffffffu;
}

// ---- a queue of one tile: the whole grouping in one block, keys and payload in LDS ----
// The passes, the run starts and the tails of the kernels above in one launch
// for total <= kTile: the same rounds and the same ranking (rg_peers, the
// waves' counts in LDS), the digit counts of the tile scanned by the block
// itself instead of through a table.
__global__ void __launch_bounds__(kRgBlock)
    rg_one_tile(const uint32_t *__restrict__ ids, uint32_t n, uint32_t total, int passes, uint32_t cap,
                uint32_t *__restrict__ perm, uint32_t *__restrict__ sel, uint32_t *__restrict__ off,
                uint32_t *__restrict__ m_out)
{
    __shared__ uint32_t key[2][kTile], pay[2][kTile];
    __shared__ uint32_t base[kDigits];
    __shared__ uint32_t wcnt[kRgWaves][kDigits];
    __shared__ uint32_t wsum[kRgWaves];
    __shared__ uint32_t s_valid;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr = (int)((total + kRgBlock - 1) / kRgBlock); // the rounds that hold an element, the same for all
    for (int r = 0; r < nr; ++r) {
        const uint32_t idx = (uint32_t)(r * kRgBlock + tid);
        if (idx < total) {
            key[0][idx] = rg_key<true>(ids, idx, n);
            pay[0][idx] = idx;
        }
    }
    int cur = 0;
    for (int p = 0; p < passes; ++p) {
        const uint32_t shift = (uint32_t)(p * kDigitBits);
        base[tid] = 0u;
#pragma unroll
        for (int w = 0; w < kRgWaves; ++w) wcnt[w][tid] = 0u;
        __syncthreads(); // also: the loads above, the previous pass's writes
        for (int r = 0; r < nr; ++r) {
            const uint32_t idx = (uint32_t)(r * kRgBlock + tid);
            const bool act = idx < total;
            const uint32_t d = act ? (key[cur][idx] >> shift) & (kDigits - 1u) : 0u;
            const uint64_t peers = rg_peers(d, act);
            if (act && (peers & rg_below(lane)) == 0u) atomicAdd(&base[d], (uint32_t)__popcll(peers));
        }
        __syncthreads();
        uint32_t all;
        const uint32_t start = rg_block_scan(base[tid], wsum, &all);
        base[tid] = start; // thread d alone reads and writes digit d's word
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const uint32_t idx = (uint32_t)(r * kRgBlock + tid);
            const bool act = idx < total;
            const uint32_t k = act ? key[cur][idx] : 0u;
            const uint32_t d = (k >> shift) & (kDigits - 1u);
            const uint64_t peers = rg_peers(d, act);
            const uint32_t rank = (uint32_t)__popcll(peers & rg_below(lane));
            if (act && rank == 0u) wcnt[wave][d] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (act) {
                uint32_t pos = base[d] + rank;
#pragma unroll
                for (int w = 0; w < kRgWaves; ++w) pos += w < wave ? wcnt[w][d] : 0u;
                if (pos < total) {
                    key[cur ^ 1][pos] = k;
                    pay[cur ^ 1][pos] = pay[cur][idx];
                }
            }
            __syncthreads();
            uint32_t add = 0;
#pragma unroll
            for (int w = 0; w < kRgWaves; ++w) {
                add += wcnt[w][tid];
                wcnt[w][tid] = 0u;
            }
            base[tid] += add;
            __syncthreads();
        }
        cur ^= 1;
    }
    __syncthreads(); // no pass at all never happens (n >= 1), but the loads must be seen
    const uint32_t *sk = key[cur];
    uint32_t t0 = 0;
    for (int r = 0; r < nr; ++r) {
        const uint32_t idx = (uint32_t)(r * kRgBlock + tid);
        const bool act = idx < total;
        const uint32_t k = act ? sk[idx] : 0u;
        if (act) {
            perm[idx] = pay[cur][idx];
            if (k < n && (idx + 1 == total || sk[idx + 1] >= n)) s_valid = idx + 1u;
            if (k >= n && idx == 0) s_valid = 0u;
        }
        const bool head = act && k < n && (idx == 0 || sk[idx - 1] != k);
        uint32_t all;
        const uint32_t t = t0 + rg_block_scan(head ? 1u : 0u, wsum, &all);
        if (head && t < cap) {
            sel[t] = k;
            off[t] = idx;
        }
        t0 += all;
    }
    __syncthreads();
    const uint32_t valid = s_valid;
    for (uint32_t t = t0 + (uint32_t)tid; t <= cap; t += kRgBlock) {
        off[t] = valid;
        if (t < cap) sel[t] = 0xffffffffu;
    }
    if (tid == 0) *m_out = t0;
}

// MK_GROUP_ONE_TILE=0 sends one-tile queues through the kernels of the larger
// ones (for the probe's comparison and the tests of that path at small totals).
inline bool rg_one_tile_enabled()
{
    const char *e = std::getenv("MK_GROUP_ONE_TILE");
    return !(e && e[0] == '0' && e[1] == 0);
}

// ---- the launch ---------------------------------------------------------------
inline size_t rg_al(size_t words) { return (words * 4 + 255) & ~(size_t)255; }

struct RgTmp {
    size_t key0, key1, perm, table, sums, cnt, csums, valid, bytes; // byte offsets, and the size
    uint32_t ntiles;
};

inline RgTmp rg_tmp_layout(size_t total)
{
    RgTmp t{};
    t.ntiles = (uint32_t)((total + kTile - 1) / kTile);
    const size_t tw = (size_t)t.ntiles * kDigits;
    size_t at = 0;
    auto take = [&](size_t words) {
        const size_t o = at;
        at += rg_al(words ? words : 1);
        return o;
    };
    t.key0 = take(total);
    t.key1 = take(total);
    t.perm = take(total);
    t.table = take(tw);
    t.sums = take(rg_scan_blocks(tw));
    t.cnt = take(t.ntiles);
    t.csums = take(rg_scan_blocks(t.ntiles));
    t.valid = take(1);
    t.bytes = at;
    return t;
}

// Caller: device current, arguments checked, total in [1, 2^32).
inline int rg_group(uint32_t n, const uint32_t *d_ids, uint32_t total, uint32_t *d_perm, uint32_t *d_sel,
                    uint32_t *d_off, uint32_t *d_m, void *d_tmp, hipStream_t st)
{
    const RgTmp L = rg_tmp_layout(total);
    char *b = (char *)d_tmp;
    uint32_t *key[2] = {(uint32_t *)(b + L.key0), (uint32_t *)(b + L.key1)};
    uint32_t *table = (uint32_t *)(b + L.table), *sums = (uint32_t *)(b + L.sums);
    uint32_t *cnt = (uint32_t *)(b + L.cnt), *csums = (uint32_t *)(b + L.csums), *valid = (uint32_t *)(b + L.valid);
    const uint32_t bits = rg_bitlen(n); // keys go up to n itself
    const int passes = (int)((bits + kDigitBits - 1) / kDigitBits);
    const dim3 grid(L.ntiles), blk(kRgBlock);
    const uint32_t cap = total < n ? total : n; // M
    if (total <= kTile && rg_one_tile_enabled()) {
        hipLaunchKernelGGL(rg_one_tile, dim3(1), blk, 0, st, d_ids, n, total, passes, cap, d_perm, d_sel, d_off, d_m);
        return hipGetLastError() == hipSuccess ? MK_OK : MK_EDEVICE;
    }
    const uint64_t tw = (uint64_t)L.ntiles * kDigits;
    // the payload alternates between d_perm and the scratch so that the last pass lands in d_perm
    uint32_t *pay[2] = {d_perm, (uint32_t *)(b + L.perm)};
    const uint32_t *src_key = d_ids, *src_pay = nullptr;
    for (int p = 0; p < passes; ++p) {
        const uint32_t shift = (uint32_t)(p * kDigitBits);
        uint32_t *dk = key[p & 1], *dp = pay[(passes - 1 - p) & 1];
        if (p == 0)
            hipLaunchKernelGGL(rg_hist<true>, grid, blk, 0, st, src_key, n, total, shift, L.ntiles, table);
        else
            hipLaunchKernelGGL(rg_hist<false>, grid, blk, 0, st, src_key, n, total, shift, L.ntiles, table);
        if (int rc = rg_scan(table, tw, sums, nullptr, st)) return rc;
        if (p == 0)
            hipLaunchKernelGGL(rg_scatter<true>, grid, blk, 0, st, src_key, src_pay, n, total, shift, L.ntiles,
                               (const uint32_t *)table, dk, dp);
        else
            hipLaunchKernelGGL(rg_scatter<false>, grid, blk, 0, st, src_key, src_pay, n, total, shift, L.ntiles,
                               (const uint32_t *)table, dk, dp);
        src_key = dk;
        src_pay = dp;
    }
    hipLaunchKernelGGL(rg_head_count, grid, blk, 0, st, src_key, n, total, cnt, valid);
    if (int rc = rg_scan(cnt, L.ntiles, csums, d_m, st)) return rc;
    hipLaunchKernelGGL(rg_head_write, grid, blk, 0, st, src_key, n, total, (const uint32_t *)cnt, cap, d_sel, d_off);
    const uint32_t tb = (uint32_t)(((uint64_t)cap + 1 + kRgBlock - 1) / kRgBlock);
    hipLaunchKernelGGL(rg_tail, dim3(tb), blk, 0, st, (const uint32_t *)d_m, (const uint32_t *)valid, cap, d_sel,
                       d_off);
    return hipGetLastError() == hipSuccess ? MK_OK : MK_EDEVICE;
}

// ---- a queue through a session set: the inputs into sorted order, the results back ----
__global__ void __launch_bounds__(kRgBlock)
    rq_gather(const int64_t *__restrict__ in, const uint32_t *__restrict__ perm, uint32_t total,
              int64_t *__restrict__ in_sorted)
{
    const uint64_t k = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (k < total) in_sorted[k] = in[perm[k]];
}

// Sorted position k answers request perm[k]; the positions from *valid on are
// the requests that name no session (key n): 0 / 0 / 0.  busy (when given) is
// set when the first request of a session reports MK_ST_CALL_OPEN.
__global__ void __launch_bounds__(kRgBlock)
    rq_scatter(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ ids, uint32_t total,
               const uint32_t *__restrict__ valid, const int32_t *__restrict__ out_s,
               const uint8_t *__restrict__ st_s, const uint32_t *__restrict__ steps_s, int32_t *__restrict__ out,
               uint8_t *__restrict__ status, uint32_t *__restrict__ steps, uint32_t *busy)
{
    const uint64_t k = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (k >= total) return;
    const uint32_t j = perm[k];
    const bool ok = k < *valid;
    const uint8_t s = ok ? st_s[k] : (uint8_t)0;
    out[j] = ok ? out_s[k] : 0;
    status[j] = s;
    if (steps) steps[j] = ok ? steps_s[k] : 0u;
    if (busy && ok && s == (uint8_t)MK_ST_CALL_OPEN && (k == 0 || ids[perm[k - 1]] != ids[j])) *busy = 1u;
}

} // namespace rg
} // namespace mk
