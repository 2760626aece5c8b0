// sess_drain.h -- the open calls of a session set as a list on the GPU, and
// the drain that resumes them slice after slice over that list
// (mk_session_open_list, mk_session_drain, include/mk.h).
//
// Both are one stable compaction of `len` entries:
//   flag      words[k] = entry k is kept (and what the pass writes per entry)
//   scan      words, exclusively and in place (req_group.h rg_scan)
//   scatter   a kept entry's session and caller column to list / pos[words[k]]
//   tail      list = 0xffffffff and pos = 0 from the count on, the count's copy
// over one of two sources:
//   DrOpen    entry t is session sel[t] (t itself for a null list), kept when
//             its call is open (io bit 3); for a drain it also writes the
//             answer of an entry without an open call into the caller's column t
//   DrFold    entry k is slot k of the list a resume slice just ran over into
//             compact columns: its out / status / steps go to the caller's
//             column pos[k], and it is kept when its status is MK_ST_BUDGET
// Stable, so a list is strictly increasing like the one it was taken from: a
// valid sel of the indexed forms, its padding dropped by their `>= n` guard.
// A list of one tile takes one block and one launch for all of it
// (dr_one_tile), so a drain over a small set costs one small launch a repack.
//
// Every kernel writes with ordinary vector stores; a value one thread writes
// for the block is written under `if (threadIdx.x == ...)`.  Included by
// mk_exec.hip after req_group.h and the session constants; everything here is
// static to it.
#pragma once

namespace mk {
namespace dr {

using rg::kRgBlock;
using rg::kRgWaves;
using rg::kTile;

constexpr uint32_t kDrPad = 0xffffffffu; // names no session: n < 2^32

struct DrOpen {
    const uint32_t *io;  // [n] the interpreter's io words
    const uint32_t *nsb; // [n] the native tier's, or null
    uint32_t n;
    const uint32_t *sel; // [len] or null
    // a drain's entry: the caller's columns, or out null for the list alone
    int32_t *out;
    uint8_t *status;
    uint32_t *steps; // nullable

    // What a resume reports for a session with no call open (tis_session_one):
    // 0, or what ended it -- a session the native tier holds has ended when its
    // nsb says so, one the interpreter holds when io bits 4-7 are set.
    __device__ __forceinline__ uint8_t idle_status(uint32_t i, uint32_t w) const
    {
        if (nsb) {
            const uint32_t b = nsb[i];
            if (b == kSessDead) return (uint8_t)MK_ST_STACK_OVERFLOW;
            if (b != kSessT1) return (uint8_t)0;
        }
        return (uint8_t)((w >> 4) & 15u);
    }

    // Entry k < len: its session and caller column; true when it is kept.
    // `emit`: this is the pass that writes the entry's answer.
    __device__ __forceinline__ bool entry(uint32_t k, bool emit, uint32_t *id, uint32_t *col) const
    {
        const uint32_t i = sel ? sel[k] : k;
        const bool real = i < n;
        const uint32_t w = real ? io[i] : 0u;
        *id = i;
        *col = k;
        if (emit && out) {
            out[k] = 0;
            status[k] = real ? idle_status(i, w) : (uint8_t)0;
            if (steps) steps[k] = 0u;
        }
        return real && ((w >> 3) & 1u);
    }
};

struct DrFold {
    const uint32_t *list, *pos; // [len] the list the slice ran over, padded with kDrPad
    uint32_t n;
    const int32_t *c_out; // [len] the slice's compact columns
    const uint8_t *c_status;
    const uint32_t *c_steps; // null with steps null
    int32_t *out;            // the caller's columns
    uint8_t *status;
    uint32_t *steps; // nullable

    __device__ __forceinline__ bool entry(uint32_t k, bool emit, uint32_t *id, uint32_t *col) const
    {
        const uint32_t i = list[k];
        const bool real = i < n;
        const uint32_t t = real ? pos[k] : 0u;
        const uint8_t st = real ? c_status[k] : (uint8_t)0;
        *id = i;
        *col = t;
        if (emit && real) {
            out[t] = c_out[k];
            status[t] = st;
            if (steps) steps[t] = c_steps[k];
        }
        return real && st == (uint8_t)MK_ST_BUDGET;
    }
};

template <class Src>
__global__ void __launch_bounds__(kRgBlock) dr_flag(Src s, uint32_t len, uint32_t *__restrict__ words)
{
    const uint64_t k = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (k >= len) return;
    uint32_t id, col;
    words[k] = s.entry((uint32_t)k, true, &id, &col) ? 1u : 0u;
}

// words: scanned, so words[k] is the rank of a kept entry k
template <class Src>
__global__ void __launch_bounds__(kRgBlock)
    dr_scatter(Src s, uint32_t len, const uint32_t *__restrict__ words, uint32_t *__restrict__ list,
               uint32_t *__restrict__ pos)
{
    const uint64_t k = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    if (k >= len) return;
    uint32_t id, col;
    if (!s.entry((uint32_t)k, false, &id, &col)) return;
    const uint32_t r = words[k];
    if (r >= len) return; // holds for words that counted these entries
    list[r] = id;
    if (pos) pos[r] = col;
}

// the padded tails, and the count's copy for the caller (count2, nullable)
__global__ void __launch_bounds__(kRgBlock)
    dr_tail(const uint32_t *__restrict__ count, uint32_t len, uint32_t *__restrict__ list, uint32_t *__restrict__ pos,
            uint32_t *__restrict__ count2)
{
    const uint64_t t = (uint64_t)blockIdx.x * kRgBlock + threadIdx.x;
    const uint32_t c = *count;
    if (count2 && blockIdx.x == 0 && threadIdx.x == 0) *count2 = c;
    if (t >= len || t < c) return;
    list[t] = kDrPad;
    if (pos) pos[t] = 0u;
}

// len <= kTile: flag, scan, scatter and tail in one block, round after round
// of the block's width with a running base, as rg_one_tile ranks its run starts
template <class Src>
__global__ void __launch_bounds__(kRgBlock)
    dr_one_tile(Src s, uint32_t len, uint32_t *__restrict__ list, uint32_t *__restrict__ pos,
                uint32_t *__restrict__ count, uint32_t *__restrict__ count2)
{
    __shared__ uint32_t wsum[kRgWaves];
    const int tid = threadIdx.x;
    const int nr = (int)((len + kRgBlock - 1) / kRgBlock); // the rounds that hold an entry, the same for all
    uint32_t t0 = 0;
    for (int r = 0; r < nr; ++r) {
        const uint32_t k = (uint32_t)(r * kRgBlock + tid);
        uint32_t id = 0, col = 0;
        const bool keep = k < len && s.entry(k, true, &id, &col);
        uint32_t all;
        const uint32_t t = t0 + rg::rg_block_scan(keep ? 1u : 0u, wsum, &all);
        if (keep && t < len) {
            list[t] = id;
            if (pos) pos[t] = col;
        }
        t0 += all;
    }
    for (uint32_t t = t0 + (uint32_t)tid; t < len; t += kRgBlock) {
        list[t] = kDrPad;
        if (pos) pos[t] = 0u;
    }
    if (tid == 0) {
        *count = t0;
        if (count2) *count2 = t0;
    }
}

// The compaction of s's `len` entries (1 <= len < 2^32) on `st`: list and pos
// (nullable) take len words each, *count and *count2 (nullable) the number
// kept.  words: len words of scratch, sums: rg_scan_blocks(len).  list and
// pos must not overlap what the source reads.
template <class Src>
inline int dr_compact(const Src &s, uint32_t len, uint32_t *list, uint32_t *pos, uint32_t *count, uint32_t *count2,
                      uint32_t *words, uint32_t *sums, hipStream_t st)
{
    const dim3 blk(kRgBlock);
    if (len <= kTile) {
        hipLaunchKernelGGL(dr_one_tile<Src>, dim3(1), blk, 0, st, s, len, list, pos, count, count2);
        return hipGetLastError() == hipSuccess ? MK_OK : MK_EDEVICE;
    }
    const dim3 grid((uint32_t)(((uint64_t)len + kRgBlock - 1) / kRgBlock));
    hipLaunchKernelGGL(dr_flag<Src>, grid, blk, 0, st, s, len, words);
    if (int rc = rg::rg_scan(words, len, sums, count, st)) return rc;
    hipLaunchKernelGGL(dr_scatter<Src>, grid, blk, 0, st, s, len, (const uint32_t *)words, list, pos);
    hipLaunchKernelGGL(dr_tail, grid, blk, 0, st, (const uint32_t *)count, len, list, pos, count2);
    return hipGetLastError() == hipSuccess ? MK_OK : MK_EDEVICE;
}

} // namespace dr
} // namespace mk
