// sess_promote.h -- the way back from the bytecode interpreter to the native
// tier: sess_convert.h read in the other direction.  An instance the
// interpreter holds between calls (its call closed) is an instance of the
// entry state of some superblock a call starts at; this finds that superblock
// and says what its registers and stack slots hold.  One restatement for the
// GPU kernels (mk_exec.hip tis_session_promote_*) and the host model's CPU
// tests (sched_check.cpp mkc_sess_promote).  Included after tis_sched.h.
//
// A superblock k is a candidate when its map has `pre` set, `deposited` and
// `changed` clear and pos 0 (what every U_YIELD target and variant 0 have).
// The instance matches it when the control agrees exactly -- every ip, pend,
// hung, pfull, the two channel bits, every ordinary stack's depth -- and every
// fact the compiler built into the superblock's code holds: a location of kind
// constant has that value (ACC / BAK as int64, the 32-bit locations as int32;
// a port only while full, INL / OUTL with their channel bit, PENDV with the
// node's pend bit), a constant stack entry has that value, a dynamic stack's
// depth is its constant DEP or any depth within the capacity for a register
// DEP, and is at least lo[s] (Ctl::lo, exported as SessEntry::lo: a POP that
// the code makes without a check).  Dead locations are ignored: nothing reads
// them before they are written.  CIN is the next call's input.  That is the
// whole of the compiler's state key (tis_sched.cpp key_of), so the code of k
// run from the filled registers does what the interpreter would have done.
//
//   In:  ip(n) acc(n) bak(n) pendv(n) port(q) pfull() bits() in_full()
//        out_full() in_val() out_val() depth(s) entry(s, j)
//   Out: reg(r, int64) slot(q, int32) dyn(s, base, d)   "stack s's d entries
//        go to slots base + j"; whatever is not named is to be 0
#pragma once

#include <algorithm>
#include <utility>
#include <vector>

#ifndef MK_HD
#define MK_HD
#endif

namespace mk {

// candidates: pre, not deposited, not changed, pos 0 (SessMapHdr::flags)
MK_HD inline bool sess_promote_candidate(const SessMapHdr &h) { return (h.flags & 0xff1cu) == 16u; }

MK_HD inline uint64_t sess_promote_mix(uint64_t h, uint64_t v)
{
    uint64_t x = (h ^ v) + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The control hash: ip[], pend | hung << 16 (the interpreter's `bits` word),
// pfull, the channel bits and the ordinary stacks' depths.
template <class Ip, class Depth>
MK_HD inline uint64_t sess_promote_hash(int N, int S, const int64_t *dyn_base, const Ip &ip, uint32_t bits,
                                        uint64_t pfull, bool in_full, bool out_full, const Depth &depth)
{
    uint64_t h = 0x4D4B50524F4D4F54ull; // "MKPROMOT"
    for (int n = 0; n < N; n++) h = sess_promote_mix(h, (uint32_t)ip(n));
    h = sess_promote_mix(h, bits);
    h = sess_promote_mix(h, pfull);
    h = sess_promote_mix(h, (in_full ? 1u : 0u) | (out_full ? 2u : 0u));
    for (int s = 0; s < S; s++)
        if (dyn_base[s] < 0) h = sess_promote_mix(h, (uint32_t)depth(s));
    return h;
}

MK_HD inline uint32_t sess_promote_bits(const SessMapHdr &h) { return (h.pend & 0xffffu) | (h.hung << 16); }

// ... of a superblock's map
MK_HD inline uint64_t sess_promote_hash_map(int N, int S, const SessMapHdr &h, const SessSrcDev *rec,
                                            const int64_t *dyn_base)
{
    auto ip = [&](int n) { return (int32_t)rec[n].c; };
    auto depth = [&](int s) {
        const SessSrcDev *sr = rec + N + 7 * N + 2 + S + 1;
        for (int t = 0; t < s; t++) sr += 1 + (uint32_t)sr->c;
        return (uint32_t)sr->c;
    };
    return sess_promote_hash(N, S, dyn_base, ip, sess_promote_bits(h), h.pfull, h.flags & 1u, h.flags & 2u, depth);
}

// ... of an instance in the interpreter's terms
template <class In>
MK_HD inline uint64_t sess_promote_hash_in(int N, int S, const int64_t *dyn_base, const In &in)
{
    auto ip = [&](int n) { return in.ip(n); };
    auto depth = [&](int s) { return in.depth(s); };
    return sess_promote_hash(N, S, dyn_base, ip, in.bits(), in.pfull(), in.in_full(), in.out_full(), depth);
}

// Is the instance an instance of superblock k's entry state?  h, rec: k's
// header and records (rec = map + h.off); lo: k's S lower bounds.
template <class In>
MK_HD inline bool sess_promote_match(int N, int S, uint32_t cap, const SessMapHdr &h, const SessSrcDev *rec,
                                     const uint8_t *lo, const int64_t *dyn_base, const In &in)
{
    if (!sess_promote_candidate(h)) return false;
    const bool in_full = in.in_full(), out_full = in.out_full();
    const uint64_t pfull = in.pfull();
    const uint32_t bits = in.bits();
    if (bits != sess_promote_bits(h) || pfull != h.pfull || in_full != ((h.flags & 1u) != 0) ||
        out_full != ((h.flags & 2u) != 0))
        return false;
    for (int n = 0; n < N; n++)
        if ((int64_t)in.ip(n) != rec[n].c) return false;
    const SessSrcDev *loc = rec + N;
    // a location against the instance's value: a constant must be it, a register takes any, a dead one is ignored
    auto ok64 = [](const SessSrcDev &x, int64_t v) { return x.kind == 1u ? x.c == v : x.kind == 0u || x.kind == 2u; };
    auto ok32 = [](const SessSrcDev &x, int32_t v) {
        return x.kind == 1u ? (int32_t)(uint32_t)(uint64_t)x.c == v : x.kind == 0u || x.kind == 2u;
    };
    for (int n = 0; n < N; n++) {
        if (!ok64(loc[n], in.acc(n)) || !ok64(loc[N + n], in.bak(n))) return false;
        if (((bits >> n) & 1u) && !ok32(loc[6 * N + n], in.pendv(n))) return false;
    }
    for (int q = 0; q < 4 * N; q++)
        if (((pfull >> q) & 1ull) && !ok32(loc[2 * N + q], in.port(q))) return false;
    if (in_full && !ok32(loc[7 * N], in.in_val())) return false;
    if (out_full && !ok32(loc[7 * N + 1], in.out_val())) return false;
    const SessSrcDev *sr = loc + 7 * N + 2 + S + 1; // after CIN
    for (int s = 0; s < S; s++) {
        const uint32_t k = (uint32_t)sr->c, d = (uint32_t)in.depth(s);
        ++sr;
        if (d > cap) return false; // no stack is deeper: nothing below reads an entry past the capacity
        if (dyn_base[s] >= 0) {
            const SessSrcDev &D = loc[7 * N + 2 + s];
            if (d < lo[s]) return false;
            if (D.kind == 1u ? (uint64_t)D.c != d : D.kind != 2u) return false;
        } else {
            if (d != k) return false;
            for (uint32_t j = 0; j < k; j++) {
                if (sr[j].kind == 1u ? (int32_t)(uint32_t)(uint64_t)sr[j].c != in.entry(s, j) : sr[j].kind != 3u)
                    return false;
            }
        }
        sr += k;
    }
    return true;
}

// The call-start superblocks by control hash: (hash, superblock) sorted by
// hash, then superblock, so that the first full match of an equal-hash run is
// the lowest-numbered superblock that matches at all (all matches of one
// instance share its control, hence its hash).
inline void sess_promote_table(int N, int S, const std::vector<SessMapHdr> &hdr, const std::vector<SessSrcDev> &map,
                               const int64_t *dyn_base, std::vector<uint64_t> &hash, std::vector<uint32_t> &sb)
{
    std::vector<std::pair<uint64_t, uint32_t>> t;
    for (size_t k = 0; k < hdr.size(); k++)
        if (sess_promote_candidate(hdr[k]))
            t.emplace_back(sess_promote_hash_map(N, S, hdr[k], map.data() + hdr[k].off, dyn_base), (uint32_t)k);
    std::sort(t.begin(), t.end());
    hash.clear();
    sb.clear();
    for (const auto &e : t) {
        hash.push_back(e.first);
        sb.push_back(e.second);
    }
}

struct SessPromoTab {
    const uint64_t *hash; // [count] ascending
    const uint32_t *sb;   // [count]
    uint32_t count;
    const uint8_t *lo;    // [superblock][S]
};

// The superblock the instance promotes to, or -1: a binary search for its
// control hash, then the run of equal hashes in order.
template <class In>
MK_HD inline int64_t sess_promote_find(int N, int S, uint32_t cap, const SessPromoTab &t, const SessMapHdr *hdr,
                                       const SessSrcDev *map, const int64_t *dyn_base, const In &in)
{
    const uint64_t want = sess_promote_hash_in(N, S, dyn_base, in);
    uint32_t a = 0, b = t.count;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2u;
        if (t.hash[mid] < want) a = mid + 1u;
        else b = mid;
    }
    for (; a < t.count && t.hash[a] == want; a++) {
        const uint32_t k = t.sb[a];
        if (sess_promote_match(N, S, cap, hdr[k], map + hdr[k].off, t.lo + (size_t)k * (size_t)S, dyn_base, in))
            return (int64_t)k;
    }
    return -1;
}

// What superblock k's registers and slots hold for the instance.  A 32-bit
// location's home gets the sign-extended int32: the generated code reads such
// a home without truncating (tis_sched.cpp load_entry, r32_).
template <class In, class Out>
MK_HD inline void sess_promote_fill(int N, int S, const SessMapHdr &h, const SessSrcDev *rec, const int64_t *dyn_base,
                                    const In &in, Out &o)
{
    (void)h;
    const SessSrcDev *loc = rec + N;
    auto put = [&](const SessSrcDev &x, int64_t v) {
        if (x.kind == 2u) o.reg(x.r, v);
    };
    for (int n = 0; n < N; n++) {
        put(loc[n], in.acc(n));
        put(loc[N + n], in.bak(n));
        put(loc[6 * N + n], (int64_t)in.pendv(n));
    }
    for (int q = 0; q < 4 * N; q++) put(loc[2 * N + q], (int64_t)in.port(q));
    put(loc[7 * N], (int64_t)in.in_val());
    put(loc[7 * N + 1], (int64_t)in.out_val());
    const SessSrcDev *sr = loc + 7 * N + 2 + S + 1;
    for (int s = 0; s < S; s++) {
        const uint32_t k = (uint32_t)sr->c;
        ++sr;
        if (dyn_base[s] >= 0) {
            const uint32_t d = (uint32_t)in.depth(s);
            put(loc[7 * N + 2 + s], (int64_t)d);
            o.dyn(s, (uint32_t)dyn_base[s], d);
        } else {
            for (uint32_t j = 0; j < k; j++)
                if (sr[j].kind == 3u) o.slot(sr[j].r, in.entry(s, j));
        }
        sr += k;
    }
}

} // namespace mk
