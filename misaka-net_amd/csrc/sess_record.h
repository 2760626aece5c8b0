// sess_record.h -- the session record: one session's whole state as a fixed
// number of 32-bit rows, the form mk_session_snapshot / mk_session_restore
// move between a set and the host, another set or another tier.  A block of
// m records is laid out [row][m] (row r of entry t at rec[r * m + t]); an
// int64 takes two rows, low word first.
//
//   control   held io csteps pin in_val out_val bits pfull(2)
//   per node  acc(2) bak(2) ip pendv port[4]          sorted-name order
//   per stack depth, then stack_cap entries           0 at and above the depth
//   native    sb, regs (2 rows each), slots           native-tier sets only
//
// The first three sections are the canonical part, in the bytecode
// interpreter's terms (mk_exec.hip SessParams): always filled, readable by
// either tier, any set of the same network and the oracle.  For a session the
// native tier holds they come from sess_convert.h over the state map of the
// superblock its next call starts at, with the call closed.  One restatement
// of the row arithmetic, the canonical writer and the range checks for the
// export / restore kernels (mk_exec.hip) and the host model (sched_check.cpp).
// Included after mk.h, tis_sched.h and sess_convert.h.
#pragma once

#ifndef MK_HD
#define MK_HD
#endif

namespace mk {

constexpr uint32_t kSessRecMagic = 0x52534B4Du; // "MKSR"
constexpr uint32_t kSessRecVersion = 1u;
constexpr uint32_t kSessRecDead = 0xFFFFFFF0u;  // MK_SS_DEAD: the native sb of an ended session

// rows of the control section, and of one node's group
enum : uint32_t { SR_HELD = 0, SR_IO, SR_CSTEPS, SR_PIN, SR_IN_VAL, SR_OUT_VAL, SR_BITS, SR_PFULL, SR_CTRL = 9 };
enum : uint32_t { SR_ACC = 0, SR_BAK = 2, SR_IP = 4, SR_PENDV = 5, SR_PORT = 6, SR_NODE = 10 };

struct SessRecShape {
    int N, S;               // program nodes, stacks
    uint32_t cap;           // stack_cap
    uint32_t nregs, nslots; // the native section's registers and slots (used only where it is present)
    MK_HD uint32_t node(int k) const { return SR_CTRL + SR_NODE * (uint32_t)k; }
    MK_HD uint32_t stack(int s) const { return SR_CTRL + SR_NODE * (uint32_t)N + (uint32_t)s * (1u + cap); }
    MK_HD uint32_t canon_rows() const { return stack(S); }
    MK_HD uint32_t native_rows() const { return 1u + 2u * nregs + nslots; }
    MK_HD uint32_t sb_row() const { return canon_rows(); }
    MK_HD uint32_t reg_row(uint32_t r) const { return canon_rows() + 1u + 2u * r; }
    MK_HD uint32_t slot_row(uint32_t q) const { return canon_rows() + 1u + 2u * nregs + q; }
};

// sess_convert's Out over a record: put(row, word).  The call is written as
// closed, so call() records nothing; entries at and above a stack's depth are 0.
template <class Put>
struct SessRecOut {
    const SessRecShape &L;
    Put &put;
    uint32_t io = 0;
    MK_HD void w64(uint32_t row, uint64_t v)
    {
        put(row, (uint32_t)v);
        put(row + 1u, (uint32_t)(v >> 32));
    }
    MK_HD void acc(int n, int64_t v) { w64(L.node(n) + SR_ACC, (uint64_t)v); }
    MK_HD void bak(int n, int64_t v) { w64(L.node(n) + SR_BAK, (uint64_t)v); }
    MK_HD void ip(int n, int32_t v) { put(L.node(n) + SR_IP, (uint32_t)v); }
    MK_HD void pendv(int n, int32_t v) { put(L.node(n) + SR_PENDV, (uint32_t)v); }
    MK_HD void port(int q, int32_t v) { put(L.node(q >> 2) + SR_PORT + ((uint32_t)q & 3u), (uint32_t)v); }
    MK_HD void pfull(uint64_t x) { w64(SR_PFULL, x); }
    MK_HD void bits(uint32_t pend, uint32_t hung) { put(SR_BITS, (pend & 0xffffu) | (hung << 16)); }
    MK_HD void chans(bool in_full, bool out_full, int32_t iv, int32_t ov)
    {
        io |= (in_full ? 1u : 0u) | (out_full ? 2u : 0u);
        put(SR_IN_VAL, (uint32_t)iv);
        put(SR_OUT_VAL, (uint32_t)ov);
    }
    MK_HD void depth(int s, uint32_t d)
    {
        put(L.stack(s), d);
        for (uint32_t j = d; j < L.cap; j++) put(L.stack(s) + 1u + j, 0u);
    }
    MK_HD void entry(int s, uint32_t d, int32_t v)
    {
        if (d < L.cap) put(L.stack(s) + 1u + d, (uint32_t)v);
    }
    MK_HD void call(bool, int32_t, int, bool) {}
};

// The canonical part of a session the native tier holds: sb is the variant
// its next call starts at (the map of superblock sb / 2) or kSessRecDead.
// The call is closed: io bits 2, 3 and 8-14 clear, pin = csteps = 0.  An
// ended session has io's dead field set and everything else zero.
template <class Reg, class Slot, class Put>
MK_HD inline void sess_record_native(const SessRecShape &L, uint32_t sb, const SessMapHdr *hdr, const SessSrcDev *map,
                                     const int64_t *dyn_base, const Reg &reg, const Slot &slot, Put &put)
{
    put(SR_HELD, 1u);
    put(SR_CSTEPS, 0u);
    put(SR_PIN, 0u);
    if (sb == kSessRecDead) {
        put(SR_IO, (uint32_t)MK_ST_STACK_OVERFLOW << 4);
        for (uint32_t r = SR_IN_VAL; r < L.canon_rows(); r++) put(r, 0u);
        return;
    }
    const SessMapHdr h = hdr[sb / 2u];
    SessRecOut<Put> o{L, put};
    sess_convert(L.N, L.S, h, map + h.off, dyn_base, reg, slot, o);
    put(SR_IO, o.io);
}

// The range checks of a restore, on the canonical part: get(row) reads the
// record.  len: the nodes' program lengths.
template <class Get>
MK_HD inline bool sess_record_ok(const SessRecShape &L, const uint32_t *len, const Get &get)
{
    if (get(SR_HELD) > 1u) return false;
    for (int k = 0; k < L.N; k++) {
        const uint32_t ip = get(L.node(k) + SR_IP);
        if (ip >= len[k] && !(ip == 0u && len[k] == 0u)) return false;
    }
    for (int s = 0; s < L.S; s++)
        if (get(L.stack(s)) > L.cap) return false;
    return true;
}

// ... and on the native section, for a record that is restored natively: sb
// is kSessRecDead or the fast variant of a superblock a call starts at (the
// `pre` maps, bit k of pre[] for superblock k of nsb), and the depth of every
// dynamic stack, which indexes the slots, is within the capacity.
template <class Get>
MK_HD inline bool sess_record_native_ok(const SessRecShape &L, uint32_t nsb, const uint32_t *pre,
                                        const SessMapHdr *hdr, const SessSrcDev *map, const int64_t *dyn_base,
                                        const Get &get)
{
    const uint32_t sb = get(L.sb_row());
    if (sb == kSessRecDead) return true;
    if ((sb & 1u) || sb / 2u >= nsb) return false;
    const uint32_t k = sb / 2u;
    if (!((pre[k >> 5] >> (k & 31u)) & 1u)) return false;
    const SessSrcDev *loc = map + hdr[k].off + L.N;
    auto reg = [&](uint32_t r) -> int64_t {
        if (r >= L.nregs) return -1;
        return (int64_t)((uint64_t)get(L.reg_row(r)) | (uint64_t)get(L.reg_row(r) + 1u) << 32);
    };
    auto slot = [&](uint32_t q) -> int32_t { return q < L.nslots ? (int32_t)get(L.slot_row(q)) : -1; };
    for (int s = 0; s < L.S; s++)
        if (dyn_base[s] >= 0 && (uint64_t)sess_value(loc[7 * L.N + 2 + s], reg, slot) > (uint64_t)L.cap) return false;
    return true;
}

} // namespace mk
