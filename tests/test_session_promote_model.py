"""Promotion of interpreter-held sessions back to the native tier, without a
GPU: the ABI is there, and the inverse map (csrc/sess_promote.h) is checked on
the schedule compiler's host model (sched_check.cpp mkc_sess_promote) against
the CPU oracle.

A canonical state -- a live instance between calls, in the interpreter's terms
-- is promoted into a slot of a host model whose registers hold garbage; the
slot must then answer further calls exactly as the instance it came from.
Every state that calls alone produce must promote (the session schedule does
not depend on the budget, so such a state is an instance of a call-start
superblock's entry state): no session is left out of that condition."""
import ctypes as C

import numpy as np
import pytest

import misaka_net_amd as mk
import schedcheck as sc
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from schedcheck import HANDOFF
from snapcheck import SnapSessions
from test_session_snapshot_model import MODEL_NETS, NS, _nstack, _prefix

PROMOTE = ["mk_session_promote", "mk_session_promote_device"]
BIG = 1 << 20  # a budget no call of these networks' prefixes reaches


def _bind():
    h = sc.lib()
    h.mkc_sess_promote.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(sc.OrcFlat), C.c_void_p]
    h.mkc_sess_loc_kind.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    return h


def promote(host, dst, flat, ent):
    """The superblock slot ``dst`` of ``host`` now starts its next call at, or -1."""
    return _bind().mkc_sess_promote(host._h, dst, C.byref(flat), ent.ctypes.data)


# ---- 1: the ABI is there and refuses a null session --------------------------
def test_promote_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in PROMOTE:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    buf = np.zeros(8, np.uint32)
    bp = buf.ctypes.data_as(C.c_void_p)
    cnt = C.c_size_t()
    assert lib.mk_session_promote(None, bp, 1, bp, C.byref(cnt)) == N.MK_EINVAL
    assert lib.mk_session_promote_device(None, bp, 1, bp, None) == N.MK_EINVAL
    for name in ("promote", "promote_device"):
        assert callable(getattr(mk.SessionSet, name))


def _same_or_handoff(got, want, i, live, ctx):
    """Host-model results of slot i against the oracle's (out, status, steps)
    of one call; a hand-off is the oracle's MK_ST_BUDGET and ends the comparison
    of that slot (live[i] cleared): the host model does not finish such a call."""
    o, s, p = (int(a) for a in got)
    if s == HANDOFF:
        assert (int(want[1]) & N.MK_ST_REASON_MASK) == N.MK_ST_BUDGET, ctx
        live[i] = False
        return False
    assert (o, s, p) == tuple(int(a) for a in want), ctx
    return True


# ---- 2: round trip; every idle state matches ---------------------------------
@pytest.mark.parametrize("name", list(MODEL_NETS))
def test_idle_state_promotes_and_continues_identically(name):
    nodes, cap, budget, gen, _ = MODEL_NETS[name]()
    a, _, idle, _, _ = _prefix(nodes, cap, budget, gen)
    b = SnapSessions(nodes, NS, stack_cap=cap)  # its registers are garbage, its slots absent
    which = np.nonzero(idle)[0]
    assert which.size >= 50
    missed = []
    for i in which:
        flat, ent = a.export_idle(int(i), _nstack(nodes))
        if promote(b, int(i), flat, ent) < 0:
            missed.append(int(i))
    print(f"{name}: {which.size} idle states, {which.size - len(missed)} promoted")
    assert not missed, f"{name}: states that calls produced match no call-start superblock: {missed[:10]}"
    for seed in (1003, 1004, 1005):
        x = po.gen_inputs(seed, NS, **gen)
        ra, rb = a.call(x, budget=budget), b.call(x, budget=budget)
        for k in range(3):
            assert np.array_equal(ra[k][which], rb[k][which]), (name, seed, k)


# ---- 3: hand-off states reach the native tier again --------------------------
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_handed_off_sessions_promote_from_the_finished_state(name):
    nodes, cap, budget, gen, mix = MODEL_NETS[name]()
    a, _, _, handed, _ = _prefix(nodes, cap, budget, gen)
    c, ref, c_idle, c_handed, _ = _prefix(nodes, cap, BIG, gen)  # the same calls, none handed off
    assert handed.sum() == mix[1] and not c_handed.any()
    took = handed & c_idle  # the rest of A's handed-off sessions ended in a stack overflow when finished
    print(f"{name}: handed off {handed.sum()}, of them live once finished {took.sum()}")
    assert took.sum() >= 50
    for i in np.nonzero(took)[0]:
        flat, ent = c.export_idle(int(i), _nstack(nodes))
        assert promote(a, int(i), flat, ent) >= 0, (name, int(i))
    live = ~handed | took  # A's sessions that are where the oracle's are
    finished = 0            # calls of promoted sessions that ran to their end and were compared
    for seed in (1003, 1004, 1005):
        x = po.gen_inputs(seed, NS, **gen)
        got, want = a.call(x, budget=budget), ref.compute(x, budget=budget)
        for i in np.nonzero(live)[0]:
            done = _same_or_handoff([r[i] for r in got], [r[i] for r in want], i, live, (name, seed, int(i)))
            finished += bool(done and took[i])
    assert finished >= 50


# ---- 4: soundness under foreign states ---------------------------------------
KINDS = ("acc", "bak", "port", "ip", "depth", "in_full")


def _perturb(kind, flat, ent, rng, nprog, nstack, cap, ips, regkind):
    """Changes one fact of the flat state in place; returns "free" when the
    changed location is a register or dead in the state's own superblock (it
    takes any value: such a change must be accepted), "other" otherwise, None
    when the state offers nothing of this kind to change.  Registers first."""
    if kind in ("acc", "bak"):
        base = 0 if kind == "acc" else nprog
        n = min(range(nprog), key=lambda n: (2, 0, 1).index(regkind(base + n)))
        v = int(rng.integers(-2**62, 2**62))
        (flat.acc if kind == "acc" else flat.bak)[n] = v
        return "free" if regkind(base + n) != 1 else "other"
    if kind == "port":
        full = [q for q in range(4 * nprog) if (flat.pfull >> q) & 1]
        if not full:
            return None
        q = min(full, key=lambda q: (2, 0, 1).index(regkind(2 * nprog + q)))
        flat.port[q] = int(rng.integers(-2**31, 2**31))
        return "free" if regkind(2 * nprog + q) != 1 else "other"
    if kind == "ip":
        for n in rng.permutation(nprog):
            other = sorted(ips[int(n)] - {flat.ip[int(n)]})
            if other:
                flat.ip[int(n)] = other[int(rng.integers(len(other)))]
                return "other"
        return None
    if kind == "depth":
        if not nstack:
            return None
        s = int(rng.integers(nstack))
        d = flat.depth[s]
        flat.depth[s] = d + 1 if d < cap and (d == 0 or rng.integers(2)) else d - 1
        return "other"
    flat.in_full = 0 if flat.in_full else 1
    flat.in_val = int(rng.integers(-2**31, 2**31)) if flat.in_full else 0
    return "other"


@pytest.mark.parametrize("name", list(MODEL_NETS))
def test_foreign_states_promote_soundly_or_not_at_all(name):
    nodes, cap, budget, gen, _ = MODEL_NETS[name]()
    capv = 1024 if cap is None else cap
    nstack, nprog = _nstack(nodes), sum(1 for n in nodes if (n.kind if hasattr(n, "name") else n[1]) == "program")
    src, _, idle, _, _ = _prefix(nodes, cap, BIG if name != "random6" else budget, gen)
    which = np.nonzero(idle)[0][:200]
    assert which.size == 200
    exports = [src.export_idle(int(i), nstack) for i in which]
    ips = [set(f.ip[n] for f, _ in exports) for n in range(nprog)]  # instruction pointers seen: valid ones
    d = SnapSessions(nodes, 200, stack_cap=cap)      # the slots promoted into
    fresh = SnapSessions(nodes, 200, stack_cap=cap)  # never touched: what a refused slot must still be
    probe = SnapSessions(nodes, 1, stack_cap=cap)    # takes each state unchanged: its own superblock
    rng = np.random.default_rng(4)
    net = po.OracleNet(nodes)
    oracles, accepted, refused, reg_total, keep = {}, 0, 0, 0, []
    h = _bind()
    for j, (flat, ent) in enumerate(exports):
        k0 = promote(probe, 0, flat, ent)
        assert k0 >= 0
        what = None
        for kind in KINDS[j % len(KINDS):] + KINDS[:j % len(KINDS)]:
            what = _perturb(kind, flat, ent, rng, nprog, nstack, capv, ips, lambda X: h.mkc_sess_loc_kind(src._h, k0, X))
            if what:
                break
        assert what
        k = promote(d, j, flat, ent)
        reg_total += what == "free"
        assert not (what == "free" and k < 0), (name, j, kind, "a register or dead location takes any value")
        if k < 0:
            refused += 1
            continue
        accepted += 1
        o = po.OracleSessions(net, 1, stack_cap=cap)
        o.import_state(0, flat)
        o.cancel()
        oracles[j] = o
        keep.append((flat, ent))
    print(f"{name}: accepted {accepted} refused {refused} (changes of register or dead locations: {reg_total})")
    live = np.ones(200, bool)
    for seed in (1003, 1004, 1005):
        x = po.gen_inputs(seed, 200, **gen)
        got, base = d.call(x, budget=budget), fresh.call(x, budget=budget)
        for j in range(200):
            if j in oracles:
                if live[j]:
                    want = oracles[j].compute([x[j]], budget=budget)
                    _same_or_handoff([r[j] for r in got], [r[0] for r in want], j, live, (name, seed, j))
            else:  # refused: nothing of the slot changed
                assert all(r[j] == b[j] for r, b in zip(got, base)), (name, seed, j)
    assert accepted + refused == 200


# ---- 5: an open call does not promote ----------------------------------------
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_handoff_export_does_not_promote(name):
    nodes, cap, budget, gen, _ = MODEL_NETS[name]()
    a, _, _, handed, _ = _prefix(nodes, cap, budget, gen)
    b = SnapSessions(nodes, 1, stack_cap=cap)
    assert handed.sum() >= 50
    for i in np.nonzero(handed)[0]:
        flat, ent = a.export(int(i), _nstack(nodes))
        assert promote(b, 0, flat, ent) == -1, (name, int(i))
    x = po.gen_inputs(1003, 1, **gen)
    got, want = b.call(x, budget=BIG), SnapSessions(nodes, 1, stack_cap=cap).call(x, budget=BIG)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))  # b's slot is still a fresh instance
