"""Indexed session launches (mk_session_*_indexed, SessionSet(..., index=)):
calls, resumes, cancels and resets on a chosen subset of a session set's
instances, against the CPU oracle.

The instances of a set are independent, so the reference is a list of n
single-instance oracle sets of which only the listed ones are stepped; out,
status and steps are compared bit-exactly.  Every scenario ends with a plain
call on all n instances: the proof that the unlisted ones kept their state
and that plain and indexed launches interleave.

n = 600 is two full blocks of 256 threads and a partial one; the selections
cover the empty list, single entries at both ends, a stride, the identity, a
random list of 257 (one full block and a one-thread tail, its gaps crossing
the block boundaries of the state index) and a contiguous run that starts
mid-block."""
import ctypes as C
import types

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from test_gpu_parity import assert_same
from tisgen import random_network, stack_loop_network

NS = 600
INDEXED = ["mk_session_compute_indexed", "mk_session_step_indexed", "mk_session_compute_indexed_device",
           "mk_session_cancel_indexed", "mk_session_reset_indexed", "mk_session_call_open"]


# ---- CPU: the ABI is there and refuses a null session -----------------------
def test_indexed_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in INDEXED:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    sel = np.zeros(1, np.uint32)
    buf = np.zeros(8, np.int64)
    sp, bp = sel.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    assert lib.mk_session_compute_indexed(None, sp, 1, bp, 1, bp, bp, bp) == N.MK_EINVAL
    assert lib.mk_session_step_indexed(None, sp, 1, bp, bp, bp, bp) == N.MK_EINVAL
    assert lib.mk_session_compute_indexed_device(None, sp, 1, bp, 1, bp, bp, bp, None) == N.MK_EINVAL
    assert lib.mk_session_cancel_indexed(None, sp, 1) == N.MK_EINVAL
    assert lib.mk_session_reset_indexed(None, sp, 1) == N.MK_EINVAL
    assert lib.mk_session_call_open(None, sp, 1, bp) == N.MK_EINVAL


def test_index_errors_name_the_first_offending_position():
    s = types.SimpleNamespace(n=10)
    check = mk.network.SessionSet._index
    assert check(s, [0, 3, 9]).dtype == np.uint32 and check(s, []).size == 0
    for bad, pos in (([1, 4, 4, 2], 2), ([0, 5, 4, 3], 2), ([0, 10], 1), ([-1, 2], 0), (list(range(11)), 10)):
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            check(s, bad)
    with pytest.raises(ValueError):
        check(s, [0.5])


# ---- the reference: n single-instance oracle sets ---------------------------
class Ref:
    def __init__(self, nodes, n, budget=None, stack_cap=None):
        net = po.OracleNet(nodes)
        self.o = [po.OracleSessions(net, 1, stack_cap=stack_cap) for _ in range(n)]
        self.n, self.budget = n, budget
        self.open = np.zeros(n, np.uint8)   # a call is open (mk_session_call_open)
        self.held = np.zeros(n, bool)       # a call ran out of its budget slice since the last reset
        self.dead = np.zeros(n, bool)       # ended by a stack overflow

    def call(self, sel, values):
        """One call on the listed instances (values None: resume)."""
        m = len(sel)
        out, st, sp = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.uint32)
        for t, i in enumerate(sel):
            o, s, p = self.o[i].compute(None if values is None else [values[t]], budget=self.budget)
            out[t], st[t], sp[t] = o[0], s[0], p[0]
            if s[0] != N.MK_ST_CALL_OPEN:
                self.open[i] = s[0] == N.MK_ST_BUDGET
            self.held[i] |= s[0] == N.MK_ST_BUDGET
            self.dead[i] |= s[0] == N.MK_ST_STACK_OVERFLOW
        return out, st, sp

    def cancel(self, sel):
        for i in sel:
            self.o[i].cancel()
            self.open[i] = 0

    def reset(self, sel):
        for i in sel:
            self.o[i].reset()
            self.open[i] = 0
            self.held[i] = self.dead[i] = False


def _selections(n=NS):
    r = np.random.default_rng(257)
    return {
        "empty": np.zeros(0, np.int64),
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "even": np.arange(0, n, 2),
        "all": np.arange(n),
        "random257": np.sort(r.choice(n, 257, replace=False)),
        "run": np.arange(200, 500),  # starts mid-block, crosses the boundaries at 256 and 512
    }


SEL = _selections()

# name -> (nodes, session options, oracle.gen_inputs options)
NETS = {
    "example": lambda: (mk.networks.example_network(), {}, {}),
    "countdown150": lambda: (mk.networks.countdown_network(), dict(budget=150), dict(kind=1, mask=1023)),
    "countdown1000": lambda: (mk.networks.countdown_network(), dict(budget=1000), dict(kind=1, mask=1023)),
    "random6": lambda: (random_network(6), dict(budget=37, stack_cap=1024), dict(kind=1, mask=1023)),
    "random19": lambda: (random_network(19), dict(budget=200, stack_cap=40), dict(kind=1, mask=1023)),
    # dynamic stacks (slots with stride n); stack_cap 8 ends some sessions, budget 40 hands others off
    "stackloop7": lambda: (stack_loop_network(7)[0], dict(budget=40, stack_cap=8), stack_loop_network(7)[1]),
}


@pytest.fixture(params=["native", "interp"])
def tier(request, monkeypatch):
    if request.param == "interp":
        monkeypatch.setenv("MK_SESSION_NATIVE", "0")
    return request.param


def _pair(name, tier):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(NS, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    return g, Ref(nodes, NS, **kw), gen


class _Inputs:
    def __init__(self, gen, seed):
        self.gen, self.seed = gen, seed

    def __call__(self, count):
        self.seed += 1
        return po.gen_inputs(self.seed, max(count, 1), **self.gen)[:count]


def _open_agrees(g, r, ctx):
    assert np.array_equal(g.call_open(), r.open), ctx
    sel = SEL["random257"]
    assert np.array_equal(g.call_open(index=sel), r.open[sel]), ctx


# ---- 1 (and 7): rounds on different selections, then a plain call -----------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_indexed_rounds_then_plain_call(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    x = _Inputs(gen, 1000)
    for k in ("even", "first", "empty", "random257", "run", "last", "all"):
        sel = SEL[k]
        v = x(len(sel))
        assert_same(g.compute(v, index=sel, busy_ok=True), r.call(sel, v), f"{name} round {k}")
    _open_agrees(g, r, "after the rounds")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(SEL["all"], v), f"{name} plain call")
    _open_agrees(g, r, "after the plain call")
    g.close()


# ---- 2: bursts, [call][m] ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_indexed_bursts_then_plain_call(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    x = _Inputs(gen, 2000)
    for k in ("random257", "empty", "run", "all"):
        sel = SEL[k]
        v = x(3 * len(sel)).reshape(3, len(sel))
        got = g.compute_seq(v, index=sel, busy_ok=True)
        assert got.out.shape == (3, len(sel))
        for c in range(3):
            assert_same(mk.network.BatchResult(got.out[c], got.status[c], got.steps[c]), r.call(sel, v[c]),
                        f"{name} burst {k} call {c}")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(SEL["all"], v), f"{name} plain call")
    _open_agrees(g, r, "after the bursts")
    g.close()


# ---- 3: open calls ----------------------------------------------------------
@pytest.mark.gpu
def test_indexed_open_calls_resume_busy_cancel(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 3000)
    a, b = SEL["even"], SEL["run"]
    v = x(len(a))
    assert_same(g.compute(v, index=a), r.call(a, v), "call on A")
    assert r.open[a].any() and not r.open[a].all() and not r.open[1::2].any()
    assert_same(g.resume(index=b), r.call(b, None), "resume B")
    rest = np.setdiff1d(a, b)
    assert r.open[rest].any()  # A's calls outside B were not advanced ...
    assert np.array_equal(g.call_open(index=rest), r.open[rest])  # ... and are still open
    _open_agrees(g, r, "after resume B")
    # a new call: MK_ST_CALL_OPEN for the entries with an open call only
    was_open = r.open.copy()
    c = SEL["random257"]
    v = x(len(c))
    got = g.compute(v, index=c, busy_ok=True)
    assert_same(got, r.call(c, v), "call on C")
    assert np.array_equal(got.status == N.MK_ST_CALL_OPEN, was_open[c] == 1) and was_open[c].any()
    # MK_EBUSY: raised for a listed open call, not for an unlisted one
    busy, idle = np.nonzero(r.open)[0], np.nonzero(r.open == 0)[0]
    d = np.sort(np.array([busy[0], idle[0]]))
    v = x(2)
    with pytest.raises(N.MkError) as e:
        g.compute(v, index=d)
    assert e.value.code == N.MK_EBUSY
    r.call(d, v)
    idle = np.nonzero(r.open == 0)[0][:50]
    v = np.zeros(len(idle), np.int64)  # countdown from 0: closes within the slice
    assert_same(g.compute(v, index=idle), r.call(idle, v), "call on idle instances")
    # cancel closes only the listed calls
    busy = np.nonzero(r.open)[0]
    k = busy[::2]
    g.cancel(index=k)
    r.cancel(k)
    assert r.open.any()
    _open_agrees(g, r, "after cancel")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(SEL["all"], v), "plain call")
    _open_agrees(g, r, "after the plain call")
    g.close()


# ---- 4: reset ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_indexed_reset(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    x = _Inputs(gen, 4000)

    def launch(k, ctx):
        sel = SEL[k]
        v = x(len(sel))
        assert_same(g.compute(v, index=sel, busy_ok=True), r.call(sel, v), f"{name} {ctx}")

    launch("all", "round 1")
    launch("even", "round 2")
    held, dead = np.nonzero(r.held)[0], np.nonzero(r.dead)[0]
    other = np.nonzero(~r.held & ~r.dead)[0]
    # sessions the interpreter holds (on the native tier: handed off at their budget), ended ones, the rest
    assert held.size > 40 and other.size > 20 and (name != "stackloop7" or dead.size > 20)
    rs = np.unique(np.concatenate([held[:20], held[-5:], dead[:20], other[:20], other[-5:]]))
    g.reset(index=rs)
    r.reset(rs)
    _open_agrees(g, r, "after reset R")
    launch("random257", "round 3")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(SEL["all"], v), f"{name} plain call 1")
    # every session the interpreter holds: none is left with it afterwards
    rs = np.nonzero(r.held)[0]
    assert rs.size
    g.reset(index=rs)
    r.reset(rs)
    _open_agrees(g, r, "after reset of every held session")
    launch("run", "round 4")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(SEL["all"], v), f"{name} plain call 2")
    _open_agrees(g, r, "at the end")
    g.close()


# ---- 5: the device form across streams --------------------------------------
@pytest.mark.gpu
def test_indexed_device_calls_across_streams(gpu, tier):
    import torch

    g, r, gen = _pair("countdown1000", tier)
    x = _Inputs(gen, 5000)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    plan = [("even", s1.cuda_stream), ("run", s2.cuda_stream), ("random257", None)]
    bufs, refs = [], []
    for k, _ in plan:
        sel = SEL[k]
        m = len(sel)
        v = x(m)
        refs.append(r.call(sel, v))
        d_sel = torch.from_numpy(sel.astype(np.int32)).cuda()  # int32 bits, read as uint32
        bufs.append((d_sel, torch.from_numpy(v).cuda(), torch.empty(m, dtype=torch.int32, device="cuda"),
                     torch.empty(m, dtype=torch.uint8, device="cuda"),
                     torch.empty(m, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for (k, stream), (d_sel, d_in, out, st, sp) in zip(plan, bufs):
        g.compute_device(d_in.data_ptr(), out.data_ptr(), st.data_ptr(), sp.data_ptr(), stream=stream,
                         index_ptr=d_sel.data_ptr(), m=d_sel.numel())
    v = x(NS)
    host = g.compute(v, index=SEL["all"], busy_ok=True)
    torch.cuda.synchronize()
    for (k, _), (_, _, out, st, sp), ref in zip(plan, bufs, refs):
        got = mk.network.BatchResult(out.cpu().numpy(), st.cpu().numpy(), sp.cpu().numpy().astype(np.uint32))
        assert_same(got, ref, f"device call {k}")
    assert_same(host, r.call(SEL["all"], v), "host call")
    _open_agrees(g, r, "at the end")
    g.close()


# ---- 6: bad lists through the host API --------------------------------------
@pytest.mark.gpu
def test_indexed_bad_lists_change_nothing(gpu, tier):
    g, r, gen = _pair("example", tier)
    x = _Inputs(gen, 6000)
    v = x(len(SEL["even"]))
    assert_same(g.compute(v, index=SEL["even"]), r.call(SEL["even"], v), "round")
    lib = N.lib()
    for bad in ([3, 3], [5, 4], [0, NS], list(range(NS + 1))):
        m = len(bad)
        for f in (lambda: g.compute(np.ones(m), index=bad), lambda: g.compute_seq(np.ones((2, m)), index=bad),
                  lambda: g.resume(index=bad), lambda: g.cancel(index=bad), lambda: g.reset(index=bad),
                  lambda: g.call_open(index=bad)):
            with pytest.raises(ValueError):
                f()
        sel = np.array(bad, np.uint32)
        buf = np.ones(2 * m, np.int64)
        sp, bp = sel.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
        assert lib.mk_session_compute_indexed(g._h, sp, m, bp, 2, bp, bp, bp) == N.MK_EINVAL
        assert lib.mk_session_step_indexed(g._h, sp, m, bp, bp, bp, bp) == N.MK_EINVAL
        assert lib.mk_session_step_indexed(g._h, sp, m, None, bp, bp, bp) == N.MK_EINVAL
        assert lib.mk_session_cancel_indexed(g._h, sp, m) == N.MK_EINVAL
        assert lib.mk_session_reset_indexed(g._h, sp, m) == N.MK_EINVAL
        assert lib.mk_session_call_open(g._h, sp, m, bp) == N.MK_EINVAL
    v = x(NS)
    assert_same(g.compute(v), r.call(SEL["all"], v), "plain call")
    g.close()
