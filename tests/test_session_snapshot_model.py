"""Session snapshots without a GPU: the ABI is there, and the record
conversion of a live session between calls (sess_record.h, the canonical part
of mk_session_snapshot for a session the native tier holds) is checked on the
schedule compiler's host model against the CPU oracle.

For every session that is idle after two calls -- neither handed off nor
ended -- the host model's state goes through its canonical record into a
fresh one-instance oracle; that oracle and the original one, which ran the
same two calls itself, must answer three further calls identically."""
import ctypes as C

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from schedcheck import HANDOFF
from snapcheck import SnapSessions
from tisgen import random_network, stack_loop_network

NS = 600
SNAPSHOT = ["mk_session_layout_get", "mk_session_snapshot", "mk_session_snapshot_device", "mk_session_restore",
            "mk_session_restore_device"]


def test_snapshot_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in SNAPSHOT:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    buf = np.zeros(64, np.uint32)
    bp = buf.ctypes.data_as(C.c_void_p)
    lay = N.mk_session_layout()
    assert C.sizeof(lay) == 48
    assert lib.mk_session_layout_get(None, C.byref(lay)) == N.MK_EINVAL
    assert lib.mk_session_snapshot(None, bp, 1, bp) == N.MK_EINVAL
    assert lib.mk_session_snapshot_device(None, bp, 1, bp, None) == N.MK_EINVAL
    assert lib.mk_session_restore(None, bp, 1, C.byref(lay), bp, 1, None) == N.MK_EINVAL
    assert lib.mk_session_restore_device(None, bp, 1, C.byref(lay), bp, 1, None, None) == N.MK_EINVAL
    for name in ("snapshot", "restore", "fork", "snapshot_device", "restore_device", "layout"):
        assert callable(getattr(mk.SessionSet, name))


# name -> (nodes, stack_cap, budget, gen options, measured idle / handed off / ended after the two calls)
MODEL_NETS = {
    "example": lambda: (mk.networks.example_network(), None, None, {}, (600, 0, 0)),
    "countdown1000": lambda: (mk.networks.countdown_network(), None, 1000, dict(kind=1, mask=1023), (84, 516, 0)),
    # the budget of test_sessions_indexed's entry: some later calls of this network never end on their own
    "random6": lambda: (random_network(6), 1024, 37, dict(kind=1, mask=1023), (600, 0, 0)),
    "stackloop7": lambda: (stack_loop_network(7)[0], 8, 40, stack_loop_network(7)[1], (382, 159, 59)),
}


def _nstack(nodes):
    return sum(1 for n in nodes if (n.kind if hasattr(n, "name") else n[1]) == "stack")


def _prefix(nodes, cap, budget, gen):
    """Two calls on the host model and on the oracle: (host, oracle, idle, handed, ended)."""
    host = SnapSessions(nodes, NS, stack_cap=cap)
    ref = po.OracleSessions(po.OracleNet(nodes), NS, stack_cap=cap)
    handed, ended = np.zeros(NS, bool), np.zeros(NS, bool)
    for seed in (1001, 1002):
        x = po.gen_inputs(seed, NS, **gen)
        _, st, _ = host.call(x, budget=budget)
        ref.compute(x, budget=budget)
        handed |= st == HANDOFF
        ended |= (st != HANDOFF) & ((st & N.MK_ST_REASON_MASK) == N.MK_ST_STACK_OVERFLOW)
    return host, ref, ~handed & ~ended, handed, ended


@pytest.mark.parametrize("name", list(MODEL_NETS))
def test_idle_export_matches_oracle(name):
    nodes, cap, budget, gen, mix = MODEL_NETS[name]()
    host, ref, idle, handed, ended = _prefix(nodes, cap, budget, gen)
    print(f"{name}: idle {idle.sum()} handed off {handed.sum()} ended {ended.sum()}")
    assert (int(idle.sum()), int(handed.sum()), int(ended.sum())) == mix
    assert idle.sum() >= 50
    net = po.OracleNet(nodes)
    probes = {}
    for i in np.nonzero(idle)[0]:
        flat, ent = host.export_idle(int(i), _nstack(nodes))
        o = po.OracleSessions(net, 1, stack_cap=cap)
        o.import_state(0, flat)
        o.cancel()  # the import marks a call open; the record has it closed
        probes[int(i)] = (o, flat, ent)
    checked = 0
    for seed in (1003, 1004, 1005):
        x = po.gen_inputs(seed, NS, **gen)
        want = ref.compute(x, budget=budget)
        for i, (o, _, _) in probes.items():
            got = o.compute([x[i]], budget=budget)
            assert tuple(int(a[0]) for a in got) == tuple(int(a[i]) for a in want), (name, seed, i)
            checked += 1
    assert checked == 3 * int(idle.sum())


@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_sess_copy_continues_identically(name):
    nodes, cap, budget, gen, _ = MODEL_NETS[name]()
    host, _, idle, handed, ended = _prefix(nodes, cap, budget, gen)
    # idle, handed-off and ended sources, each into a slot in another state
    src = np.concatenate([np.nonzero(idle)[0][:40], np.nonzero(handed)[0][:10], np.nonzero(ended)[0][:10]])
    dst = np.setdiff1d(np.arange(NS), src)[::-1][: src.size]
    for d, s in zip(dst, src):
        host.copy(int(d), int(s))
    for seed in (1003, 1004, 1005):
        x = po.gen_inputs(seed, NS, **gen)
        x[dst] = x[src]
        out, st, sp = host.call(x, budget=budget)
        assert np.array_equal(out[dst], out[src]) and np.array_equal(st[dst], st[src]) and \
            np.array_equal(sp[dst], sp[src]), (name, seed)
