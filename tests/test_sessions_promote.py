"""Promotion on the GPU (mk_session_promote, SessionSet.promote): instances the
interpreter holds between calls go back to the native tier, against the CPU
oracle.  The reference is test_sessions_indexed's: n single-instance oracle
sets; its ``held`` marks the instances a budget slice handed to the
interpreter, which is what a promotion must find and take back.  Promotion
changes no result, so every call after one is compared bit-exactly.

n = 600: two full blocks and a partial one, a ragged last wave for the
per-wave count of promoted instances."""
import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, SEL, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)

ALL = SEL["all"]
BIG = 1 << 20


def _pair(name, tier="native", **over):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(NS, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    return g, Ref(nodes, NS, **dict(kw, **over)), gen


def _call(g, r, v, ctx):
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), ctx)


def _close_calls(g, r, ctx):
    """resume() until no call is open, at most 16 times, then cancel what is
    left; the reference does the same.  Returns the instances cancelled."""
    for k in range(16):
        if not r.open.any():
            break
        assert_same(g.resume(), r.call(ALL, None), f"{ctx} resume {k}")
    assert np.array_equal(g.call_open(), r.open), ctx
    left = np.nonzero(r.open)[0]
    if left.size:
        g.cancel()
        r.cancel(left)
    assert not g.call_open().any(), ctx
    return left


# ---- 6: cycles of calls, resumes and a promotion of everything ---------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7", "random19"])
def test_promote_cycles(gpu, name):
    g, r, gen = _pair(name)
    x = _Inputs(gen, 6000)
    for cycle in range(3):
        ctx = f"{name} cycle {cycle}"
        for c in range(2):
            v = x(NS)
            if name == "stackloop7" and cycle == 0 and c == 0:
                # this network's generator stops at 15, which no call turns into an overflow after a
                # hand-off: its loop takes 3 off the input per round and pushes once on each stack, so
                # from 32 on a call passes the budget of 40 steps (handed off) and then the capacity
                # of 8 (ended on the interpreter).  Every fourth instance: ended and interpreter-held.
                v[::4] += 32
            _call(g, r, v, f"{ctx} call {c}")
        cancelled = _close_calls(g, r, ctx)
        if name != "random19":
            assert cancelled.size == 0  # from the reference: every call of these networks ends
        clean = np.ones(NS, bool)
        clean[cancelled] = False
        flags = g.promote()
        print(f"{ctx}: held {int(r.held.sum())} promoted {int(flags.sum())} of them ended "
              f"{int((flags & r.dead).sum())} cancelled {cancelled.size}")
        assert flags.dtype == bool and flags.shape == (NS,)
        assert np.array_equal(flags[clean], r.held[clean]), ctx  # interpreter-held and eligible, ended ones included
        assert not (flags & ~r.held).any(), ctx
        if cycle == 0 and name != "random19":
            assert flags.sum() >= 50
            assert name != "stackloop7" or (flags & r.dead).sum() >= 50  # ended ones go back as ended
        r.held[flags] = False
        assert np.array_equal(g.snapshot().held, ~r.held), ctx
        if name != "random19":
            assert g.snapshot().held.all(), ctx
    _call(g, r, x(NS), f"{name} last call")
    g.close()


# ---- 7: a listed subset ------------------------------------------------------
@pytest.mark.gpu
def test_promote_subset_then_the_rest(gpu):
    g, r, gen = _pair("countdown1000")
    x = _Inputs(gen, 7000)
    for c in range(2):
        _call(g, r, x(NS), f"call {c}")
    assert _close_calls(g, r, "prefix").size == 0
    sel = SEL["random257"]
    listed = np.zeros(NS, bool)
    listed[sel] = True
    before = g.snapshot().held
    assert np.array_equal(before, ~r.held) and (r.held & listed).sum() >= 50 and (r.held & ~listed).sum() >= 50
    flags = g.promote(index=sel)
    assert flags.shape == (len(sel),) and np.array_equal(flags, r.held[sel])
    after = g.snapshot().held
    assert np.array_equal(after[~listed], before[~listed]) and not after[~listed & r.held].any()
    assert after[sel].all()
    r.held[sel] = False
    _call(g, r, np.zeros(NS, np.int64), "plain call")  # countdown from 0: hands nothing off
    rest = g.promote()
    assert np.array_equal(rest, r.held) and np.array_equal(rest, ~listed & ~before)
    assert g.snapshot().held.all()
    _call(g, r, x(NS), "last call")
    g.close()


# ---- 8: what is not eligible stays -------------------------------------------
@pytest.mark.gpu
def test_promote_leaves_open_calls_alone(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 8000)
    _call(g, r, x(NS), "call")
    for k in range(2):  # some of the open calls close: interpreter-held (on the native tier) and eligible
        assert_same(g.resume(), r.call(ALL, None), f"resume {k}")
    is_open = r.open == 1
    assert is_open.sum() >= 50 and (r.held & ~is_open).sum() >= 20
    flags = g.promote()
    assert not flags[is_open].any()
    assert np.array_equal(flags, r.held & ~is_open if tier == "native" else np.zeros(NS, bool))
    assert np.array_equal(g.call_open(), r.open)
    r.held[flags] = False
    assert_same(g.resume(), r.call(ALL, None), "resume after promote")
    _call(g, r, x(NS), "last call")
    g.close()


@pytest.mark.gpu
def test_promote_after_cancel_changes_no_result(gpu):
    g, r, gen = _pair("random6")  # some of its calls never end
    x = _Inputs(gen, 8500)
    for c in range(3):  # the third call of this network does not end
        _call(g, r, x(NS), f"call {c}")
    assert r.open.sum() >= 50
    g.cancel()
    r.cancel(np.nonzero(r.open)[0])
    before = g.snapshot().held
    flags = g.promote()
    after = g.snapshot().held
    print(f"random6: held {int((~before).sum())} promoted after a cancel {int(flags.sum())}")
    assert np.array_equal(after & ~before, flags) and np.array_equal(after | flags, after) and not (before & ~after).any()
    for c in range(3):
        _call(g, r, x(NS), f"call {c} after promote")
    g.close()


# ---- 9: migration from the interpreter's tier --------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["example", "countdown1000", "stackloop7"])
def test_promote_after_migration_takes_every_instance(gpu, name, monkeypatch):
    nodes, kw, gen = NETS[name]()
    net = mk.Network(nodes)
    monkeypatch.setenv("MK_SESSION_NATIVE", "0")
    src = net.sessions(NS, **dict(kw, budget=BIG))  # every call closes
    monkeypatch.delenv("MK_SESSION_NATIVE")
    assert src.plan().startswith("tier=interp")
    r = Ref(nodes, NS, **dict(kw, budget=BIG))
    x = _Inputs(gen, 9000)
    for c in range(2):
        _call(src, r, x(NS), f"{name} source call {c}")
    assert not r.open.any()
    snap = src.snapshot()
    src.close()
    g = net.sessions(NS, **kw)
    assert g.plan().startswith("tier=native")
    g.restore(snap)
    assert not g.snapshot().held.any()
    flags = g.promote()
    assert flags.all(), f"{name}: {int((~flags).sum())} states of plain calls did not promote"
    print(f"{name}: promoted {int(flags.sum())}, of them ended {int(r.dead.sum())}")
    assert name != "stackloop7" or r.dead.sum() >= 50  # ended instances go back as ended
    assert g.snapshot().held.all()
    r.budget = kw.get("budget")
    for c in range(3):
        _call(g, r, x(NS), f"{name} call {c} after promote")
    g.close()


# ---- 10: the device form, ordering, degenerate inputs ------------------------
@pytest.mark.gpu
def test_promote_device_between_calls_on_another_stream(gpu):
    import torch

    g, r, gen = _pair("countdown1000")
    x = _Inputs(gen, 10000)
    _call(g, r, x(NS), "prefix call")
    assert _close_calls(g, r, "prefix").size == 0 and r.held.sum() >= 50
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    v = [x(NS), np.zeros(NS, np.int64)]  # the second call from 0: it closes, whichever tier runs it
    d_in = [torch.from_numpy(a).cuda() for a in v]
    bufs = [(torch.empty(NS, dtype=torch.int32, device="cuda"), torch.empty(NS, dtype=torch.uint8, device="cuda"),
             torch.empty(NS, dtype=torch.int32, device="cuda")) for _ in v]
    d_flags = torch.full((NS,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.compute_device(d_in[0].data_ptr(), *(b.data_ptr() for b in bufs[0]), stream=s1.cuda_stream)
    g.promote_device(d_flags.data_ptr(), stream=s2.cuda_stream)
    g.compute_device(d_in[1].data_ptr(), *(b.data_ptr() for b in bufs[1]), stream=s1.cuda_stream)
    held_after = g.snapshot().held  # a host form: ordered after the three
    torch.cuda.synchronize()
    want0 = r.call(ALL, v[0])
    eligible = r.held & (r.open == 0)
    assert eligible.sum() >= 50 and r.open.sum() >= 50
    want1 = r.call(ALL, v[1])
    for (out, st, sp), want, ctx in zip(bufs, (want0, want1), ("first", "second")):
        got = mk.network.BatchResult(out.cpu().numpy(), st.cpu().numpy(), sp.cpu().numpy().astype(np.uint32))
        assert_same(got, want, f"{ctx} device call")
    assert np.array_equal(d_flags.cpu().numpy(), eligible.astype(np.uint8))
    assert np.array_equal(held_after, ~(r.held & ~eligible))
    g.close()


@pytest.mark.gpu
def test_promote_degenerate_inputs(gpu, tier):
    import torch

    g, r, gen = _pair("countdown1000", tier)
    x = _Inputs(gen, 11000)
    _call(g, r, x(NS), "call")
    _close_calls(g, r, "prefix")
    assert r.held.sum() >= 50
    before = g.snapshot()
    # nothing listed: nothing launched, nothing changed
    assert g.promote(index=[]).shape == (0,)
    d_none = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert N.lib().mk_session_promote_device(g._h, d_none.data_ptr(), 0, None, None) == N.MK_OK
    assert N.lib().mk_session_promote_device(g._h, None, NS - 1, None, None) == N.MK_EINVAL  # a null list is all n
    for bad in ([3, 3], [5, 4], [0, NS], list(range(NS + 1))):
        with pytest.raises(ValueError):
            g.promote(index=bad)
    assert np.array_equal(g.snapshot().rec, before.rec)
    # a device list with entries that name no instance: they report 0 and touch nothing
    held = np.nonzero(r.held)[0]
    lst = np.array([held[0], held[1], NS, NS + 7, 0xFFFFFFFF], np.uint32)
    d_sel = torch.from_numpy(lst.view(np.int32)).cuda()
    d_flags = torch.full((len(lst),), 7, dtype=torch.uint8, device="cuda")
    g.promote_device(d_flags.data_ptr(), index_ptr=d_sel.data_ptr(), m=len(lst))
    after = g.snapshot()  # ordered after the device form
    took = tier == "native"
    assert d_flags.cpu().numpy().tolist() == [int(took), int(took), 0, 0, 0]
    changed = np.nonzero((after.rec != before.rec).any(axis=0))[0]
    assert set(changed.tolist()) == (set(lst[:2].tolist()) if took else set())
    if took:
        r.held[lst[:2]] = False
    flags = g.promote()
    assert np.array_equal(flags, r.held if took else np.zeros(NS, bool))
    # every instance promoted: a snapshot / restore round trip is word-identical
    full = g.snapshot()
    assert full.held.all() == took
    g.restore(full)
    assert np.array_equal(g.snapshot().rec, full.rec)
    r.held[:] = r.held & (not took)
    _call(g, r, x(NS), "last call")
    g.close()
