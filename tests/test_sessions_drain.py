"""Open calls finished on the GPU (mk_session_open_list, _resume_device,
_drain; SessionSet.open_list / resume_device / drain), against the CPU oracle.

The reference is the sequence that defines a drain (include/mk.h): a resume of
the listed instances, then of exactly those whose last status was
MK_ST_BUDGET, up to max_slices times, each entry reporting the last slice that
ran it -- run on test_sessions_indexed's n single-instance oracle sets.

n = 600: two full blocks and a 24-lane last wave; every list there takes the
one-block path of the compaction.  n = 10,840 = 4 * 2048 + 2048 + 600 is past
the 8,192 words one block scans alone (req_group.h kSerialChunks * kScanTile),
so its flags go through the scan's three kernels, and is neither a tile nor a
wave multiple; the scan has no further level."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, SEL, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)

ALL = SEL["all"]
DRAIN = ["mk_session_open_list", "mk_session_open_list_device", "mk_session_resume_device", "mk_session_drain",
         "mk_session_drain_device"]
BUDGET = N.MK_ST_BUDGET
PAD = 0xFFFFFFFF
NBIG = 4 * 2048 + 2048 + 600


# ---- CPU: the ABI is there, refuses a null session; the adapter checks first ----
def test_drain_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in DRAIN:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    buf = np.zeros(8, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)
    cnt = C.c_size_t()
    assert lib.mk_session_open_list(None, bp, 1, bp, bp, C.byref(cnt)) == N.MK_EINVAL
    assert lib.mk_session_open_list_device(None, bp, 1, bp, bp, bp, None) == N.MK_EINVAL
    assert lib.mk_session_resume_device(None, bp, 1, bp, bp, bp, None) == N.MK_EINVAL
    assert lib.mk_session_drain(None, bp, 1, 4, bp, bp, bp, C.byref(cnt)) == N.MK_EINVAL
    assert lib.mk_session_drain_device(None, bp, 1, 4, bp, bp, bp, bp, None) == N.MK_EINVAL


def test_drain_and_open_list_check_before_the_library():
    # no handle: anything that reached the library would be an AttributeError
    S = mk.network.SessionSet
    s = types.SimpleNamespace(n=10)
    s._index = functools.partial(S._index, s)
    s._listed = functools.partial(S._listed, s)
    for bad in (0, -1, 1 << 32):
        with pytest.raises(ValueError, match="max_slices"):
            S.drain(s, max_slices=bad)
        with pytest.raises(ValueError, match="max_slices"):
            S.drain_device(s, bad, 1, 1)
    for bad, pos in (([1, 4, 4, 2], 2), ([0, 10], 1), ([-1, 2], 0), (list(range(11)), 10)):
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            S.drain(s, index=bad)
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            S.open_list(s, index=bad)
    for f in (lambda **kw: S.open_list_device(s, 1, 1, 1, **kw), lambda **kw: S.resume_device(s, 1, 1, **kw),
              lambda **kw: S.drain_device(s, 4, 1, 1, **kw)):
        with pytest.raises(ValueError, match="go together"):
            f(m=3)
        with pytest.raises(ValueError, match="go together"):
            f(index_ptr=1)
        with pytest.raises(ValueError, match="outside"):
            f(index_ptr=1, m=11)


# ---- the reference ----------------------------------------------------------
def ref_drain(r, sel, max_slices):
    """The defining sequence on the oracle sets: ((out, status, steps), still_open)."""
    sel = np.asarray(sel, np.int64)
    out, st, sp = r.call(sel, None)
    for _ in range(1, max_slices):
        k = np.flatnonzero(st == BUDGET)
        if not k.size:
            break
        out[k], st[k], sp[k] = r.call(sel[k], None)
    return (out, st, sp), int((st == BUDGET).sum())


def _pair(name, tier="native"):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(NS, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    return g, Ref(nodes, NS, **kw), gen


def _call(g, r, v, ctx):
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), ctx)


def _first_call(g, r, x, name):
    v = x(NS)
    if name == "stackloop7":
        v[::4] += 32  # past the budget, then past the stack's capacity: ended while the interpreter holds them
    _call(g, r, v, f"{name} call")


def _drain(g, r, ctx, *, index=None, max_slices=32):
    sel = ALL if index is None else index
    got = g.drain(index=index, max_slices=max_slices)
    want, left = ref_drain(r, sel, max_slices)
    assert_same(got, want, ctx)
    assert got.still_open == left, ctx
    return got


# ---- 1: drain to the end, both tiers ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown150", "countdown1000", "stackloop7"])
def test_drain_to_the_end(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    x = _Inputs(gen, 12000)
    _first_call(g, r, x, name)
    opened = int(r.open.sum())
    assert opened >= 50
    got = _drain(g, r, f"{name} drain")
    print(f"{name} {tier}: {opened} open calls drained, {int((got.status == N.MK_ST_STACK_OVERFLOW).sum())} ended")
    assert got.still_open == 0 and not r.open.any()  # the cap of 32 slices hid nothing
    assert not g.call_open().any()
    assert name != "stackloop7" or (got.status == N.MK_ST_STACK_OVERFLOW).sum() >= 50
    # nothing open: a second drain reports what a resume does, the ended instances as ended
    _drain(g, r, f"{name} drain of nothing")
    _call(g, r, x(NS), f"{name} plain call")
    g.close()


# ---- 2: the slice limit -----------------------------------------------------
@pytest.mark.gpu
def test_drain_stops_at_the_slice_limit(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 13000)
    _first_call(g, r, x, "countdown150")
    got = _drain(g, r, "four slices", max_slices=4)
    assert got.still_open > 50 and got.still_open == int(r.open.sum())
    assert np.array_equal(g.call_open(), r.open)
    was_open = r.open.copy()
    v = x(NS)
    busy = g.compute(v, busy_ok=True)
    assert_same(busy, r.call(ALL, v), "call between the drains")
    assert np.array_equal(busy.status == N.MK_ST_CALL_OPEN, was_open == 1)
    got = _drain(g, r, "the rest")
    assert got.still_open == 0 and not g.call_open().any() and not r.open.any()
    _call(g, r, x(NS), "plain call")
    g.close()


# ---- 3: subsets -------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", ["empty", "first", "last", "even", "random257", "run"])
def test_drain_of_a_listed_subset(gpu, key):
    g, r, gen = _pair("countdown150")
    x = _Inputs(gen, 14000)
    _first_call(g, r, x, "countdown150")
    sel = SEL[key]
    got = _drain(g, r, f"drain {key}", index=sel)
    assert got.out.shape == (len(sel),) and got.still_open == 0
    assert not r.open[sel].any() and r.open.sum() >= 50
    assert np.array_equal(g.call_open(), r.open)  # unlisted open calls stay open
    _drain(g, r, "drain of all")
    assert not g.call_open().any() and not r.open.any()
    _call(g, r, x(NS), "plain call")
    g.close()


# ---- 4: the open list -------------------------------------------------------
def _check_open_list(g, r, ctx):
    lst, pos = g.open_list()
    assert lst.dtype == np.uint32 and pos.dtype == np.uint32
    assert np.array_equal(lst, np.flatnonzero(r.open)) and np.array_equal(pos, lst), ctx
    for key, sel in SEL.items():
        lst, pos = g.open_list(index=sel)
        assert np.array_equal(lst, sel[r.open[sel] == 1]), f"{ctx} {key}"
        assert np.array_equal(sel[pos], lst), f"{ctx} {key}"


@pytest.mark.gpu
def test_open_list(gpu, tier):
    import torch

    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 15000)
    _check_open_list(g, r, "fresh")
    _first_call(g, r, x, "countdown150")
    _check_open_list(g, r, "after the call")
    for k in range(3):
        assert_same(g.resume(), r.call(ALL, None), f"resume {k}")
    assert 50 <= r.open.sum() <= NS - 50
    _check_open_list(g, r, "after three resumes")
    # the device form: padded to m, and usable as the list of an indexed launch as it stands
    for key in ("all", "random257", "run"):
        sel = SEL[key]
        m = len(sel)
        d_sel = torch.from_numpy(sel.astype(np.int32)).cuda()
        d_list = torch.full((m,), 7, dtype=torch.int32, device="cuda")
        d_pos = torch.full((m,), 7, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        if key == "all":
            g.open_list_device(d_list.data_ptr(), d_pos.data_ptr(), d_cnt.data_ptr())
        else:
            g.open_list_device(d_list.data_ptr(), d_pos.data_ptr(), d_cnt.data_ptr(), index_ptr=d_sel.data_ptr(), m=m)
        torch.cuda.synchronize()
        want = sel[r.open[sel] == 1]
        c = int(d_cnt.cpu().numpy().view(np.uint32)[0])
        lst, pos = d_list.cpu().numpy().view(np.uint32), d_pos.cpu().numpy().view(np.uint32)
        assert c == len(want) and np.array_equal(lst[:c], want) and np.array_equal(sel[pos[:c]], want), key
        assert (lst[c:] == PAD).all() and (pos[c:] == 0).all() and c < m, key
    # the list alone (no pos), then a device resume over the padded list: the padding is dropped
    d_list = torch.full((NS,), 7, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((NS,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((NS,), 7, dtype=torch.uint8, device="cuda")
    sp = torch.full((NS,), 7, dtype=torch.int32, device="cuda")
    g.open_list_device(d_list.data_ptr(), None, d_cnt.data_ptr())
    g.resume_device(out.data_ptr(), st.data_ptr(), sp.data_ptr(), index_ptr=d_list.data_ptr(), m=NS)
    torch.cuda.synchronize()
    want = np.flatnonzero(r.open)
    c = len(want)
    assert int(d_cnt.cpu()[0]) == c and np.array_equal(d_list.cpu().numpy().view(np.uint32)[:c], want)
    got = mk.network.BatchResult(out.cpu().numpy()[:c], st.cpu().numpy()[:c], sp.cpu().numpy()[:c].astype(np.uint32))
    assert_same(got, r.call(want, None), "resume over the device list")
    assert not out.cpu().numpy()[c:].any() and not st.cpu().numpy()[c:].any() and not sp.cpu().numpy()[c:].any()
    _check_open_list(g, r, "after the listed resume")
    g.close()


@pytest.mark.gpu
def test_open_list_and_drain_with_nothing_open(gpu, tier):
    g, r, gen = _pair("example", tier)
    x = _Inputs(gen, 15500)
    _call(g, r, x(NS), "call")
    lst, pos = g.open_list()
    assert lst.size == 0 and pos.size == 0
    got = _drain(g, r, "drain")
    assert got.still_open == 0 and not got.status.any() and not got.out.any() and not got.steps.any()
    assert g.drain(steps=False).steps is None
    _call(g, r, x(NS), "plain call")
    g.close()


# ---- 5: the device forms on a second stream ---------------------------------
@pytest.mark.gpu
def test_drain_device_between_calls_on_another_stream(gpu, tier):
    import torch

    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 16000)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    v = [x(NS), x(NS)]
    d_in = [torch.from_numpy(a).cuda() for a in v]
    bufs = [(torch.full((NS,), 7, dtype=torch.int32, device="cuda"), torch.full((NS,), 7, dtype=torch.uint8, device="cuda"),
             torch.full((NS,), 7, dtype=torch.int32, device="cuda")) for _ in range(3)]
    d_left = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.compute_device(d_in[0].data_ptr(), *(b.data_ptr() for b in bufs[0]), stream=s1.cuda_stream)
    g.drain_device(24, *(b.data_ptr() for b in bufs[1]), d_left.data_ptr(), stream=s2.cuda_stream)
    g.compute_device(d_in[1].data_ptr(), *(b.data_ptr() for b in bufs[2]), stream=s1.cuda_stream)
    open_after = g.call_open()  # a host form: ordered after the three
    torch.cuda.synchronize()
    want = [r.call(ALL, v[0])]
    assert r.open.sum() >= 50
    want.append(ref_drain(r, ALL, 24)[0])
    assert not r.open.any()
    want.append(r.call(ALL, v[1]))
    for (out, st, sp), w, ctx in zip(bufs, want, ("first call", "drain", "second call")):
        got = mk.network.BatchResult(out.cpu().numpy(), st.cpu().numpy(), sp.cpu().numpy().astype(np.uint32))
        assert_same(got, w, ctx)
    assert int(d_left.cpu()[0]) == 0
    assert np.array_equal(open_after, r.open)
    g.close()


@pytest.mark.gpu
def test_drain_device_listed_with_a_slice_limit_and_resume_device(gpu, tier):
    import torch

    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 16500)
    _first_call(g, r, x, "countdown150")
    out = torch.full((NS,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((NS,), 7, dtype=torch.uint8, device="cuda")
    sp = torch.full((NS,), 7, dtype=torch.int32, device="cuda")

    def result(m):
        torch.cuda.synchronize()
        return mk.network.BatchResult(out.cpu().numpy()[:m], st.cpu().numpy()[:m], sp.cpu().numpy()[:m].astype(np.uint32))

    # resume_device with a null list is resume()
    g.resume_device(out.data_ptr(), st.data_ptr(), sp.data_ptr())
    assert_same(result(NS), r.call(ALL, None), "resume_device")
    # a listed drain with a limit, an entry that names no instance in the list, no steps wanted
    sel = SEL["random257"]
    lst = np.concatenate([sel, [NS + 3, PAD]]).astype(np.uint32)
    m = len(lst)
    d_sel = torch.from_numpy(lst.view(np.int32)).cuda()
    d_left = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    sp.fill_(7)
    g.drain_device(3, out.data_ptr(), st.data_ptr(), None, d_left.data_ptr(), index_ptr=d_sel.data_ptr(), m=m)
    got = result(m)
    want, left = ref_drain(r, sel, 3)
    assert left >= 20 and int(d_left.cpu()[0]) == left
    assert np.array_equal(got.out[:-2], want[0]) and np.array_equal(got.status[:-2], want[1])
    assert not got.out[-2:].any() and not got.status[-2:].any()
    assert (got.steps == 7).all()  # no steps array given: none written
    assert np.array_equal(g.call_open(), r.open)
    _drain(g, r, "the rest")
    _call(g, r, x(NS), "plain call")
    g.close()


# ---- 6: past one tile and past the serial scan -------------------------------
@pytest.mark.gpu
def test_drain_and_open_list_past_the_serial_scan(gpu):
    nodes, kw, gen = NETS["countdown150"]()
    n = NBIG
    g = mk.Network(nodes).sessions(n, **kw)
    o = po.OracleSessions(po.OracleNet(nodes), n)
    v = po.gen_inputs(17001, n, **gen)
    first = o.compute(v, budget=kw["budget"], threads=8)
    assert_same(g.compute(v, busy_ok=True), first, "call")
    is_open = first[1] == BUDGET
    assert is_open.sum() > 8192  # the list itself is past the serial scan too
    lst, pos = g.open_list()
    assert np.array_equal(lst, np.flatnonzero(is_open)) and np.array_equal(pos, lst)
    # the reference: the whole set resumed slice after slice; an instance's last slice is its answer
    out, st, sp = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    todo, slices = is_open.copy(), 0
    while todo.any():
        a, b, c = o.compute(None, budget=kw["budget"], threads=8)
        out[todo], st[todo], sp[todo] = a[todo], b[todo], c[todo]
        todo &= b == BUDGET
        slices += 1
    assert 2 <= slices <= 32
    third = np.arange(0, n, 3)
    lst3, pos3 = g.open_list(index=third)
    assert np.array_equal(lst3, third[is_open[third]]) and np.array_equal(third[pos3], lst3)
    got = g.drain(index=third, max_slices=32)
    assert_same(got, (out[third], st[third], sp[third]), "drain of every third")
    assert got.still_open == 0
    rest = is_open.copy()
    rest[third] = False
    assert np.array_equal(g.call_open(), rest.astype(np.uint8))
    got = g.drain(max_slices=32)
    for a in (out, st, sp):
        a[third] = 0  # closed by the first drain: nothing to resume
    assert_same(got, (out, st, sp), "drain of all")
    assert got.still_open == 0 and not g.call_open().any()
    v = po.gen_inputs(17002, n, **gen)
    assert_same(g.compute(v, busy_ok=True), o.compute(v, budget=kw["budget"], threads=8), "plain call")
    g.close()


# ---- 7: refusals, and promote=True ------------------------------------------
@pytest.mark.gpu
def test_drain_refusals(gpu):
    import torch

    # a mixed deployment: the host serves the peers between slices
    net = mk.Network([("g", "program", "IN ACC\nPUSH ACC, s\nPOP s, ACC\nOUT ACC"), ("s", "remote_stack", "")])
    h = net.sessions(8)
    with pytest.raises(N.MkError) as e:
        h.drain()
    assert e.value.code == N.MK_EINVAL
    d = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert N.lib().mk_session_drain_device(h._h, None, 8, 4, d.data_ptr(), d.data_ptr(), None, None, None) == N.MK_EINVAL
    h.close()
    g, r, gen = _pair("countdown150")
    x = _Inputs(gen, 18000)
    _first_call(g, r, x, "countdown150")
    lib = N.lib()
    buf = np.zeros(2 * NS + 2, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)
    cnt = C.c_size_t()
    assert lib.mk_session_drain(g._h, None, NS, 0, bp, bp, bp, None) == N.MK_EINVAL
    assert lib.mk_session_drain_device(g._h, None, NS, 0, d.data_ptr(), d.data_ptr(), None, None, None) == N.MK_EINVAL
    assert lib.mk_session_drain(g._h, None, NS - 1, 4, bp, bp, bp, None) == N.MK_EINVAL  # a null list is all n
    assert lib.mk_session_open_list(g._h, None, NS - 1, bp, bp, C.byref(cnt)) == N.MK_EINVAL
    for f in (lib.mk_session_open_list_device, lib.mk_session_resume_device):
        assert f(g._h, None, NS - 1, d.data_ptr(), d.data_ptr(), d.data_ptr(), None) == N.MK_EINVAL
    for bad in ([3, 3], [5, 4], [0, NS], list(range(NS + 1))):
        with pytest.raises(ValueError):
            g.drain(index=bad)
        with pytest.raises(ValueError):
            g.open_list(index=bad)
        sel = np.array(bad, np.uint32)
        sp = sel.ctypes.data_as(C.c_void_p)
        assert lib.mk_session_drain(g._h, sp, len(bad), 4, bp, bp, bp, None) == N.MK_EINVAL
        assert lib.mk_session_open_list(g._h, sp, len(bad), bp, bp, C.byref(cnt)) == N.MK_EINVAL
    # nothing listed: nothing launched
    assert g.drain(index=[]).out.shape == (0,) and g.open_list(index=[])[0].size == 0
    assert lib.mk_session_drain_device(g._h, d.data_ptr(), 0, 4, None, None, None, None, None) == N.MK_OK
    assert np.array_equal(g.call_open(), r.open) and r.open.sum() >= 50  # none of that touched a call
    _drain(g, r, "drain")
    _call(g, r, x(NS), "plain call")
    g.close()


@pytest.mark.gpu
def test_drain_then_promote(gpu):
    g, r, gen = _pair("countdown1000")
    x = _Inputs(gen, 19000)
    _first_call(g, r, x, "countdown1000")
    assert r.open.sum() >= 50 and not g.snapshot().held.all()
    got = g.drain(max_slices=32, promote=True)
    assert_same(got, ref_drain(r, ALL, 32)[0], "drain")
    assert got.still_open == 0
    assert g.snapshot().held.all()
    _call(g, r, x(NS), "call after the promotion")
    g.close()
