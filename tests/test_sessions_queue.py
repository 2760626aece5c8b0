"""Request queues (mk_session_compute_queue, SessionSet.compute_queue): requests
in arrival order, (instance, value) pairs with instances repeated and unsorted,
grouped on the GPU (mk_requests_group_device) and served in one ragged launch,
every answer back at its own position.

The grouping is checked alone against numpy -- stable argsort, unique,
searchsorted, the padded tails and m, all exact -- at every total and n at
which the sort takes another path: a tile is 2048 requests (up to one tile a
single block does everything in one launch), the histogram
table of a pass is scanned by one block up to 4 chunks of 2048 words (16,384
and 65,536 requests are the last totals of the one-chunk and the one-block
scan), a pass covers 8 bits of n.  The session forms are checked against the
CPU oracle of test_sessions_indexed, served one request at a time or through
test_sessions_ragged's reference on numpy's grouping."""
import ctypes as C
import hashlib
import types

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)
from test_sessions_ragged import ref_ragged
from tisgen import stack_loop_network

QUEUE = ["mk_session_compute_queue", "mk_session_compute_queue_device", "mk_requests_group_tmp_bytes",
         "mk_requests_group_device"]
ALL = np.arange(NS)
# sha256 of the generated text of the two entries of a session module, computed on the commit before request
# queues (the same for every network: the entries are wrappers around the lane code)
PLAIN_ENTRY_SHA256 = "7938f5be9a48e89b441b852d948917b4453340b2a696677629ffecdcb5e7b988"
SEL_ENTRY_SHA256 = "71757f3b01d32e99c2231405a4a9b788a047c6d25edbe2ce09977eb527407f7a"
PLAIN_ENTRY = 'extern "C" __global__ void __launch_bounds__(256) mk_sess_exec(SessK p)'
SEL_ENTRY = 'extern "C" __global__ void __launch_bounds__(256) mk_sess_exec_sel(SessKSel q)'


def _reason(st):
    return np.asarray(st) & N.MK_ST_REASON_MASK


# ---- CPU ----------------------------------------------------------------------
def test_queue_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in QUEUE:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    ids = np.zeros(1, np.uint32)
    buf = np.zeros(8, np.int64)
    ip, bp = ids.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    assert lib.mk_session_compute_queue(None, ip, bp, 1, bp, bp, bp) == N.MK_EINVAL
    assert lib.mk_session_compute_queue_device(None, ip, bp, 1, bp, bp, bp, None) == N.MK_EINVAL


def test_group_tmp_bytes_nonzero_monotone_and_refuses_n0():
    import torch  # noqa: F401

    size = mk.network.group_requests_tmp_bytes
    for n in (1, 600, 70001, (1 << 32) - 1):
        got = [size(n, t) for t in (0, 1, 2048, 2049, 16385, 65537, 1100003)]
        assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[1] < got[-1], (n, got)
    with pytest.raises(N.MkError) as e:
        size(0, 10)
    assert e.value.code == N.MK_EINVAL
    b = C.c_size_t()
    assert N.lib().mk_requests_group_tmp_bytes(600, 1 << 32, C.byref(b)) == N.MK_EINVAL
    assert N.lib().mk_requests_group_device(0, 0, None, 0, None, None, None, None, None, 0, None) == N.MK_EINVAL


def test_queue_errors_name_the_first_offending_position():
    s = types.SimpleNamespace(n=10)
    check = mk.network.SessionSet._queue
    ids, v = check(s, [9, 0, 9, 3], [1, 2, 3, 4])
    assert ids.dtype == np.uint32 and ids.tolist() == [9, 0, 9, 3] and v.dtype == np.int64 and v.tolist() == [1, 2, 3, 4]
    ids, v = check(s, [], [])
    assert ids.size == 0 and v.size == 0
    for bad, values, pos in (
            ([1, 4, 10, 11], [0] * 4, 2),         # an id >= n, the first of two
            ([0, -1, 3], [0] * 3, 1),             # a negative id
            ([0, 2.0, 3], [0] * 3, 1),            # a float, even a whole one
            ([0.5, 2], [0] * 2, 0),
            (np.array([1.0, 2.0]), [0] * 2, 0),
            ([1, 2, 3], [0] * 2, 2),              # more ids than values
            ([1, 2], [0] * 5, 2)):                # more values than ids
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            check(s, bad, values)


def _entry(src, head):
    a = src.index(head)
    b = src.find('extern "C"', a + 1)
    return src[a:b if b >= 0 else len(src)]


def test_generated_session_entries_are_the_parents():
    import schedcheck as sc

    for nodes, kw in ((mk.networks.example_network(), {}), (mk.networks.countdown_network(), {}),
                      (stack_loop_network(7)[0], dict(stack_cap=8))):
        src = sc.session_module(nodes, **kw)
        assert hashlib.sha256(_entry(src, SEL_ENTRY).encode()).hexdigest() == SEL_ENTRY_SHA256
        assert hashlib.sha256(_entry(src, PLAIN_ENTRY).encode()).hexdigest() == PLAIN_ENTRY_SHA256


# ---- 1: the grouping against numpy ------------------------------------------------
TILE = 2048
TOTALS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 4095, 4096, 4097, 8191, 8192,
          8193, 16384, 16385, 16386,  # 16,385: the first histogram table of more than one scan chunk
          20000, 65536, 65537, 65538]  # 65,537: the first of more than one scan block
GROUP_NS = [1, 2, 255, 256, 257, 600, 65536, 70001, (1 << 24) + 1, (1 << 32) - 1]
PATTERNS = ["uniform", "equal", "decreasing", "sorted", "two", "invalid"]


def _invalid_pool(n):
    pool = [n, n + 1, 0xffffffff] + [n + (1 << k) for k in range(1, 32)]
    return np.array(sorted({x for x in pool if x < 1 << 32}), np.uint64)


def _ids(pattern, n, total, rng):
    if pattern == "uniform":
        return rng.integers(0, n, total, dtype=np.uint64).astype(np.uint32)
    if pattern == "equal":
        return np.full(total, n - 1, np.uint32)
    if pattern == "decreasing":  # strictly, where n has room for it
        top = max(n, total)
        a = top - 1 - np.arange(total, dtype=np.uint64)
        return np.minimum(a, 0xffffffff).astype(np.uint32)
    if pattern == "sorted":
        return np.sort(rng.integers(0, n, total, dtype=np.uint64)).astype(np.uint32)
    if pattern == "two":
        return np.where(np.arange(total) % 2 == 0, n - 1, n // 2).astype(np.uint32)
    ids = rng.integers(0, n, total, dtype=np.uint64)
    bad = rng.random(total) < 0.1
    ids[bad] = rng.choice(_invalid_pool(n), int(bad.sum()))
    return ids.astype(np.uint32)


def _expected(ids, n):
    total = ids.size
    key = np.minimum(ids.astype(np.uint64), n)
    perm = np.argsort(key, kind="stable")
    sk = key[perm]
    valid = int((sk < n).sum())
    sel = np.unique(sk[:valid])
    off = np.searchsorted(sk, sel, side="left")
    M = min(total, n)
    sel_pad, off_pad = np.full(M - sel.size, 0xffffffff, np.uint64), np.full(M + 1 - sel.size, valid, np.uint64)
    return (perm.astype(np.uint32), np.concatenate([sel, sel_pad]).astype(np.uint32),
            np.concatenate([off.astype(np.uint64), off_pad]).astype(np.uint32), sel.size)


def _group(torch, ids, n):
    total = ids.size
    M = min(total, n)
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    perm, sel, off, m = (torch.full((k,), -7, dtype=torch.int32, device="cuda") for k in (max(total, 1), max(M, 1),
                                                                                          M + 1, 1))
    nb = mk.network.group_requests_tmp_bytes(n, total)
    tmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    mk.network.group_requests_device(n, d_ids.data_ptr(), total, perm.data_ptr(), sel.data_ptr(), off.data_ptr(),
                                     m.data_ptr(), tmp.data_ptr(), nb, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    u32 = lambda t, k: t.cpu().numpy().view(np.uint32)[:k]  # noqa: E731
    return u32(perm, total), u32(sel, M), u32(off, M + 1), int(u32(m, 1)[0])


def _check_group(torch, ids, n, ctx):
    got, want = _group(torch, ids, n), _expected(ids, n)
    assert got[3] == want[3], (ctx, "m", got[3], want[3])
    for name, a, b in zip(("perm", "sel", "off"), got, want):
        if not np.array_equal(a, b):
            at = int(np.argmax(a != b)) if a.shape == b.shape else -1
            raise AssertionError(f"{ctx}: {name} differs first at {at}: got {a[at]}, want {b[at]}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", GROUP_NS)
def test_grouping_equals_numpy(gpu, n):
    import torch

    rng = np.random.default_rng(n % 9973)
    for total in TOTALS:
        # every pattern at the totals around a tile and the scan thresholds, two of them elsewhere
        edge = total in (1, 2, 65, TILE - 1, TILE, TILE + 1, 16385, 20000, 65537)
        for i, pattern in enumerate(PATTERNS):
            if edge or pattern == "invalid" or i == total % 5:
                _check_group(torch, _ids(pattern, n, total, rng), n, f"n {n} total {total} {pattern}")


@pytest.mark.gpu
def test_grouping_of_one_tile_through_the_tiled_kernels(gpu, monkeypatch):
    """A queue of at most one tile is grouped by one block in one launch; MK_GROUP_ONE_TILE=0 sends it through
    the kernels of the larger queues, which must agree at those totals too."""
    import torch

    monkeypatch.setenv("MK_GROUP_ONE_TILE", "0")
    rng = np.random.default_rng(11)
    for n in (1, 257, 600, (1 << 32) - 1):
        for total in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, TILE - 1, TILE):
            for pattern in PATTERNS:
                _check_group(torch, _ids(pattern, n, total, rng), n, f"tiled: n {n} total {total} {pattern}")


@pytest.mark.gpu
def test_grouping_of_nothing(gpu):
    import torch

    off, m = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    mk.network.group_requests_device(600, None, 0, None, None, off.data_ptr(), m.data_ptr(), None, 0,
                                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert off.item() == 0 and m.item() == 0
    ids = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = ids.data_ptr()
    assert N.lib().mk_requests_group_device(0, 600, p, 8, p, p, p, p, p, 16, None) == N.MK_EINVAL  # scratch too small
    assert N.lib().mk_requests_group_device(0, 600, p, 8, None, p, p, p, p, 1 << 20, None) == N.MK_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("n", [600, 70001])
def test_grouping_of_a_million(gpu, n):
    import torch

    _check_group(torch, _ids("invalid", n, 1100003, np.random.default_rng(n)), n, f"n {n} total 1100003")


# ---- the session forms ----------------------------------------------------------------
def _pair(name, tier):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(NS, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    return g, Ref(nodes, NS, **kw), gen


def _device_queue(torch, g, ids, v, stream=None):
    """compute_queue_device on fresh device arrays; returns the result tensors (read after a synchronize)."""
    total = len(ids)
    d_ids = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32)).cuda()
    d_in = torch.from_numpy(np.ascontiguousarray(v, np.int64)).cuda()
    out, sp = (torch.full((total,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    st = torch.full((total,), 0x55, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.compute_queue_device(d_ids.data_ptr(), d_in.data_ptr(), total, out.data_ptr(), st.data_ptr(), sp.data_ptr(),
                           stream=stream)
    return (d_ids, d_in), (out, st, sp)


def _result(bufs):
    out, st, sp = bufs
    return mk.network.BatchResult(out.cpu().numpy(), st.cpu().numpy(), sp.cpu().numpy().view(np.uint32))


def _ref_queue(r, ids, v):
    """The queue on the reference through numpy's grouping: ref_ragged on the sorted requests, scattered back."""
    ids = np.asarray(ids, np.int64)
    perm = np.argsort(ids, kind="stable")
    sel, cnt = np.unique(ids, return_counts=True)
    so, ss, sp = ref_ragged(r, sel, cnt, np.asarray(v)[perm])
    out, st, steps = np.zeros_like(so), np.zeros_like(ss), np.zeros_like(sp)
    out[perm], st[perm], steps[perm] = so, ss, sp
    return out, st, steps


# ---- 2: arrival order, one request at a time ---------------------------------------------
@pytest.mark.gpu
def test_queue_equals_one_request_at_a_time(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    rng = np.random.default_rng(20)
    ids = rng.choice(rng.choice(NS, 60, replace=False), 200)  # 200 requests on at most 60 sessions
    assert np.unique(ids).size < 200 and (np.diff(ids) < 0).any()
    v = po.gen_inputs(9800, 200, **gen)
    out, st, sp = np.zeros(200, np.int32), np.zeros(200, np.uint8), np.zeros(200, np.uint32)
    for j in range(200):
        o, s, p = r.call([ids[j]], [v[j]])
        out[j], st[j], sp[j] = o[0], s[0], p[0]
    assert (_reason(st) == N.MK_ST_CALL_OPEN).sum() >= 20 and (_reason(st) == N.MK_ST_BUDGET).sum() >= 20
    assert_same(g.compute_queue(ids, v, busy_ok=True), (out, st, sp), "queue of 200")
    x = po.gen_inputs(9801, NS, **gen)
    assert_same(g.compute(x, busy_ok=True), r.call(ALL, x), "plain call")
    g.close()


# ---- 3: the main scenario -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["example", "countdown150", "random19", "stackloop7"])
def test_queue_shuffled_host_and_device(gpu, name, tier):
    import torch

    g, r, gen = _pair(name, tier)
    h, _, _ = _pair(name, tier)
    rng = np.random.default_rng(4242)
    cnt = rng.integers(0, 6, NS)
    cnt[37] = 40
    total = int(cnt.sum())
    ids = rng.permutation(np.repeat(ALL, cnt))
    assert (cnt == 0).any() and (np.diff(ids) < 0).sum() > total // 4
    v = po.gen_inputs(9001, total, **gen)
    want = _ref_queue(r, ids, v)
    rs = _reason(want[1])
    if name in ("countdown150", "random19"):
        assert (rs == N.MK_ST_CALL_OPEN).sum() >= 50, (rs == N.MK_ST_CALL_OPEN).sum()
    if name == "stackloop7":
        assert (rs == N.MK_ST_BUDGET).sum() >= 1 and (rs == N.MK_ST_STACK_OVERFLOW).sum() >= 1
    if name == "example":
        assert ((want[1] & N.MK_ST_HAS_OUTPUT) != 0).sum() == total
    assert_same(g.compute_queue(ids, v, busy_ok=True), want, f"{name} host form")
    keep, bufs = _device_queue(torch, h, ids, v)
    torch.cuda.synchronize()
    assert_same(_result(bufs), want, f"{name} device form")
    # sessions without a request kept their state, the others moved on alike
    x = po.gen_inputs(9002, NS, **gen)
    plain = r.call(ALL, x)
    assert_same(g.compute(x, busy_ok=True), plain, f"{name} plain call after the host form")
    assert_same(h.compute(x, busy_ok=True), plain, f"{name} plain call after the device form")
    assert np.array_equal(g.call_open(), r.open)
    g.close()
    h.close()


# ---- 4: equivalences ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown150", "stackloop7"])
def test_queue_equals_indexed_and_seq(gpu, name, tier):
    g, _, gen = _pair(name, tier)
    h, _, _ = _pair(name, tier)
    x = _Inputs(gen, 9900)
    sel = np.sort(np.random.default_rng(257).choice(NS, 257, replace=False))
    v = x(len(sel))
    a, b = g.compute_queue(sel, v, busy_ok=True), h.compute(v, index=sel, busy_ok=True)
    assert_same(a, (b.out, b.status, b.steps), f"{name} increasing ids once each")
    v = x(9)
    i = int(sel[100])
    a, b = g.compute_queue(np.full(9, i), v, busy_ok=True), h.compute_seq(v.reshape(9, 1), index=[i], busy_ok=True)
    assert_same(a, (b.out.reshape(-1), b.status.reshape(-1), b.steps.reshape(-1)), f"{name} nine requests on one")
    assert np.array_equal(g.snapshot().rec, h.snapshot().rec), "the two sets differ after equal launches"
    g.close()
    h.close()


# ---- 5: what the host form refuses ------------------------------------------------------------
@pytest.mark.gpu
def test_queue_host_form_refusals(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 9950)
    a = np.arange(0, NS, 2)
    v = x(len(a))
    assert_same(g.compute(v, index=a), r.call(a, v), "call on the even sessions")
    busy, idle = np.nonzero(r.open)[0], np.nonzero(r.open == 0)[0]
    assert busy.size >= 20 and idle.size >= 20
    before = g.snapshot().rec.copy()
    lib = N.lib()
    buf = np.ones(16, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)
    for bad in ([1, NS, 2], [NS + 1024], [3, 0xffffffff]):
        ids = np.array(bad, np.uint32)
        assert lib.mk_session_compute_queue(g._h, ids.ctypes.data_as(C.c_void_p), bp, len(bad), bp, bp, bp) == N.MK_EINVAL
        with pytest.raises(ValueError):
            g.compute_queue(bad, [0] * len(bad))
    assert np.array_equal(g.snapshot().rec, before), "a refused queue changed a session"
    # a first request on a session with a call open: MK_EBUSY, its input not taken; one that only follows a
    # call this queue itself left open does not raise
    zero = np.zeros(4, np.int64)  # countdown from 0 closes within the slice
    ids = np.array([idle[0], busy[0], idle[0]])
    with pytest.raises(N.MkError) as e:
        g.compute_queue(ids, zero[:3])
    assert e.value.code == N.MK_EBUSY
    r.call([idle[0]], zero[:1])
    r.call([idle[0]], zero[:1])
    ids, big = np.array([idle[1], idle[1], idle[2]]), np.array([1023, 0, 0])
    want = _ref_queue(r, ids, big)
    assert want[1].tolist()[:2] == [N.MK_ST_BUDGET, N.MK_ST_CALL_OPEN]
    assert_same(g.compute_queue(ids, big), want, "a call left open by the queue itself")
    assert np.array_equal(g.call_open(), r.open)
    # the refused inputs were never taken: a resume of everything agrees with a reference that never saw them
    assert_same(g.resume(), r.call(ALL, None), "resume of everything")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), "plain call")
    g.close()


# ---- 6: the device form's net ---------------------------------------------------------------------
@pytest.mark.gpu
def test_queue_device_form_drops_ids_that_name_no_session(gpu, tier):
    import torch

    g, r, gen = _pair("countdown150", tier)
    rng = np.random.default_rng(60)
    total = 300
    ids = rng.integers(0, NS, total).astype(np.uint64)
    bad = np.zeros(total, bool)
    bad[rng.choice(total, 40, replace=False)] = True
    # none names a session, though the low bits of most do: 5 + 2^10, 7 + 2^16, 11 + 2^31 ...
    pool = np.array([NS, NS + 1, 5 + (1 << 10), 7 + (1 << 16), 11 + (1 << 31), 599 + (1 << 12), 0xffffffff, 1 << 31],
                    np.uint64)
    ids[bad] = pool[np.arange(40) % pool.size]
    ids = ids.astype(np.uint32)
    v = po.gen_inputs(9960, total, **gen)
    want = [np.zeros(total, np.int32), np.zeros(total, np.uint8), np.zeros(total, np.uint32)]
    good = np.nonzero(~bad)[0]
    for w, a in zip(want, _ref_queue(r, ids[good], v[good])):
        w[good] = a
    keep, bufs = _device_queue(torch, g, ids, v)
    torch.cuda.synchronize()
    assert_same(_result(bufs), want, "device form with ids that name no session")
    x = po.gen_inputs(9961, NS, **gen)
    assert_same(g.compute(x, busy_ok=True), r.call(ALL, x), "plain call")
    assert np.array_equal(g.call_open(), r.open)
    g.close()


# ---- 7: the scratch grows, and queues order against other launches ------------------------------------
@pytest.mark.gpu
def test_queue_scratch_growth_and_stream_order(gpu, tier):
    import torch

    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 9970)
    rng = np.random.default_rng(70)
    for total in (10, 5000, 10):
        ids = rng.integers(0, NS, total)
        v = x(total)
        assert_same(g.compute_queue(ids, v, busy_ok=True), _ref_queue(r, ids, v), f"queue of {total}")
    g.cancel()
    r.cancel(ALL)
    # a queue on one caller stream, a plain call on another: the second follows the first
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ids = rng.integers(0, NS, 8000)  # grows the scratch once more, under the device form
    v = x(8000)
    want = _ref_queue(r, ids, v)
    y = x(NS)
    d_y = torch.from_numpy(y).cuda()
    out, sp = (torch.empty(NS, dtype=torch.int32, device="cuda") for _ in range(2))
    st = torch.empty(NS, dtype=torch.uint8, device="cuda")
    keep, bufs = _device_queue(torch, g, ids, v, stream=s1.cuda_stream)
    g.compute_device(d_y.data_ptr(), out.data_ptr(), st.data_ptr(), sp.data_ptr(), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert_same(_result(bufs), want, "queue on a caller stream")
    assert_same(_result((out, st, sp)), r.call(ALL, y), "plain call on another stream")
    assert np.array_equal(g.call_open(), r.open)
    g.close()
