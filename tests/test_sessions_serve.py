"""Request queues served to completion on the GPU (mk_session_serve,
mk_session_serve_device; SessionSet.serve / serve_device), against the CPU
oracle.

The reference is the sequence that defines a serve (include/mk.h): the requests
one at a time in arrival order, each a one-entry call on its instance and then
up to max_slices resumes while it reports MK_ST_BUDGET -- run on
test_sessions_indexed's n single-instance oracle sets.  Its round count follows
the round structure on the oracle's statuses: an instance's requests run in
round 1 up to and including its first MK_ST_BUDGET, and move to the next round
each time a drained call answered and requests are left behind it.  For the
device form the reference stops an instance at max_rounds and marks the rest
status 0 without running them.

Every GPU test ends by comparing call_open() and one plain call on all
instances with the reference: the state, not only the answers.

n = 600: two full blocks and a 24-lane last wave.  3,000 requests are two
grouping tiles; 10,840 = 4 * 2048 + 2048 + 600 requests are past the 8,192
words one block scans alone.  The lists a serve compacts have one slot per
instance with a request, so the case with 10,840 instances is the one whose
round and drain lists go through the compaction's three kernels."""
import ctypes as C

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po  # noqa: F401
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)

ALL = np.arange(NS)
SERVE = ["mk_session_serve", "mk_session_serve_device"]
BUDGET, CALL_OPEN, OVERFLOW = N.MK_ST_BUDGET, N.MK_ST_CALL_OPEN, N.MK_ST_STACK_OVERFLOW
NBIG = 4 * 2048 + 2048 + 600
SEED1 = 21000  # the queue of test 1 (and of the device form)
SEED4 = 24000  # the queue of the slice limit
ROUNDS1 = 16   # rounds that serve the countdown150 queue of test 1 to the end (it takes 13)


# ---- CPU: the ABI is there, refuses a null session; the adapter checks first ----
def test_serve_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in SERVE:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    buf = np.zeros(8, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.mk_session_serve(None, bp, bp, 1, 4, bp, bp, bp, C.byref(a), C.byref(b)) == N.MK_EINVAL
    assert lib.mk_session_serve_device(None, bp, bp, 1, 4, 2, bp, bp, bp, bp, None) == N.MK_EINVAL


def test_serve_checks_before_the_library():
    # no handle: anything that reached the library would be an AttributeError
    S = mk.network.SessionSet
    s = S.__new__(S)
    s.n = 10
    for bad in (0, -1, 1 << 32):
        with pytest.raises(ValueError, match="max_slices"):
            s.serve([1, 2], [5, 6], max_slices=bad)
        with pytest.raises(ValueError, match="max_slices"):
            s.serve_device(1, 1, 2, bad, 4, 1, 1)
    with pytest.raises(ValueError, match="max_rounds"):
        s.serve_device(1, 1, 2, 4, 0, 1, 1)
    for bad, pos in (([1, 4, 10, 2], 2), ([0, 11], 1), ([-1, 2], 0), ([3, 3, 3, -7], 3)):
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            s.serve(bad, [0] * len(bad))
    with pytest.raises(ValueError, match=r"position 2\b"):
        s.serve([1, 2, 3], [5, 6])
    with pytest.raises(ValueError, match=r"position 1\b"):
        s.serve([1], [5, 6])
    with pytest.raises(ValueError, match="total"):
        s.serve_device(1, 1, 1 << 32, 4, 4, 1, 1)


# ---- the reference ----------------------------------------------------------
def ref_serve(r, ids, v, max_slices, max_rounds=None):
    """The defining sequence on the oracle sets: ((out, status, steps),
    still_open, rounds); with max_rounds also the number of requests unserved."""
    ids = np.asarray(ids, np.int64)
    total = len(ids)
    out, st, sp = np.zeros(total, np.int32), np.zeros(total, np.uint8), np.zeros(total, np.uint32)
    rnd = {}  # the round an instance's next request runs in
    rounds = unserved = 0
    for j in range(total):
        i = int(ids[j])
        if not 0 <= i < r.n:
            continue  # names no instance: 0 / 0 / 0, not counted
        k = rnd.setdefault(i, 1)
        if max_rounds is not None and k > max_rounds:
            unserved += 1
            continue
        rounds = max(rounds, k)
        o, s, p = r.call([i], [v[j]])
        if s[0] == BUDGET:
            for _ in range(max_slices):
                o, s, p = r.call([i], None)
                if s[0] != BUDGET:
                    break
            if s[0] != BUDGET:
                rnd[i] = k + 1  # the drained call answered: what is behind it runs in the next round
        out[j], st[j], sp[j] = o[0], s[0], p[0]
    res = ((out, st, sp), int((st == BUDGET).sum()), rounds)
    return res if max_rounds is None else res + (unserved,)


def _queue(seed, total, gen, n=NS):
    """`total` requests with uniformly random ids and the net's inputs."""
    ids = np.random.default_rng(seed).integers(0, n, total)
    v = po.gen_inputs(seed, max(total, 1), **gen)[:total]
    return ids, v


def _stack_queue(ids, v):
    v = v.copy()
    v[::4] += 32  # past the budget, then past the stack's capacity: calls that end their instance
    return ids, v


def _behind_overflow(ids, st, out):
    """Requests that report MK_ST_STACK_OVERFLOW with out 0 behind their instance's first overflow."""
    ov = st == OVERFLOW
    seen, c = set(), 0
    for j in np.flatnonzero(ov):
        if ids[j] in seen:
            assert out[j] == 0
            c += 1
        seen.add(ids[j])
    return c


# ---- CPU: the chosen inputs reach what the GPU tests are about ----------------
def test_chosen_queues_meet_their_caps_on_the_oracle():
    nodes, kw, gen = NETS["countdown150"]()
    ids, v = _queue(SEED1, 3000, gen)
    (_, st, _), left, rounds = ref_serve(Ref(nodes, NS, **kw), ids, v, 32)
    assert left == 0 and rounds >= 3, (left, rounds)
    assert 8 < rounds <= ROUNDS1  # the device form reaches the end with ROUNDS1 rounds and not with 8
    ids, v = _queue(SEED4, 3000, gen)
    (_, st, _), left, _ = ref_serve(Ref(nodes, NS, **kw), ids, v, 2)
    assert left >= 50 and (st == CALL_OPEN).sum() >= 50, (left, int((st == CALL_OPEN).sum()))
    for total, n in ((64, 1), (256, 3)):
        ids, v = _queue(22000 + total, total, gen, n)
        _, left, rounds = ref_serve(Ref(nodes, NS, **kw), ids, v, 32)
        assert left == 0 and rounds >= 3, (total, left, rounds)
    nodes, kw, gen = NETS["stackloop7"]()
    ids, v = _stack_queue(*_queue(SEED1, 3000, gen))
    (out, st, _), _, _ = ref_serve(Ref(nodes, NS, **kw), ids, v, 32)
    assert _behind_overflow(ids, st, out) >= 50


def test_ref_serve_is_each_instance_alone_whatever_the_interleaving():
    nodes, kw, gen = NETS["countdown150"]()
    n, total = 40, 400
    ids, v = _queue(23000, total, gen, n)
    want, left, _ = ref_serve(Ref(nodes, n, **kw), ids, v, 32)
    assert left == 0
    # each instance's requests one after another to completion, instance after instance
    order = np.argsort(ids, kind="stable")
    alone, left, rounds = ref_serve(Ref(nodes, n, **kw), ids[order], v[order], 32)
    assert left == 0 and rounds >= 3
    for a, b in zip(want, alone):
        assert np.array_equal(a[order], b)
    # another interleaving of the same per-instance sequences
    rng = np.random.default_rng(23001)
    mix = rng.permutation(ids)  # which instance takes each position: the same multiset
    nxt = {i: iter(np.flatnonzero(ids == i)) for i in range(n)}
    src = np.array([next(nxt[int(i)]) for i in mix])  # position p serves request src[p], per instance in order
    assert not np.array_equal(src, np.arange(total)) and np.array_equal(np.sort(src), np.arange(total))
    got, left, _ = ref_serve(Ref(nodes, n, **kw), ids[src], v[src], 32)
    assert left == 0
    for a, b in zip(want, got):
        assert np.array_equal(a[src], b)


# ---- GPU --------------------------------------------------------------------
def _pair(name, tier="native", n=NS):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(n, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    return g, Ref(nodes, n, **kw), gen


def _serve(g, r, ids, v, ctx, *, max_slices=32, **kw):
    got = g.serve(ids, v, max_slices=max_slices, **kw)
    want, left, rounds = ref_serve(r, ids, v, max_slices)
    assert_same(got, want, ctx)
    assert got.still_open == left and got.rounds == rounds, (ctx, got.still_open, left, got.rounds, rounds)
    return got


def _state_agrees(g, r, x, ctx):
    assert np.array_equal(g.call_open(), r.open), ctx
    v = x(r.n)
    assert_same(g.compute(v, busy_ok=True), r.call(np.arange(r.n), v), f"{ctx}: plain call")
    assert np.array_equal(g.call_open(), r.open), ctx


def _drain(g, r, ctx):
    """Every open call finished on both sides (the drain's own defining sequence)."""
    d = g.drain(max_slices=32)
    out, st, sp = r.call(ALL, None)
    for _ in range(31):
        k = np.flatnonzero(st == BUDGET)
        if not k.size:
            break
        out[k], st[k], sp[k] = r.call(ALL[k], None)
    assert_same(d, (out, st, sp), ctx)
    assert d.still_open == 0 and not r.open.any(), ctx


# ---- 1: equals the definition -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown150", "stackloop7", "random19", "example"])
def test_serve_equals_the_definition(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    ids, v = _queue(SEED1, 3000, gen)
    if name == "stackloop7":
        ids, v = _stack_queue(ids, v)
    if name == "example":
        twin = mk.Network(NETS[name]()[0]).sessions(NS)
        want = twin.compute_queue(ids, v)
        twin.close()
    got = _serve(g, r, ids, v, f"{name} serve")
    print(f"{name} {tier}: rounds {got.rounds}, still open {got.still_open}")
    if name == "example":
        assert got.rounds == 1
        assert_same(got, (want.out, want.status, want.steps), "serve against compute_queue")
    if name == "countdown150":
        assert got.rounds >= 3 and got.still_open == 0
    if name == "stackloop7":
        assert _behind_overflow(ids, got.status, got.out) >= 50
    assert g.serve([], []).out.size == 0 and g.serve(ids[:7], v[:7], steps=False, busy_ok=True).steps is None
    ref_serve(r, ids[:7], v[:7], 16)
    _state_agrees(g, r, _Inputs(gen, SEED1 + 500), f"{name} after the serve")
    g.close()


# ---- 2: many rounds on few instances ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("total,n", [(64, 1), (256, 3)])
def test_serve_many_rounds_on_few_instances(gpu, tier, total, n):
    g, r, gen = _pair("countdown150", tier)
    ids, v = _queue(22000 + total, total, gen, n)
    ids = ids + (NS - n)  # the last instances: the list's slots are not the instance numbers
    got = _serve(g, r, ids, v, f"{total} requests on {n}")
    assert got.rounds >= 3 and got.still_open == 0
    _state_agrees(g, r, _Inputs(gen, 22500), "after the serve")
    g.close()


# ---- 3: past one block's scan -----------------------------------------------
@pytest.mark.gpu
def test_serve_requests_past_the_serial_scan(gpu):
    g, r, gen = _pair("countdown150")
    ids, v = _queue(25000, NBIG, gen)
    got = _serve(g, r, ids, v, "10,840 requests")
    assert got.rounds >= 3 and got.still_open == 0
    _state_agrees(g, r, _Inputs(gen, 25500), "after the serve")
    g.close()


@pytest.mark.gpu
def test_serve_instances_past_the_serial_scan(gpu):
    # one slot per instance with a request: more than 8,192 of them, so the round
    # list and the drain list are packed by the compaction's three kernels
    g, r, gen = _pair("countdown150", n=NBIG)
    rng = np.random.default_rng(25001)
    ids = rng.permutation(np.concatenate([rng.permutation(NBIG)[:8500], rng.integers(0, 100, 500) * 97]))
    v = po.gen_inputs(25001, len(ids), **gen)
    assert np.unique(ids).size > 8192
    got = _serve(g, r, ids, v, "10,840 instances")
    assert got.rounds >= 3 and got.still_open == 0
    _state_agrees(g, r, _Inputs(gen, 25600), "after the serve")
    g.close()


# ---- 4: the slice limit -----------------------------------------------------
@pytest.mark.gpu
def test_serve_stops_at_the_slice_limit(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    ids, v = _queue(SEED4, 3000, gen)
    got = _serve(g, r, ids, v, "two slices", max_slices=2)
    assert got.still_open >= 50 and got.still_open == int(r.open.sum())
    assert (got.status == CALL_OPEN).sum() >= 50
    # behind a call left open every request of its instance reports MK_ST_CALL_OPEN
    for i in np.flatnonzero(r.open)[:20]:
        mine = np.flatnonzero(ids == i)
        at = int(np.flatnonzero(got.status[mine] == BUDGET)[0])
        assert (got.status[mine[at + 1:]] == CALL_OPEN).all() and not got.out[mine[at + 1:]].any()
    assert np.array_equal(g.call_open(), r.open)
    _drain(g, r, "drain after the serve")
    ids, v = _queue(SEED4 + 1, 3000, gen)
    _serve(g, r, ids, v, "a second serve")
    _state_agrees(g, r, _Inputs(gen, SEED4 + 500), "after the second serve")
    g.close()


# ---- 5: calls open beforehand -----------------------------------------------
@pytest.mark.gpu
def test_serve_leaves_calls_open_beforehand_alone(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 26000)
    v = x(NS)
    v[::2] = 0  # countdown from 0: closes within the slice
    assert_same(g.compute(v), r.call(ALL, v), "the plain call")
    was_open = r.open.copy()
    held = np.flatnonzero(was_open)
    assert held.size >= 50 and held.size <= NS - 50
    with pytest.raises(N.MkError) as e:
        g.serve([held[0], held[3]], [1, 2])
    assert e.value.code == N.MK_EBUSY
    ref_serve(r, [held[0], held[3]], [1, 2], 16)
    ids = np.concatenate([np.random.default_rng(26001).permutation(NS) for _ in range(3)])
    v = x(len(ids))
    got = _serve(g, r, ids, v, "serve over all instances", busy_ok=True)
    assert (got.status[was_open[ids] == 1] == CALL_OPEN).all()
    assert not (got.status[was_open[ids] == 0] == CALL_OPEN).any() and got.still_open == 0
    assert np.array_equal(g.call_open(), was_open) and np.array_equal(r.open, was_open)
    # the serve did not resume them: their next slice is their second
    assert_same(g.resume(index=held), r.call(held, None), "resume of the calls open beforehand")
    _state_agrees(g, r, x, "after the resume")
    g.close()


# ---- 6: the device form -----------------------------------------------------
class _Dev:
    """A queue and its result arrays on the device."""

    def __init__(self, ids, v):
        import torch

        self.total = len(ids)
        self.ids = torch.from_numpy(np.asarray(ids, np.int64).astype(np.uint32).view(np.int32)).cuda()
        self.v = torch.from_numpy(np.ascontiguousarray(v, np.int64)).cuda()
        self.out = torch.full((self.total,), 7, dtype=torch.int32, device="cuda")
        self.st = torch.full((self.total,), 7, dtype=torch.uint8, device="cuda")
        self.sp = torch.full((self.total,), 7, dtype=torch.int32, device="cuda")
        self.left = torch.full((2,), 7, dtype=torch.int32, device="cuda")

    def serve(self, g, max_slices, max_rounds, stream=None):
        g.serve_device(self.ids.data_ptr(), self.v.data_ptr(), self.total, max_slices, max_rounds, self.out.data_ptr(),
                       self.st.data_ptr(), self.sp.data_ptr(), self.left.data_ptr(), stream=stream)

    def result(self):
        import torch

        torch.cuda.synchronize()
        return (mk.network.BatchResult(self.out.cpu().numpy(), self.st.cpu().numpy(),
                                       self.sp.cpu().numpy().view(np.uint32)),
                self.left.cpu().numpy().view(np.uint32).tolist())


@pytest.mark.gpu
def test_serve_device_to_the_end_on_its_own_stream(gpu, tier):
    import torch

    g, r, gen = _pair("countdown150", tier)
    ids, v = _queue(SEED1, 3000, gen)
    ids[5::50] = [0xFFFFFFFF, NS, NS + 5] * 20  # name no instance: 0 / 0 / 0, nothing touched, not counted
    d = _Dev(ids, v)
    x = _Inputs(gen, SEED1 + 700)
    w = x(NS)
    d_w = torch.from_numpy(w).cuda()
    o2 = (torch.full((NS,), 7, dtype=torch.int32, device="cuda"), torch.full((NS,), 7, dtype=torch.uint8, device="cuda"),
          torch.full((NS,), 7, dtype=torch.int32, device="cuda"))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    d.serve(g, 32, ROUNDS1, stream=s1.cuda_stream)
    # a plain call on another stream, issued right after: ordered behind the serve
    g.compute_device(d_w.data_ptr(), *(b.data_ptr() for b in o2), stream=s2.cuda_stream)
    got, left = d.result()
    want, still, rounds, unserved = ref_serve(r, ids, v, 32, ROUNDS1)
    assert 3 <= rounds < ROUNDS1 and unserved == 0 and still == 0
    assert_same(got, want, "serve_device")
    bad = ids >= NS
    assert bad.sum() == 60 and not got.out[bad].any() and not got.status[bad].any() and not got.steps[bad].any()
    assert left == [0, 0]
    plain = mk.network.BatchResult(o2[0].cpu().numpy(), o2[1].cpu().numpy(), o2[2].cpu().numpy().view(np.uint32))
    assert_same(plain, r.call(ALL, w), "the plain call behind it")
    _state_agrees(g, r, x, "after the device serve")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_rounds", [1, 8])
def test_serve_device_some_rounds_then_the_unserved_again(gpu, tier, max_rounds):
    g, r, gen = _pair("countdown150", tier)
    ids, v = _queue(SEED1, 3000, gen)
    nodes, kw, _ = NETS["countdown150"]()
    whole, _, rounds = ref_serve(Ref(nodes, NS, **kw), ids, v, 32)  # what the host form gives
    d = _Dev(ids, v)
    d.serve(g, 32, max_rounds)
    got, left = d.result()
    want, still, _, unserved = ref_serve(r, ids, v, 32, max_rounds)
    assert unserved >= 50
    assert_same(got, want, "the first serve")
    assert left == [still, unserved] and ((got.status == 0).sum() == unserved)
    out, st, sp = got.out.copy(), got.status.copy(), got.steps.copy()
    calls = 1
    while (st == 0).any():
        todo = np.flatnonzero(st == 0)  # in their original order
        d = _Dev(ids[todo], v[todo])
        d.serve(g, 32, max_rounds)
        part, left = d.result()
        assert_same(part, ref_serve(r, ids[todo], v[todo], 32, max_rounds)[0], f"serve {calls} of the unserved")
        assert left[1] == (part.status == 0).sum() < len(todo)
        out[todo], st[todo], sp[todo] = part.out, part.status, part.steps
        calls += 1
    assert calls == -(-rounds // max_rounds)
    assert_same(mk.network.BatchResult(out, st, sp), whole, "the unserved served again, against one serve")
    _state_agrees(g, r, _Inputs(gen, SEED1 + 800), "after the serves")
    g.close()


# ---- 7: refusals change nothing; the scratch grows ---------------------------
@pytest.mark.gpu
def test_serve_refusals_and_scratch_growth(gpu):
    import torch

    # a mixed deployment: the host serves the peers between slices
    net = mk.Network([("g", "program", "IN ACC\nPUSH ACC, s\nPOP s, ACC\nOUT ACC"), ("s", "remote_stack", "")])
    h = net.sessions(8)
    with pytest.raises(N.MkError) as e:
        h.serve([1, 2], [3, 4])
    assert e.value.code == N.MK_EINVAL
    t = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert N.lib().mk_session_serve_device(h._h, t.data_ptr(), t.data_ptr(), 2, 4, 4, t.data_ptr(), t.data_ptr(), None,
                                           None, None) == N.MK_EINVAL
    h.close()
    g, r, gen = _pair("stackloop7")
    x = _Inputs(gen, 27000)
    ids, v = _queue(27001, 100, gen)
    _serve(g, r, ids, v, "100 requests")
    lib = N.lib()
    q = np.array([1, NS, 2], np.uint32)
    buf = np.ones(8, np.int64)
    qp, bp = q.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    assert lib.mk_session_serve(g._h, qp, bp, 3, 4, bp, bp, bp, None, None) == N.MK_EINVAL
    assert lib.mk_session_serve(g._h, qp, bp, 1, 0, bp, bp, bp, None, None) == N.MK_EINVAL
    for bad in (0, 1 << 32):
        with pytest.raises(ValueError):
            g.serve(ids, v, max_slices=bad)
    with pytest.raises(ValueError):
        g.serve([0, NS], [1, 2])
    _state_agrees(g, r, x, "after the refusals")
    _drain(g, r, "drain of the plain call's open calls")
    for total in (20000, 100):
        ids, v = _queue(27002 + total, total, gen)
        _serve(g, r, ids, v, f"{total} requests")
    _state_agrees(g, r, x, "after the growth")
    g.close()
