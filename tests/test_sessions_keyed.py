"""The directory of a session set from 64-bit client keys to instances
(mk_session_dir_*, mk_session_bind / lookup / release and their device forms,
mk_session_compute_queue_keyed, mk_session_serve_keyed; SessionSet.directory()).

The specification is `Model` below, the contract of include/mk.h written down
as a dict and a deque: bound keys give their instance, new keys take the free
instances in the order of their first occurrence, the rest are rejected, and a
release puts the released instances to the back in increasing order.  Every id
and count is compared for equality.  The answers of keyed queues are those of
test_sessions_serve's reference on the model's ids.

n = 600 is test_sessions_indexed's NS; the totals are the boundaries
test_sessions_queue uses for the scan and tile paths."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po  # noqa: F401
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)
from test_sessions_serve import SEED1, _queue, _stack_queue, ref_serve

NONE = mk.KEY_NONE
NOID = 0xFFFFFFFF
KEYED = ["mk_session_dir_open", "mk_session_dir_close", "mk_session_dir_info_get", "mk_session_dir_export",
         "mk_session_dir_import", "mk_session_bind", "mk_session_bind_device", "mk_session_lookup",
         "mk_session_lookup_device", "mk_session_release", "mk_session_release_device",
         "mk_session_compute_queue_keyed", "mk_session_serve_keyed", "mk_session_reset_indexed_device",
         "mk_session_dir_slots", "mk_session_dir_home"]


# ---- the specification ------------------------------------------------------
class Model:
    def __init__(self, n):
        self.n, self.map, self.fifo = n, {}, collections.deque(range(n))

    def bind(self, keys, admit=True):
        ids = np.full(len(keys), NOID, np.uint32)
        rejected, adm, rejreq = set(), 0, 0
        for j, k in enumerate(int(k) for k in keys):
            if k == NONE:
                continue
            if k in self.map:
                ids[j] = self.map[k]
            elif not admit:
                continue
            elif k not in rejected and self.fifo:
                ids[j] = self.map[k] = self.fifo.popleft()
                adm += 1
            else:
                rejected.add(k)
                rejreq += 1
        return ids, (adm, len(rejected), rejreq)

    def lookup(self, keys):
        return self.bind(keys, admit=False)[0]

    def release(self, keys):
        gone = sorted({self.map.pop(int(k)) for k in keys if int(k) in self.map})
        self.fifo.extend(gone)
        return gone

    def export(self):
        owner = np.full(self.n, NONE, np.uint64)
        for k, i in self.map.items():
            owner[i] = k
        return owner

    def load(self, owner):
        bound = [int(k) for k in owner if int(k) != NONE]
        if len(set(bound)) != len(bound):
            raise ValueError("a key occurs twice")
        self.map = {int(k): i for i, k in enumerate(owner) if int(k) != NONE}
        self.fifo = collections.deque(i for i, k in enumerate(owner) if int(k) == NONE)


def spread(x):
    """splitmix64's finaliser on x + 1: an injective map of the instance numbers to keys."""
    z = (np.asarray(x).astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


# ---- CPU ----------------------------------------------------------------------
def test_keyed_symbols_resolve_and_refuse_null_and_plain_sets():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in KEYED:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    buf = np.zeros(8, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)
    a, b = C.c_size_t(), C.c_size_t()
    info = N.mk_session_dir_info()
    assert lib.mk_session_dir_open(None) == N.MK_EINVAL
    assert lib.mk_session_dir_close(None) == N.MK_EINVAL
    assert lib.mk_session_dir_info_get(None, C.byref(info)) == N.MK_EINVAL
    assert lib.mk_session_dir_export(None, bp) == N.MK_EINVAL
    assert lib.mk_session_dir_import(None, bp) == N.MK_EINVAL
    assert lib.mk_session_bind(None, bp, 1, bp, None) == N.MK_EINVAL
    assert lib.mk_session_bind_device(None, bp, 1, bp, None, None) == N.MK_EINVAL
    assert lib.mk_session_lookup(None, bp, 1, bp) == N.MK_EINVAL
    assert lib.mk_session_lookup_device(None, bp, 1, bp, None) == N.MK_EINVAL
    assert lib.mk_session_release(None, bp, 1, C.byref(a)) == N.MK_EINVAL
    assert lib.mk_session_release_device(None, bp, 1, None, None) == N.MK_EINVAL
    assert lib.mk_session_compute_queue_keyed(None, bp, bp, 1, bp, bp, bp, bp, None) == N.MK_EINVAL
    assert lib.mk_session_serve_keyed(None, bp, bp, 1, 4, bp, bp, bp, bp, None, C.byref(a), C.byref(b)) == N.MK_EINVAL
    assert lib.mk_session_reset_indexed_device(None, bp, 1, None) == N.MK_EINVAL


def test_dir_slots_is_a_power_of_two_of_at_least_2n():
    for n in (1, 2, 3, 600, 70001, (1 << 24) + 1):
        s = mk.directory_slots(n)
        assert s >= 2 * n and s & (s - 1) == 0, (n, s)
    out = C.c_uint32()
    assert N.lib().mk_session_dir_slots(0, C.byref(out)) == N.MK_EINVAL
    assert N.lib().mk_session_dir_slots(5, None) == N.MK_EINVAL


@pytest.mark.parametrize("n", [NS, 70001])
def test_dir_home_is_stable_in_range_and_spreads(n):
    slots = mk.directory_slots(n)
    count = 4096
    # distinct slots a uniform draw of `count` hits on average: slots * (1 - (1 - 1/slots)^count)
    uniform = slots * (1.0 - (1.0 - 1.0 / slots) ** count)
    base = 0x123456789
    runs = {"consecutive": np.arange(base, base + count, dtype=np.uint64),
            "high word only": (np.arange(count, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xABCDEF)}
    for what, keys in runs.items():
        home = mk.directory_home(keys, slots)
        assert home.max() < slots, what
        assert np.array_equal(home, mk.directory_home(keys, slots)), what
        distinct = np.unique(home).size
        print(f"n {n} slots {slots} {what}: {distinct} distinct homes, uniform {uniform:.0f}")
        assert distinct > uniform / 2, (what, distinct, uniform)
    for bad in (0, 3, 1000):
        h = np.zeros(1, np.uint32)
        k = np.zeros(1, np.uint64)
        assert N.lib().mk_session_dir_home(k.ctypes.data_as(C.c_void_p), 1, bad,
                                           h.ctypes.data_as(C.c_void_p)) == N.MK_EINVAL


def test_key_errors_name_the_first_offending_position():
    check = mk.SessionDirectory._keys
    k = check([0, 5, (1 << 64) - 1, np.uint64(7)])
    assert k.dtype == np.uint64 and k.tolist() == [0, 5, (1 << 64) - 1, 7]
    assert check(np.array([3, 4], np.int32)).dtype == np.uint64 and check([]).size == 0
    for bad, pos in (([1, 2.0, 3], 1),            # a float
                     ([1, 2, 3, -4], 3),          # a negative
                     ([1 << 64, 2], 0),           # past 64 bits
                     ([1, 2, True], 2),           # a bool
                     ([1, "7"], 1),               # not a number
                     (np.array([1, 2, -3]), 2),   # a negative in an array
                     (np.array([1, 2, "x", 4], dtype=object), 2),  # an object array: its first bad element
                     (np.array([1.0, 2.0]), 0)):  # an array of floats
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            check(bad)
    with pytest.raises(ValueError, match=r"position 2\b"):
        check([1, 2, 3], [5, 6])
    with pytest.raises(ValueError, match=r"position 1\b"):
        check([1], [5, 6])
    kk, vv = check([9, 8], [1, 2])
    assert kk.dtype == np.uint64 and vv.dtype == np.int64
    # no handle: anything that reached the library would be an AttributeError
    d = mk.SessionDirectory.__new__(mk.SessionDirectory)
    for call in (lambda: d.bind([1, -1]), lambda: d.lookup([1, -1]), lambda: d.release([1, -1]),
                 lambda: d.compute_queue([1, -1], [0, 0]), lambda: d.serve([1, -1], [0, 0])):
        with pytest.raises(ValueError, match=r"position 1\b"):
            call()
    with pytest.raises(ValueError, match="max_slices"):
        d.serve([1], [1], max_slices=0)


def test_model_on_a_hand_written_scenario():
    m = Model(4)
    # first occurrence orders the admissions; a repeat gets its key's instance; no key is counted nowhere
    ids, counts = m.bind([50, 10, 50, NONE, 30, 10])
    assert ids.tolist() == [0, 1, 0, NOID, 2, 1] and counts == (3, 0, 0)
    # one instance left: 70 takes it, 80 and 90 are rejected with all their requests, 10 is a hit
    ids, counts = m.bind([70, 80, 10, 90, 80, 70])
    assert ids.tolist() == [3, NOID, 1, NOID, NOID, 3] and counts == (1, 2, 3)
    assert m.lookup([80, 70, NONE, 10]).tolist() == [NOID, 3, NOID, 1]
    assert m.export().tolist() == [50, 10, 30, 70]
    # release: unbound keys, no key and repeats are ignored; increasing instance order to the back
    assert m.release([70, 99, 50, NONE, 70]) == [0, 3]
    assert m.release([70]) == [] and list(m.fifo) == [0, 3]
    assert m.release([30]) == [2] and list(m.fifo) == [0, 3, 2]
    ids, counts = m.bind([80, 90, 80])
    assert ids.tolist() == [0, 3, 0] and counts == (2, 0, 0) and list(m.fifo) == [2]
    # import: the FIFO is the free instances in increasing order
    m.load(np.array([NONE, 7, NONE, NONE], np.uint64))
    assert list(m.fifo) == [0, 2, 3] and m.lookup([7, 80]).tolist() == [1, NOID]
    with pytest.raises(ValueError):
        m.load(np.array([5, NONE, 5, 1], np.uint64))
    assert list(m.fifo) == [0, 2, 3] and m.map == {7: 1}


# ---- GPU ----------------------------------------------------------------------
def _set(name="example", n=NS, tier=None):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(n, **kw)
    if tier:
        assert g.plan().startswith("tier=" + tier), g.plan()
    return g, nodes, kw, gen


def _agrees(d, m, seen, ctx):
    """lookup of every key ever seen, export and info against the model."""
    keys = np.fromiter(seen, np.uint64, len(seen))
    assert np.array_equal(d.lookup(keys), m.lookup(keys)), ctx
    assert np.array_equal(d.export(), m.export()), ctx
    i = d.info()
    assert (i.live, i.free) == (len(m.map), len(m.fifo)), (ctx, i.live, i.free, len(m.map), len(m.fifo))
    assert i.tombstones <= i.slots and i.slots == mk.directory_slots(m.n), ctx


def _bind(d, m, keys, seen, ctx):
    ids, counts = d.bind(keys)
    want, wcounts = m.bind(keys)
    seen.update(int(k) for k in keys if int(k) != NONE)
    assert counts == wcounts, (ctx, counts, wcounts)
    bad = np.flatnonzero(ids != want)
    assert bad.size == 0, (ctx, bad[:5], ids[bad[:5]], want[bad[:5]])
    return ids


TOTALS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 16385, 65537)


def _patterns(rng, total, n):
    """name -> the queues bound in a row on a fresh directory."""
    distinct = rng.permutation(np.arange(1, total + 1, dtype=np.uint64) * np.uint64(0x10001))
    some = rng.integers(0, 1 << 63, 16).astype(np.uint64)
    holes = rng.integers(0, max(total // 3, 1), total).astype(np.uint64)
    holes[rng.random(total) < 0.1] = np.uint64(NONE)
    # all but total // 2 instances taken, then `total` new keys: the FIFO runs out part way
    filler = np.arange(max(n - total // 2, 0), dtype=np.uint64) + np.uint64(1 << 40)
    many = rng.permutation(np.arange(total, dtype=np.uint64)) * np.uint64(7919) + np.uint64(3)
    many[rng.integers(0, total, total // 8)] = many[0]  # and some repeats among them
    first = rng.integers(0, max(n // 2, 1), total).astype(np.uint64)
    second = rng.integers(0, n, total).astype(np.uint64)  # hits on the first queue's keys and new ones
    return {
        "all distinct": [distinct],
        "one key": [np.full(total, 0xDEADBEEF, np.uint64)],
        "16 keys": [some[rng.integers(0, 16, total)]],
        "high word": [(rng.integers(0, max(total // 2, 1), total).astype(np.uint64) << np.uint64(32)) | np.uint64(5)],
        "a tenth no key": [holes],
        "more keys than instances": [filler, many],
        "two binds": [first, second],
    }


# ---- 1: bind and lookup against the model -------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, NS, 70001])
def test_bind_and_lookup_equal_the_model(gpu, n):
    g, *_ = _set(n=n)
    rng = np.random.default_rng(31000 + n)
    cases = rejected = 0
    for total in TOTALS:
        for what, queues in _patterns(rng, total, n).items():
            d, m, seen = g.directory(), Model(n), set()
            for q, keys in enumerate(queues):
                _bind(d, m, keys, seen, f"n {n}, {total} requests, {what}, queue {q}")
            _agrees(d, m, seen, f"n {n}, {total} requests, {what}")
            cases += 1
            rejected += len(seen) > len(m.map)
            d.close()
    print(f"n {n}: {cases} cases, {rejected} of them with keys rejected")
    assert cases == 7 * len(TOTALS) and rejected >= len(TOTALS)
    g.close()


# ---- 2: collisions and wrap-around --------------------------------------------
def _keys_at_the_end(count, seed, slots, last=4):
    """`count` distinct random keys whose probe starts in the table's last `last` slots."""
    rng = np.random.default_rng(seed)
    got = np.zeros(0, np.uint64)
    while got.size < count:
        k = rng.integers(0, 1 << 63, 1 << 18).astype(np.uint64)
        got = np.unique(np.concatenate([got, k[mk.directory_home(k, slots) >= slots - last]]))
    return rng.permutation(got)[:count]


@pytest.mark.gpu
def test_colliding_keys_wrap_around_the_table(gpu):
    slots = mk.directory_slots(NS)
    keys = _keys_at_the_end(450, 32000, slots)
    assert np.unique(keys).size == 450 and (mk.directory_home(keys, slots) >= slots - 4).all()
    a, b = keys[:300], keys[300:]
    g, *_ = _set()
    d, m, seen = g.directory(), Model(NS), set()
    _bind(d, m, a, seen, "300 colliding keys")
    assert d.release(a[::2]) == len(m.release(a[::2])) == 150
    assert np.array_equal(d.lookup(a), m.lookup(a))
    _agrees(d, m, seen, "after releasing every second one")
    _bind(d, m, np.concatenate([b, a[:40]]), seen, "150 more with the same homes, and 40 of the first")
    _agrees(d, m, seen, "after the second bind")
    g.close()


# ---- 3: churn -------------------------------------------------------------------
@pytest.mark.gpu
def test_churn_of_fifty_tables_worth_of_admissions(gpu):
    n, rounds = 64, 150
    g, *_ = _set(n=n)
    d, m, seen = g.directory(), Model(n), set()
    rng = np.random.default_rng(33000)
    fresh = iter(range(1, 1 << 30))
    admitted = 0
    for r in range(rounds):
        bound = np.array(sorted(m.map), np.uint64)
        if bound.size:
            gone = rng.choice(bound, min(48, bound.size), replace=False)
            assert d.release(gone) == len(m.release(gone)), r
        new = spread(np.array([next(fresh) for _ in range(64)]))
        keys = new[rng.integers(0, 64, 96)]
        ids, counts = d.bind(keys)
        want, wcounts = m.bind(keys)
        assert np.array_equal(ids, want) and counts == wcounts, (r, counts, wcounts)
        admitted += counts[0]
        i = d.info()
        assert (i.live, i.free) == (len(m.map), len(m.fifo)) and i.tombstones <= i.slots, r
        assert d.lookup([0x5EED0000 + r])[0] == NOID, r
    assert admitted >= 7000 > 50 * d.info().slots, admitted
    assert np.array_equal(d.export(), m.export())
    g.close()


# ---- 4: keyed queue and serve against the oracle ------------------------------
def _keyed_queue(name):
    nodes, kw, gen = NETS[name]()
    ids, v = _queue(SEED1, 3000, gen)
    if name == "stackloop7":
        ids, v = _stack_queue(ids, v)
    return nodes, kw, spread(ids), v


@functools.lru_cache(maxsize=None)
def _wanted(name, form):
    """The model's ids of the queue and the oracle's answers on them (shared by both tiers)."""
    nodes, kw, keys, v = _keyed_queue(name)
    ids, counts = Model(NS).bind(keys)
    r = Ref(nodes, NS, **kw)
    if form == "serve":
        want, left, rounds = ref_serve(r, ids, v, 32)
    else:
        cols = [r.call([int(i)], [x]) for i, x in zip(ids, v)]
        want = tuple(np.array([c[k][0] for c in cols]) for k in range(3))
        left = rounds = None
    return ids, counts, want, left, rounds


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["queue", "serve"])
@pytest.mark.parametrize("name", ["example", "countdown150", "stackloop7"])
def test_keyed_queue_and_serve_equal_the_oracle_on_the_models_ids(gpu, name, form, tier):
    ids, counts, want, left, rounds = _wanted(name, form)
    _, _, keys, v = _keyed_queue(name)
    g, *_ = _set(name, tier=tier)
    d = g.directory()
    if form == "serve":
        got = d.serve(keys, v, max_slices=32)
        assert (got.still_open, got.rounds) == (left, rounds)
    else:
        got = d.compute_queue(keys, v)
    assert np.array_equal(got.ids, ids) and got.counts == counts == (len(set(keys.tolist())), 0, 0)
    assert_same(got, want, f"{name} keyed {form}")
    g.close()


@pytest.mark.gpu
def test_keyed_serve_with_fewer_instances_than_keys(gpu, tier):
    n, nkeys = 40, 60
    nodes, kw, gen = NETS["countdown150"]()
    ids0, v = _queue(34000, 700, gen, nkeys)
    keys = spread(ids0)
    g = mk.Network(nodes).sessions(n, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    d, m, r = g.directory(), Model(n), Ref(nodes, n, **kw)
    ids, counts = m.bind(keys)
    assert counts[0] == n and counts[1] == nkeys - n and counts[2] > 100
    got = d.serve(keys, v, max_slices=32)
    want, left, rounds = ref_serve(r, ids, v, 32)
    assert np.array_equal(got.ids, ids) and got.counts == counts
    assert_same(got, want, "the first serve")
    rej = ids == NOID
    assert rej.sum() == counts[2]
    assert not got.out[rej].any() and not got.status[rej].any() and not got.steps[rej].any()
    # 25 clients leave; the rejected requests again, in their order
    gone = keys[~rej][::9][:25]
    freed = m.release(gone)
    assert d.release(gone) == len(freed) == len(set(gone.tolist()))
    r.reset(freed)
    ids2, counts2 = m.bind(keys[rej])
    assert counts2[0] == min(len(freed), nkeys - n) > 0
    got = d.serve(keys[rej], v[rej], max_slices=32)
    want, _, _ = ref_serve(r, ids2, v[rej], 32)
    assert np.array_equal(got.ids, ids2) and got.counts == counts2
    assert_same(got, want, "the rejected requests after the release")
    assert np.array_equal(d.export(), m.export())
    g.close()


# ---- 5: a release resets ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown150", "stackloop7"])
def test_release_resets_the_instance(gpu, name, tier):
    n = 8  # as many instances as A has keys: whoever comes after A gets an instance A used
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(n, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    d, m, r = g.directory(), Model(n), Ref(nodes, n, **kw)
    x = _Inputs(gen, 35000)
    A, B = spread(np.arange(100, 108)), spread(np.arange(200, 206))

    def queue(keys, ctx):
        keys = np.concatenate([keys, keys[::-1], keys])  # three calls a key: history matters
        v = x(keys.size)
        if name == "stackloop7":
            v[::4] += 32
        got = d.compute_queue(keys, v, busy_ok=True)
        ids, counts = m.bind(keys)
        want = [r.call([int(i)], [w]) for i, w in zip(ids, v)]
        assert np.array_equal(got.ids, ids) and got.counts == counts, ctx
        assert_same(got, tuple(np.array([c[k][0] for c in want]) for k in range(3)), ctx)

    queue(A, "A's calls")
    assert r.held.any(), "no call ran out of its budget: nothing was handed to the interpreter"
    if name == "countdown150":
        assert r.open.any(), "no call left open"
    freed = m.release(A)
    assert d.release(A) == len(freed) == 8
    r.reset(freed)
    assert not g.call_open(index=freed).any()
    assert np.array_equal(g.call_open(), r.open)
    queue(B, "B on instances A left")
    assert sorted(m.lookup(B).tolist()) == freed[:6]  # B took what A had left, from the FIFO's front on
    queue(A[:2], "A again, fresh")
    assert sorted(m.lookup(A[:2]).tolist()) == freed[6:]
    # the interpreter's share of the set is counted right: a plain call on all agrees
    v = x(n)
    assert_same(g.compute(v, busy_ok=True), r.call(np.arange(n), v), "plain call on all")
    assert np.array_equal(g.call_open(), r.open)
    g.close()


# ---- 6: the device forms, nothing read back -----------------------------------
def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).cuda()


@pytest.mark.gpu
def test_device_forms_chain_without_a_read_back(gpu, tier):
    import torch

    nodes, kw, gen = NETS["countdown150"]()
    g, twin = (mk.Network(nodes).sessions(NS, **kw) for _ in range(2))
    assert g.plan().startswith("tier=" + tier), g.plan()
    d, t = g.directory(), twin.directory()
    ids0, v = _queue(36000, 3000, gen, NS + 200)  # more clients than instances
    keys = spread(ids0)
    keys[7::100] = np.uint64(NONE)
    gone = keys[3::5][:400]
    keys2 = spread(np.random.default_rng(36001).integers(0, NS + 400, 3000))
    total, rounds = 3000, 16

    d_keys, d_v, d_gone, d_keys2 = (_dev(torch, a) for a in (keys, v, gone, keys2))
    i32 = lambda count: torch.full((count,), 7, dtype=torch.int32, device="cuda")  # noqa: E731
    d_ids, d_ids2, d_cnt, d_cnt2, d_rel, d_left = i32(total), i32(total), i32(3), i32(3), i32(1), i32(2)
    d_out, d_sp, d_st = i32(total), i32(total), torch.full((total,), 7, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = s.cuda_stream
    d.bind_device(d_keys.data_ptr(), total, d_ids.data_ptr(), d_cnt.data_ptr(), stream=st)
    g.serve_device(d_ids.data_ptr(), d_v.data_ptr(), total, 32, rounds, d_out.data_ptr(), d_st.data_ptr(),
                   d_sp.data_ptr(), d_left.data_ptr(), stream=st)
    d.release_device(d_gone.data_ptr(), gone.size, d_rel.data_ptr(), stream=st)
    d.bind_device(d_keys2.data_ptr(), total, d_ids2.data_ptr(), d_cnt2.data_ptr(), stream=st)
    torch.cuda.synchronize()

    u32 = lambda x: x.cpu().numpy().view(np.uint32)  # noqa: E731
    ids, counts = t.bind(keys)
    served = t.serve(keys, v, max_slices=32)  # every key that fits is bound by now
    assert served.counts == (0, counts[1], counts[2]) and np.array_equal(served.ids, ids)
    assert np.array_equal(u32(d_ids), ids) and tuple(u32(d_cnt).tolist()) == counts
    got = mk.network.BatchResult(d_out.cpu().numpy(), d_st.cpu().numpy(), u32(d_sp))
    assert served.rounds <= rounds and u32(d_left).tolist() == [served.still_open, 0]
    assert_same(got, (served.out, served.status, served.steps), "bind_device, serve_device")
    assert int(u32(d_rel)[0]) == t.release(gone) > 0
    ids2, counts2 = t.bind(keys2)
    assert np.array_equal(u32(d_ids2), ids2) and tuple(u32(d_cnt2).tolist()) == counts2
    assert np.array_equal(d.export(), t.export())
    # both sets in the same state: one plain call on all
    w = _Inputs(gen, 36500)(NS)
    a, b = g.compute(w, busy_ok=True), twin.compute(w, busy_ok=True)
    assert_same(a, (b.out, b.status, b.steps), "plain call on both")
    g.close()
    twin.close()


@pytest.mark.gpu
def test_reset_indexed_device_then_a_plain_call(gpu, tier):
    import torch

    nodes, kw, gen = NETS["countdown150"]()
    g = mk.Network(nodes).sessions(NS, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    r = Ref(nodes, NS, **kw)
    x = _Inputs(gen, 37000)
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(np.arange(NS), v), "a call that leaves calls open")
    assert r.open.any()
    sel = np.sort(np.random.default_rng(37001).choice(NS, 257, replace=False))
    listed = np.concatenate([sel, [NS, NS + 9, NOID]]).astype(np.uint32)  # the last three touch nothing
    d_sel = _dev(torch, listed)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g.reset_device(d_sel.data_ptr(), listed.size, stream=s.cuda_stream)
    r.reset(sel)
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(np.arange(NS), v), "plain call behind the device reset")
    assert np.array_equal(g.call_open(), r.open)
    g.close()


# ---- 7: export and import -----------------------------------------------------
@pytest.mark.gpu
def test_export_snapshot_restore_import_carry_a_keyed_set(gpu):
    nodes, kw, gen = NETS["stackloop7"]()
    g, h = (mk.Network(nodes).sessions(NS, **kw) for _ in range(2))
    d = g.directory()
    ids0, v = _queue(38000, 2000, gen, 400)
    keys = spread(ids0)
    d.compute_queue(keys, v, busy_ok=True)
    d.release(keys[::7][:60])  # free instances in the middle, and a FIFO that is not increasing
    owner = d.export()
    free = np.flatnonzero(owner == np.uint64(NONE))
    assert 200 < free.size < NS and (owner != np.uint64(NONE)).sum() == d.info().live
    e = h.directory()
    h.restore(g.snapshot())
    e.load(owner)
    assert np.array_equal(e.export(), owner) and (e.info().live, e.info().free) == (NS - free.size, free.size)
    # the original's FIFO in the same order as an import leaves it: both directories from the same array
    d.load(owner)
    ids1, v1 = _queue(38001, 2500, gen, 700)  # old clients and new ones, more than fit
    k1 = spread(ids1)
    a, b = d.serve(k1, v1, max_slices=8, busy_ok=True), e.serve(k1, v1, max_slices=8, busy_ok=True)
    m = Model(NS)
    m.load(owner)
    want, counts = m.bind(k1)
    assert np.array_equal(a.ids, want) and np.array_equal(b.ids, want) and a.counts == b.counts == counts
    assert counts[1] > 0
    assert_same(a, (b.out, b.status, b.steps), "the same keyed queue on both sets")
    assert np.array_equal(d.export(), e.export())
    # a key twice: refused, nothing changes
    before = e.export()
    twice = before.copy()
    bound = np.flatnonzero(twice != np.uint64(NONE))
    twice[bound[5]] = twice[bound[300]]
    with pytest.raises(ValueError, match="twice"):
        e.load(twice)
    assert N.lib().mk_session_dir_import(h._h, twice.ctypes.data_as(C.c_void_p)) == N.MK_EINVAL
    assert np.array_equal(e.export(), before) and np.array_equal(e.lookup(k1), m.lookup(k1))
    g.close()
    h.close()


# ---- 8: refusals --------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_without_a_directory_and_after_close(gpu):
    g, nodes, kw, gen = _set()
    lib = N.lib()
    k = np.arange(4, dtype=np.uint64)
    w = np.zeros(4, np.int64)
    buf = np.zeros(16, np.int64)
    kp, wp, bp = (a.ctypes.data_as(C.c_void_p) for a in (k, w, buf))
    a, b = C.c_size_t(), C.c_size_t()
    info = N.mk_session_dir_info()

    def refused():
        assert lib.mk_session_bind(g._h, kp, 4, bp, None) == N.MK_EINVAL
        assert lib.mk_session_lookup(g._h, kp, 4, bp) == N.MK_EINVAL
        assert lib.mk_session_release(g._h, kp, 4, C.byref(a)) == N.MK_EINVAL
        assert lib.mk_session_bind_device(g._h, kp, 4, bp, None, None) == N.MK_EINVAL
        assert lib.mk_session_lookup_device(g._h, kp, 4, bp, None) == N.MK_EINVAL
        assert lib.mk_session_release_device(g._h, kp, 4, None, None) == N.MK_EINVAL
        assert lib.mk_session_compute_queue_keyed(g._h, kp, wp, 4, bp, bp, bp, bp, None) == N.MK_EINVAL
        assert lib.mk_session_serve_keyed(g._h, kp, wp, 4, 4, bp, bp, bp, bp, None, C.byref(a),
                                          C.byref(b)) == N.MK_EINVAL
        assert lib.mk_session_dir_info_get(g._h, C.byref(info)) == N.MK_EINVAL
        assert lib.mk_session_dir_export(g._h, bp) == N.MK_EINVAL
        assert lib.mk_session_dir_import(g._h, bp) == N.MK_EINVAL
        assert lib.mk_session_dir_close(g._h) == N.MK_EINVAL

    refused()
    r = Ref(nodes, NS, **kw)
    x = _Inputs(gen, 39000)
    v = x(NS)
    assert_same(g.compute(v), r.call(np.arange(NS), v), "before the directory")
    d = g.directory()  # opening resets the set
    r.reset(np.arange(NS))
    assert g.directory() is d
    assert lib.mk_session_dir_open(g._h) == N.MK_EINVAL  # a second open
    assert lib.mk_session_bind(g._h, kp, 1 << 32, bp, None) == N.MK_EINVAL
    assert lib.mk_session_release(g._h, kp, 1 << 32, C.byref(a)) == N.MK_EINVAL
    ids, counts = d.bind([])
    assert ids.size == 0 and counts == (0, 0, 0) and d.release([]) == 0 and d.lookup([]).size == 0
    got = d.compute_queue([], [])
    assert got.out.size == 0 and got.counts == (0, 0, 0)
    got = d.compute_queue([5, 9, 5], [1, 2, 3])
    assert got.ids.tolist() == [0, 1, 0]
    want = [r.call([i], [w]) for i, w in zip([0, 1, 0], [1, 2, 3])]
    assert_same(got, tuple(np.array([c[k][0] for c in want]) for k in range(3)), "a keyed queue")
    # a plain reset leaves the bindings in place
    g.reset()
    r.reset(np.arange(NS))
    assert d.lookup([9, 5, 6]).tolist() == [1, 0, NOID]
    d.close()
    with pytest.raises(ValueError, match="closed"):
        d.bind([1])
    refused()
    # the unkeyed forms as before
    ids, v = _queue(39001, 500, gen)
    want = [r.call([int(i)], [w]) for i, w in zip(ids, v)]
    assert_same(g.compute_queue(ids, v), tuple(np.array([c[k][0] for c in want]) for k in range(3)),
                "compute_queue after the close")
    v = x(NS)
    assert_same(g.compute(v), r.call(np.arange(NS), v), "a plain call after the close")
    g.close()
