"""Use stamps, idle clients and eviction on a tracked directory
(mk_session_dir_track, mk_session_dir_use_*, mk_session_idle_select,
mk_session_evict, mk_session_bind_evict and their device forms;
SessionDirectory.track / idle / evict / bind(evict=) / export_use / load_use).

The specification is `EModel` below: test_sessions_keyed's Model with the
stamps `last` and a clock, and the contract of include/mk.h (idle clients)
written down as a sort:

    age(i)   = min(clock - last[i], 2^32 - 1)
    eligible = bound, age >= max(min_idle, 1), no call open
    the k most idle = the first k eligible by (age descending, instance
                      ascending), reported in increasing instance order

Every id, key, count and exported stamp is compared for equality.  The sizes
of the selection test are the boundaries of the kernels: one tile is 2,048
instances (8 rounds of a block of 256), and 70,001 instances are 35 tiles,
the last of them partly filled."""
import ctypes as C

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)
from test_sessions_keyed import NOID, NONE, Model, _dev, spread
from test_sessions_serve import ref_serve

CAP = (1 << 32) - 1
EVICT = ["mk_session_dir_track", "mk_session_dir_use_info_get", "mk_session_dir_use_export",
         "mk_session_dir_use_import", "mk_session_idle_select", "mk_session_idle_select_device", "mk_session_evict",
         "mk_session_evict_device", "mk_session_bind_evict", "mk_session_bind_evict_device"]


# ---- the specification ------------------------------------------------------
class EModel(Model):
    def __init__(self, n):
        super().__init__(n)
        self.last, self.clock = np.zeros(n, np.uint64), 0  # the stamps (0 for a free instance)
        self._owner = None  # export(), until the bindings change

    def owner(self):
        if self._owner is None:
            self._owner = self.export()
        return self._owner

    def most_idle(self, k, min_idle=1, busy=()):
        """The k most idle instances, increasing; busy: the instances with a call open."""
        age = np.minimum(np.uint64(self.clock) - self.last, np.uint64(CAP)).astype(np.int64)
        ok = (self.owner() != np.uint64(NONE)) & (age >= max(min_idle, 1))
        ok[list(busy)] = False
        inst = np.flatnonzero(ok)
        order = np.lexsort((inst, -age[inst]))  # age descending, then instance ascending
        return sorted(inst[order[:k]].tolist())

    def idle(self, want, min_idle=1, busy=()):
        ids = np.array(self.most_idle(want, min_idle, busy), np.int64)
        return self.owner()[ids], ids.astype(np.uint32)

    def release(self, keys):
        gone = super().release(keys)
        self.last[gone] = 0
        self._owner = None
        return gone

    def evict(self, want, min_idle=1, busy=()):
        keys, ids = self.idle(want, min_idle, busy)
        assert self.release(keys) == ids.tolist()
        return keys, ids

    def bind(self, keys, admit=True, evict=None, min_idle=1, busy=()):
        keys = [int(k) for k in keys]
        if not admit:
            return super().bind(keys, admit=False)
        if len(keys):
            self.clock += 1
        # the hits are stamped before anybody is evicted: what this bind touches has age 0
        self.last[[self.map[k] for k in keys if k in self.map]] = self.clock
        ek, ei = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        if evict is not None and len(keys):
            new = len({k for k in keys if k != NONE and k not in self.map})
            need = max(0, new - len(self.fifo))
            ek, ei = self.evict(min(need, evict), min_idle, busy)
        ids, counts = super().bind(keys)
        self.last[ids[ids != NOID]] = self.clock
        self._owner = None
        return (ids, counts) if evict is None else (ids, counts + (len(ei),), ek, ei)

    def load(self, owner):
        super().load(owner)
        self._owner = None
        self.last = np.where(self.owner() != np.uint64(NONE), np.uint64(self.clock), np.uint64(0))

    def export_use(self):
        return self.last.copy(), self.clock

    def load_use(self, last, clock):
        bound = self.owner() != np.uint64(NONE)
        last = np.asarray(last, np.uint64)
        if (last[bound] > np.uint64(clock)).any():
            raise ValueError("a stamp above the clock")
        self.last, self.clock = np.where(bound, last, np.uint64(0)), clock


# ---- CPU ----------------------------------------------------------------------
def test_evict_symbols_resolve_and_refuse_null_sets():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in EVICT:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    buf = np.zeros(8, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)
    a, clock, info = C.c_size_t(), C.c_uint64(), N.mk_session_dir_use_info()
    assert lib.mk_session_dir_track(None) == N.MK_EINVAL
    assert lib.mk_session_dir_use_info_get(None, C.byref(info)) == N.MK_EINVAL
    assert lib.mk_session_dir_use_export(None, bp, C.byref(clock)) == N.MK_EINVAL
    assert lib.mk_session_dir_use_import(None, bp, 0) == N.MK_EINVAL
    assert lib.mk_session_idle_select(None, 1, 1, bp, bp, C.byref(a)) == N.MK_EINVAL
    assert lib.mk_session_idle_select_device(None, 1, 1, bp, bp, None, None) == N.MK_EINVAL
    assert lib.mk_session_evict(None, 1, 1, None, None, C.byref(a)) == N.MK_EINVAL
    assert lib.mk_session_evict_device(None, 1, 1, None, None, None, None) == N.MK_EINVAL
    assert lib.mk_session_bind_evict(None, bp, 1, bp, 1, 1, None, None, None) == N.MK_EINVAL
    assert lib.mk_session_bind_evict_device(None, bp, 1, bp, 1, 1, None, None, None, None) == N.MK_EINVAL
    assert C.sizeof(info) == 16
    # no handle: anything that reached the library would be an AttributeError
    d = mk.SessionDirectory.__new__(mk.SessionDirectory)
    for call in (lambda: d.bind([1, -1], evict=3), lambda: d.compute_queue([1, -1], [0, 0], evict=3)):
        with pytest.raises(ValueError, match=r"position 1\b"):
            call()
    for call in (lambda: d.idle(-1), lambda: d.evict(1 << 32), lambda: d.idle(1, min_idle=1 << 32),
                 lambda: d.bind([1], evict=1.5)):
        with pytest.raises(ValueError):
            call()


def test_emodel_on_a_hand_written_scenario():
    m = EModel(4)
    ids, counts = m.bind([50, 10, 50, 30])  # clock 1
    assert ids.tolist() == [0, 1, 0, 2] and counts == (3, 0, 0) and m.clock == 1
    m.bind([10])       # clock 2: instance 1
    m.bind([70, 50])   # clock 3: instance 3 admitted, instance 0 a hit
    assert m.export_use()[0].tolist() == [3, 2, 1, 3] and m.clock == 3
    assert m.lookup([10, 99]).tolist() == [1, NOID] and m.clock == 3  # a lookup ticks and stamps nothing
    m.bind([])
    assert m.clock == 3  # nor does an empty bind
    # ages 0, 1, 2, 0: age 0 is never eligible; the oldest first, reported increasing
    assert m.most_idle(4) == [1, 2] and m.most_idle(1) == [2] and m.most_idle(4, min_idle=2) == [2]
    assert m.most_idle(4, busy=[2]) == [1] and m.most_idle(0) == []
    keys, ids = m.idle(1)
    assert keys.tolist() == [30] and ids.tolist() == [2] and m.clock == 3
    # A full set, two new keys, one of them twice.  10 is touched by this very bind and stays; of the ages
    # 1, 0, 3, 1 the oldest is instance 2, and instance 0 wins the tie against 3.  The victims are reported
    # in increasing order, and in that order the new keys take them.
    ids, counts, ek, ei = m.bind([80, 10, 90, 80], evict=2)
    assert m.clock == 4 and ei.tolist() == [0, 2] and ek.tolist() == [50, 30]
    assert ids.tolist() == [0, 1, 2, 0] and counts == (2, 0, 0, 2)
    m.bind([10])  # clock 5; ages 1, 0, 1, 2
    assert m.most_idle(1) == [3] and m.most_idle(2) == [0, 3] and m.most_idle(3) == [0, 2, 3]
    ids, counts, ek, ei = m.bind([91, 92, 93], evict=2)  # need 3, at most 2: the third is rejected
    assert ei.tolist() == [0, 3] and ek.tolist() == [80, 70] and ids.tolist() == [0, 3, NOID]
    assert counts == (2, 1, 1, 2) and m.export_use()[0].tolist() == [6, 5, 4, 6]
    # ages saturate: from 2^32 - 1 on they tie, and the instance number decides
    m.load_use(np.array([0, 1 << 33, (1 << 34) - 5, (1 << 34) - CAP], np.uint64), 1 << 34)
    assert m.most_idle(2) == [0, 1] and m.most_idle(3) == [0, 1, 3] and m.most_idle(9) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        m.load_use(np.array([0, 0, 0, (1 << 34) + 1], np.uint64), 1 << 34)
    # an evict: the victim queues up behind the instances already free (none here)
    assert m.evict(1)[1].tolist() == [0] and list(m.fifo) == [0]
    # import stamps what it binds with the clock
    m.load(np.array([NONE, 5, NONE, 6], np.uint64))
    assert m.export_use()[0].tolist() == [0, m.clock, 0, m.clock] and m.most_idle(4) == []


# ---- GPU ----------------------------------------------------------------------
def _tracked(name="example", n=64, tier=None):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(n, **kw)
    if tier:
        assert g.plan().startswith("tier=" + tier), g.plan()
    d = g.directory()
    d.track()
    return g, d, nodes, kw, gen


def _same_state(d, m, ctx):
    assert np.array_equal(d.export(), m.export()), ctx
    last, clock = d.export_use()
    wlast, wclock = m.export_use()
    assert clock == wclock and np.array_equal(last, wlast), (ctx, clock, wclock, np.flatnonzero(last != wlast)[:5])
    i = d.info()
    assert (i.live, i.free) == (len(m.map), len(m.fifo)), (ctx, i.live, i.free)
    assert i.tombstones <= i.slots // 4, (ctx, i.tombstones, i.slots)
    u = d.use_info()
    assert (u.clock, u.tracking) == (wclock, 1), ctx


def _check_idle(d, m, want, min_idle, ctx, busy=()):
    keys, ids = d.idle(want, min_idle)
    wkeys, wids = m.idle(want, min_idle, busy)
    assert ids.dtype == np.uint32 and keys.dtype == np.uint64
    assert ids.size == wids.size, (ctx, ids.size, wids.size)
    bad = np.flatnonzero(ids != wids)
    assert bad.size == 0, (ctx, bad[:5], ids[bad[:5]], wids[bad[:5]])
    assert np.array_equal(keys, wkeys), ctx
    return ids


# ---- 1: the selection alone -----------------------------------------------------
CLOCK = 1 << 40


def _age_patterns(rng, n):
    return {
        "all equal": np.full(n, 5, np.uint64),
        "all distinct": (rng.permutation(n) + 1).astype(np.uint64),
        "three values": rng.choice(np.array([3, 300, 70000], np.uint64), n),
        "byte 0": rng.choice(np.array([255, 256], np.uint64), n),
        "byte 1": rng.choice(np.array([65535, 65536], np.uint64), n),
        "byte 2": rng.choice(np.array([(1 << 24) - 1, (1 << 24) + 1], np.uint64), n),
        # the last four all have age 2^32 - 1
        "byte 3": rng.choice(np.array([CAP - 1, CAP, CAP + 1, 1 << 33, CLOCK], np.uint64), n),
        "a few young": np.where(rng.random(n) < 0.2, 0, 9).astype(np.uint64),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 64, 2047, 2049, 4097, 70001])
def test_idle_select_equals_the_model(gpu, n):
    g, d, *_ = _tracked(n=n)
    m = EModel(n)
    rng = np.random.default_rng(41000 + n)
    owner = spread(np.arange(n))
    if n >= 64:  # some free instances, one of them at a tile's edge when there is one
        owner[rng.choice(n, n // 16, replace=False)] = np.uint64(NONE)
        owner[min(2048, n - 1)] = np.uint64(NONE)
    d.load(owner)
    m.load(owner)
    calls = 0
    for what, age in _age_patterns(rng, n).items():
        last = np.uint64(CLOCK) - age
        d.load_use(last, CLOCK)
        m.load_use(last, CLOCK)
        elig = len(m.most_idle(n))
        wants = {0, 1, max(elig - 1, 0), elig, elig + 1, n}
        # the threshold class cut between two rounds of a block and between two tiles: with equal ages, and
        # with older ones in front of the class
        bound = owner != np.uint64(NONE)
        capped = np.minimum(age, np.uint64(CAP))
        classes = np.unique(capped)
        for edge in (256, 2048, 4096):
            if edge < n and classes.size <= 8:
                for t in classes:
                    if t:
                        wants.add(int((bound & (capped > t)).sum() + (bound & (capped == t))[:edge].sum()))
        for want in sorted(wants):
            _check_idle(d, m, want, 1, f"n {n}, {what}, want {want}")
            calls += 1
        # min_idle that excludes everything (where an age below 2^32 - 1 allows it), and exactly one class
        some = classes if classes.size <= 8 else classes[[0, classes.size // 2, -1]]
        for mi in sorted({int(t) + 1 for t in some if t < CAP}):
            for want in (1, max(elig // 2, 1), n):
                ids = _check_idle(d, m, want, mi, f"n {n}, {what}, want {want}, min_idle {mi}")
                calls += 1
                if mi > capped[bound].max():
                    assert ids.size == 0
    _same_state(d, m, f"n {n}: a selection changes nothing")
    print(f"n {n}: {calls} selections")
    g.close()


# ---- 2: open calls are not evicted ------------------------------------------------
@pytest.mark.gpu
def test_open_calls_are_not_evicted(gpu, tier):
    n = 64
    g, d, nodes, kw, gen = _tracked("countdown150", n, tier)
    m = EModel(n)
    keys = spread(np.arange(n))
    v = _Inputs(gen, 42000)(n)
    got = d.compute_queue(keys, v, busy_ok=True)
    m.bind(keys)
    busy = np.flatnonzero(g.call_open())
    assert 0 < busy.size < n, busy.size
    assert got.counts == (n, 0, 0)
    assert d.idle(n)[1].size == 0  # everyone was seen by the latest bind
    d.bind([NONE])  # a bind that names nobody: the clock ticks
    m.bind([NONE])
    ids = _check_idle(d, m, n, 1, "with calls open", busy.tolist())
    assert ids.size == n - busy.size and not np.isin(ids, busy).any()
    ek, ei = d.evict(n)
    wk, wi = m.evict(n, 1, busy.tolist())
    assert np.array_equal(ei, wi) and np.array_equal(ek, wk) and ei.size == n - busy.size
    _same_state(d, m, "after evict(n)")
    assert np.array_equal(np.flatnonzero(d.export() != np.uint64(NONE)), busy)
    assert np.array_equal(np.flatnonzero(g.call_open()), busy)
    assert g.drain(max_slices=32).still_open == 0
    ids = _check_idle(d, m, n, 1, "after the drain")
    assert np.array_equal(ids, busy)
    g.close()


# ---- 3: a bind that makes room, against the model ---------------------------------
def _check_bind(d, m, keys, evict, min_idle, ctx, busy=()):
    got = d.bind(keys, evict=evict, min_idle=min_idle)
    want = m.bind(keys, evict=evict, min_idle=min_idle, busy=busy)
    assert got[1] == want[1], (ctx, got[1], want[1])
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (ctx, bad[:5], got[0][bad[:5]], want[0][bad[:5]])
    if evict is not None:
        assert np.array_equal(got[3], want[3]), (ctx, got[3], want[3])
        assert np.array_equal(got[2], want[2]), ctx
    _same_state(d, m, ctx)
    return got


@pytest.mark.gpu
def test_bind_evict_equals_the_model(gpu):
    n = 64
    g, d, *_ = _tracked(n=n)
    twin, t, *_ = _tracked(n=n)
    m, mt = EModel(n), EModel(n)
    old = spread(np.arange(n))
    fresh = iter(range(1000, 1 << 20))
    new = lambda count: spread(np.array([next(fresh) for _ in range(count)]))  # noqa: E731
    # fill one client per bind, so that every age is different; then some become young again
    for k in old:
        d.bind([k], evict=4)
        m.bind([k], evict=4)
    _check_bind(d, m, old[[5, 9, 33]], 4, 1, "three hits")
    for k in old:
        t.bind([k])
        mt.bind([k])
    _check_bind(t, mt, old[[5, 9, 33]], None, 1, "the twin: three hits")
    c = _check_bind(d, m, new(3), 8, 1, "need 3 below max_evict 8")[1]
    assert c == (3, 0, 0, 3)
    c = _check_bind(d, m, np.concatenate([new(8), old[40:44]]), 8, 1, "need 8 at max_evict 8, and four hits")[1]
    assert c == (8, 0, 0, 8)
    q = new(12)
    q = np.concatenate([q, q[11:], [np.uint64(NONE)]])
    c = _check_bind(d, m, q, 8, 1, "need 12 above max_evict 8: four rejected, one of them twice")[1]
    assert c == (8, 4, 5, 8)
    # the oldest client left is in the queue: its age 0 protects it, the next oldest go
    oldest = int(m.most_idle(1)[0])
    ko = m.export()[oldest]
    got = _check_bind(d, m, np.concatenate([new(2), [ko]]), 4, 1, "a queue that touches the oldest client")
    assert got[1] == (2, 0, 0, 2) and oldest not in got[3].tolist() and got[0][2] == oldest
    # need above the number eligible: only the clients silent for 30 binds may go
    m.clock += 1  # as the bind will see it
    elig = len(m.most_idle(n, 30))
    m.clock -= 1
    assert 0 < elig < 20
    c = _check_bind(d, m, new(elig + 6), 64, 30, "partial eviction and rejection together")[1]
    assert c == (elig, 6, 6, elig)
    c = _check_bind(d, m, new(70), 1 << 20, 1, "more new keys than instances, max_evict past n")[1]
    assert c[0] == c[3] and c[0] + c[1] == 70 and c[1] >= 6
    # max_evict 0 is the plain bind: the same outputs as the twin's, which never evicted
    for r in range(3):
        q = np.concatenate([new(5), old[rng_pick(r)]])
        a = d.bind(q, evict=0)
        b = m.bind(q, evict=0)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1][3] == 0 and a[2].size == a[3].size == 0
    q = np.concatenate([new(5), old[:10], [np.uint64(NONE)], new(3)])
    a, b = t.bind(q, evict=0), t.lookup(q)
    wa = mt.bind(q, evict=0)
    assert np.array_equal(a[0], wa[0]) and a[1] == wa[1] == (0, 8, 8, 0) and np.array_equal(a[0], b)
    _same_state(d, m, "after max_evict 0")
    _same_state(t, mt, "the twin after max_evict 0")
    g.close()
    twin.close()


def rng_pick(r):
    return np.random.default_rng(43000 + r).integers(0, 64, 7)


# ---- 4: churn ---------------------------------------------------------------------
@pytest.mark.gpu
def test_churn_with_eviction_equals_the_model(gpu):
    n, rounds, nkeys = 64, 150, 200
    g, d, *_ = _tracked(n=n)
    m = EModel(n)
    rng = np.random.default_rng(44000)
    pool = spread(np.arange(nkeys) + 5000)
    evicted = rejected = 0
    for r in range(rounds):
        # a skew: the low client numbers come back often, the high ones rarely
        keys = pool[(nkeys * rng.random(int(rng.integers(1, 97))) ** 3).astype(np.int64)]
        evict = int(rng.choice([0, 1, 4, 16, 64, 1000]))
        got = _check_bind(d, m, keys, evict, int(rng.choice([1, 1, 2, 5])), f"round {r}")
        evicted += got[1][3]
        rejected += got[1][1]
        if r % 25 == 24:
            ek, ei = d.evict(5, 3)
            wk, wi = m.evict(5, 3)
            assert np.array_equal(ek, wk) and np.array_equal(ei, wi), r
            _same_state(d, m, f"round {r}: evict")
    print(f"{rounds} rounds: {evicted} evicted, {rejected} keys rejected, clock {m.clock}")
    assert evicted > 4 * n and rejected > 0
    g.close()


# ---- 5: answers ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["queue", "serve"])
@pytest.mark.parametrize("name", ["countdown150", "stackloop7"])
def test_keyed_queues_that_evict_equal_the_oracle_on_the_models_ids(gpu, name, form, tier):
    n, nkeys = 24, 60
    g, d, nodes, kw, gen = _tracked(name, n, tier)
    m, r = EModel(n), Ref(nodes, n, **kw)
    rng = np.random.default_rng(45000)
    x = _Inputs(gen, 45001)
    pool = spread(np.arange(nkeys) + 100)
    evicted = back = 0
    gone = set()
    for rnd in range(8):
        keys = pool[(nkeys * rng.random(40) ** 2).astype(np.int64)]
        v = x(keys.size)
        if name == "stackloop7":
            v[::4] += 32
        busy = np.flatnonzero(r.open).tolist()
        ids, counts, ek, ei = m.bind(keys, evict=6, busy=busy)
        r.reset(ei.tolist())  # an eviction resets, before any of the queue's calls
        back += len(gone & set(keys[ids != NOID].tolist()))
        gone = (gone | set(ek.tolist())) - set(keys[ids != NOID].tolist())
        served = ids != NOID
        if form == "serve":
            got = d.serve(keys, v, max_slices=2, busy_ok=True, evict=6)
            w, left, nr = ref_serve(r, ids[served], v[served], 2)
            assert got.still_open == left
        else:
            got = d.compute_queue(keys, v, busy_ok=True, evict=6)
            cols = [r.call([int(i)], [w]) for i, w in zip(ids[served], v[served])]
            w = tuple(np.array([c[k][0] for c in cols]) for k in range(3))
        ctx = f"{name} {form} round {rnd}"
        assert np.array_equal(got.ids, ids) and got.counts == counts, (ctx, got.counts, counts)
        assert np.array_equal(got.evicted_ids, ei) and np.array_equal(got.evicted_keys, ek), ctx
        part = mk.network.BatchResult(got.out[served], got.status[served], got.steps[served])
        assert_same(part, w, ctx)
        assert not got.out[~served].any() and not got.status[~served].any() and not got.steps[~served].any()
        assert np.array_equal(g.call_open(), r.open), ctx
        evicted += counts[3]
        _same_state(d, m, ctx)
        # every second open call is abandoned, so that some instances stay busy and the others can go
        some = np.flatnonzero(r.open)[::2]
        if some.size:
            g.cancel(index=some)
            r.cancel(some.tolist())
    print(f"{name} {form}: {evicted} evicted, {back} evicted clients came back")
    assert evicted >= 10 and back >= 3
    g.close()


# ---- 6: parking a client on the host and bringing it back ---------------------------
@pytest.mark.gpu
def test_parking_round_trip(gpu, tier):
    n = 16
    g, d, nodes, kw, gen = _tracked("countdown150", n, tier)
    A, B = spread(np.arange(300, 316)), spread(np.arange(400, 406))
    client = {int(k): c for c, k in enumerate(np.concatenate([A, B]))}
    r = Ref(nodes, len(client), **kw)  # one oracle instance per client: a client that never leaves
    x = _Inputs(gen, 46000)

    def queue(keys, ctx):
        keys = np.concatenate([keys, keys[::-1], keys])  # three calls a key: history matters
        v = x(keys.size)
        got = d.serve(keys, v, max_slices=32)  # to completion: nobody is left with a call open
        assert got.counts[1] == 0, ctx
        want, left, _ = ref_serve(r, [client[int(k)] for k in keys], v, 32)
        assert got.still_open == left == 0, ctx
        assert_same(got, want, ctx)

    queue(A, "A's calls")
    queue(A[:9], "nine of A again")
    queue(A[:4], "four of A again")
    assert r.held.any(), "no call ran out of its budget: nothing was handed to the interpreter"
    keys, ids = d.idle(6)
    # the most idle are among the seven seen once, none of them with a call open
    assert ids.size == 6 and set(keys.tolist()) <= set(A[9:].tolist())
    assert not g.call_open(index=ids).any()
    snap = g.snapshot(index=ids)
    assert d.release(keys) == 6
    assert (d.lookup(keys) == NOID).all()
    queue(B, "B on the instances of the parked clients")
    assert sorted(d.lookup(B).tolist()) == ids.tolist()
    queue(A[:9], "those that stayed")
    assert d.release(B) == 6
    back, counts = d.bind(keys)
    assert counts == (6, 0, 0)
    order = np.argsort(back)
    g.restore(snap, index=back[order], take=order)
    queue(A, "all of A, six of them back from the host")
    queue(keys, "the parked clients once more")
    g.close()


# ---- 7: the device forms, nothing read back -------------------------------------------
@pytest.mark.gpu
def test_device_forms_chain_without_a_read_back(gpu, tier):
    import torch

    n, total, rounds, max_evict = 64, 300, 5, 24
    nodes, kw, gen = NETS["stackloop7"]()
    g, twin = (mk.Network(nodes).sessions(n, **kw) for _ in range(2))
    assert g.plan().startswith("tier=" + tier), g.plan()
    d, t = g.directory(), twin.directory()
    d.track()
    t.track()
    rng = np.random.default_rng(47000)
    x = _Inputs(gen, 47001)
    qs = []
    for r in range(rounds):
        keys = spread((150 * rng.random(total) ** 2).astype(np.int64) + 40 * r)
        keys[3::50] = np.uint64(NONE)
        v = x(total)
        v[::4] += 32  # past the budget, then past the stack's capacity
        qs.append((keys, v))
    i32 = lambda count: torch.full((count,), 7, dtype=torch.int32, device="cuda")  # noqa: E731
    dev = [dict(keys=_dev(torch, k), v=_dev(torch, v), ids=i32(total), cnt=i32(4), out=i32(total), sp=i32(total),
                st=torch.full((total,), 7, dtype=torch.uint8, device="cuda"), ek=_dev(torch, np.zeros(max_evict, np.uint64)),
                ei=i32(max_evict)) for k, v in qs]
    sel_k, sel_i, sel_c = _dev(torch, np.zeros(n, np.uint64)), i32(n), i32(1)
    ev_c = i32(1)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = s.cuda_stream
    for a in dev:
        d.bind_evict_device(a["keys"].data_ptr(), total, a["ids"].data_ptr(), max_evict, min_idle=2,
                            ev_keys_ptr=a["ek"].data_ptr(), ev_ids_ptr=a["ei"].data_ptr(),
                            counts_ptr=a["cnt"].data_ptr(), stream=st)
        g.compute_queue_device(a["ids"].data_ptr(), a["v"].data_ptr(), total, a["out"].data_ptr(), a["st"].data_ptr(),
                               a["sp"].data_ptr(), stream=st)
    d.idle_device(n, sel_k.data_ptr(), sel_i.data_ptr(), sel_c.data_ptr(), stream=st)
    d.evict_device(7, None, None, ev_c.data_ptr(), stream=st)
    torch.cuda.synchronize()

    u32 = lambda a: a.cpu().numpy().view(np.uint32)  # noqa: E731
    u64 = lambda a: a.cpu().numpy().view(np.uint64)  # noqa: E731
    evicted = 0
    for r, ((keys, v), a) in enumerate(zip(qs, dev)):
        want = t.compute_queue(keys, v, busy_ok=True, evict=max_evict, min_idle=2)
        c = want.counts[3]
        evicted += c
        assert tuple(u32(a["cnt"]).tolist()) == want.counts, (r, u32(a["cnt"]), want.counts)
        assert np.array_equal(u32(a["ids"]), want.ids), r
        assert np.array_equal(u32(a["ei"])[:c], want.evicted_ids) and (u32(a["ei"])[c:] == NOID).all(), r
        assert np.array_equal(u64(a["ek"])[:c], want.evicted_keys) and (u64(a["ek"])[c:] == np.uint64(NONE)).all(), r
        got = mk.network.BatchResult(a["out"].cpu().numpy(), a["st"].cpu().numpy(), u32(a["sp"]))
        assert_same(got, (want.out, want.status, want.steps), f"round {r}")
    assert evicted > 20
    wk, wi = t.idle(n)
    c = int(u32(sel_c)[0])
    assert c == wi.size > 0 and np.array_equal(u32(sel_i)[:c], wi) and np.array_equal(u64(sel_k)[:c], wk)
    assert (u32(sel_i)[c:] == NOID).all() and (u64(sel_k)[c:] == np.uint64(NONE)).all()
    assert int(u32(ev_c)[0]) == t.evict(7)[1].size > 0
    assert np.array_equal(d.export(), t.export())
    a, b = d.export_use(), t.export_use()
    assert a[1] == b[1] == rounds and np.array_equal(a[0], b[0])
    assert np.array_equal(g.call_open(), twin.call_open())
    w = x(n)
    a, b = g.compute(w, busy_ok=True), twin.compute(w, busy_ok=True)
    assert_same(a, (b.out, b.status, b.steps), "plain call on both")
    g.close()
    twin.close()


# ---- 8: an untracked directory is what it was -------------------------------------------
@pytest.mark.gpu
def test_untracked_directory_beside_a_tracked_twin(gpu):
    n, rounds = 64, 150
    g, twin = (mk.Network(mk.networks.example_network()).sessions(n) for _ in range(2))
    d, t, m = g.directory(), twin.directory(), Model(n)
    t.track()
    assert d.use_info().tracking == 0 and t.use_info().tracking == 1
    # test_sessions_keyed's churn, release by release and bind by bind
    rng = np.random.default_rng(33000)
    fresh = iter(range(1, 1 << 30))
    for r in range(rounds):
        bound = np.array(sorted(m.map), np.uint64)
        if bound.size:
            gone = rng.choice(bound, min(48, bound.size), replace=False)
            assert d.release(gone) == t.release(gone) == len(m.release(gone)), r
        new = spread(np.array([next(fresh) for _ in range(64)]))
        keys = new[rng.integers(0, 64, 96)]
        a, b, w = d.bind(keys), t.bind(keys), m.bind(keys)
        assert np.array_equal(a[0], w[0]) and np.array_equal(b[0], w[0]) and a[1] == b[1] == w[1], r
        assert np.array_equal(d.export(), t.export()), r
    assert np.array_equal(d.export(), m.export())
    assert d.use_info().clock == 0 and t.use_info().clock == rounds
    g.close()
    twin.close()


# ---- 9: refusals and degenerate sizes -----------------------------------------------------
@pytest.mark.gpu
def test_refusals_untracked_and_degenerate(gpu):
    n = 8
    g = mk.Network(mk.networks.example_network()).sessions(n)
    lib = N.lib()
    k = np.arange(4, dtype=np.uint64) + np.uint64(10)
    buf, buf2 = np.zeros(16, np.int64), np.zeros(16, np.int64)
    kp, bp, bp2 = (a.ctypes.data_as(C.c_void_p) for a in (k, buf, buf2))
    a, clock, info = C.c_size_t(), C.c_uint64(), N.mk_session_dir_use_info()

    def refused():
        assert lib.mk_session_dir_use_export(g._h, bp, C.byref(clock)) == N.MK_EINVAL
        assert lib.mk_session_dir_use_import(g._h, bp, 0) == N.MK_EINVAL
        assert lib.mk_session_idle_select(g._h, 1, 1, bp, bp2, C.byref(a)) == N.MK_EINVAL
        assert lib.mk_session_idle_select_device(g._h, 1, 1, bp, bp2, None, None) == N.MK_EINVAL
        assert lib.mk_session_evict(g._h, 1, 1, None, None, C.byref(a)) == N.MK_EINVAL
        assert lib.mk_session_evict_device(g._h, 1, 1, None, None, None, None) == N.MK_EINVAL
        assert lib.mk_session_bind_evict(g._h, kp, 4, bp, 1, 1, None, None, None) == N.MK_EINVAL
        assert lib.mk_session_bind_evict(g._h, kp, 4, bp, 0, 1, None, None, None) == N.MK_EINVAL
        assert lib.mk_session_bind_evict_device(g._h, kp, 4, bp, 1, 1, None, None, None, None) == N.MK_EINVAL

    assert lib.mk_session_dir_track(g._h) == N.MK_EINVAL  # no directory
    assert lib.mk_session_dir_use_info_get(g._h, C.byref(info)) == N.MK_EINVAL
    refused()
    d = g.directory()
    refused()  # a directory, not tracked
    assert d.bind(k)[1] == (4, 0, 0)
    d.track()
    with pytest.raises(ValueError, match="tracked already"):
        d.track()
    assert lib.mk_session_dir_track(g._h) == N.MK_EINVAL
    # what was bound when tracking began has stamp 0, and clock 0 makes nobody idle
    last, c = d.export_use()
    assert c == 0 and not last.any() and d.idle(n)[1].size == 0
    for big in (1 << 32, 1 << 40):
        assert lib.mk_session_idle_select(g._h, big, 1, bp, bp2, C.byref(a)) == N.MK_EINVAL
        assert lib.mk_session_evict(g._h, big, 1, None, None, None) == N.MK_EINVAL
        assert lib.mk_session_bind_evict(g._h, kp, 4, bp, big, 1, None, None, None) == N.MK_EINVAL
        assert lib.mk_session_bind_evict_device(g._h, kp, 4, bp, big, 1, None, None, None, None) == N.MK_EINVAL
    assert lib.mk_session_bind_evict(g._h, kp, 1 << 32, bp, 1, 1, None, None, None) == N.MK_EINVAL
    assert lib.mk_session_idle_select(g._h, 1, 1, None, bp2, C.byref(a)) == N.MK_EINVAL
    assert lib.mk_session_idle_select(g._h, 1, 1, bp, None, C.byref(a)) == N.MK_EINVAL
    assert lib.mk_session_idle_select_device(g._h, 1, 1, None, None, None, None) == N.MK_EINVAL
    assert lib.mk_session_bind_evict(g._h, None, 4, bp, 1, 1, None, None, None) == N.MK_EINVAL
    assert lib.mk_session_dir_use_export(g._h, None, C.byref(clock)) == N.MK_EINVAL
    assert lib.mk_session_dir_use_import(g._h, None, 5) == N.MK_EINVAL
    # want 0 and an empty queue are MK_OK and do nothing
    assert lib.mk_session_idle_select(g._h, 0, 1, None, None, C.byref(a)) == N.MK_OK and a.value == 0
    assert lib.mk_session_evict(g._h, 0, 1, None, None, C.byref(a)) == N.MK_OK and a.value == 0
    assert lib.mk_session_evict_device(g._h, 0, 1, None, None, None, None) == N.MK_OK
    assert lib.mk_session_bind_evict(g._h, None, 0, None, 3, 1, None, None, None) == N.MK_OK
    assert d.use_info().clock == 0
    got = d.bind([], evict=3)
    assert got[0].size == 0 and got[1] == (0, 0, 0, 0) and got[2].size == got[3].size == 0
    # the victims' lists are nullable: a bind_evict and an evict that report the count only
    m = EModel(n)
    m.bind(k)
    m.last[:] = 0  # bound before tracking began
    m.clock = 0
    for r in range(3):
        q = np.arange(3, dtype=np.uint64) + np.uint64(100 + 10 * r)
        d.bind(q)
        m.bind(q)
    q = np.arange(5, dtype=np.uint64) + np.uint64(200)
    ids = np.zeros(5, np.uint32)
    cnt = (C.c_size_t * 4)()
    assert lib.mk_session_bind_evict(g._h, q.ctypes.data_as(C.c_void_p), 5, ids.ctypes.data_as(C.c_void_p), 4, 1,
                                     None, None, cnt) == N.MK_OK
    w = m.bind(q, evict=4)
    assert np.array_equal(ids, w[0]) and tuple(cnt) == w[1] == (4, 1, 1, 4)
    assert lib.mk_session_evict(g._h, 2, 1, None, None, C.byref(a)) == N.MK_OK
    assert a.value == m.evict(2)[1].size == 2
    _same_state(d, m, "after the forms without lists")
    # a stamp above the clock: refused, nothing changes
    last, c = d.export_use()
    bad = last.copy()
    bad[np.flatnonzero(d.export() != np.uint64(NONE))[0]] = c + 1
    with pytest.raises(ValueError, match="nothing loaded"):
        d.load_use(bad, c)
    _same_state(d, m, "after the refused import")
    free = np.flatnonzero(d.export() == np.uint64(NONE))
    ok = last.copy()
    ok[free] = c + 99  # a free instance's stamp is not looked at, and exported as 0
    d.load_use(ok, c)
    _same_state(d, m, "after an import with stamps on free instances")
    # import of the directory on a tracked one: every bound instance was seen just now
    owner = d.export()
    d.load(owner)
    m.load(owner)
    _same_state(d, m, "after load")
    assert d.idle(n)[1].size == 0
    # closing the directory ends the tracking
    d.close()
    refused()
    d = g.directory()
    assert d.use_info().tracking == 0
    refused()
    g.close()
