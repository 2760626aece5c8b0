"""Session fuzz: every way to drive a SessionSet, interleaved on one set,
against the CPU oracle.  A helper module (model, generator, driver) for
tests/test_sessions_fuzz.py.

Model.  SessModel is test_sessions_indexed.Ref -- n single-instance oracle
sets -- plus each instance's history since its last reset: the calls, resumes
and cancels that changed it.  An oracle instance is a deterministic function
of that history, so a snapshot is a copy of histories and flags, and a restore
replays a history into a fresh oracle instance.  Nothing is read from the GPU's
own records.

Generator.  A pure function of (network, tier, seed): it looks at the model
before each draw and at nothing else, so the CPU tests run exactly the
sequences the GPU tests run.  Kinds come from a shuffled deck (every kind in
every sequence); when more than STEER_OPEN of the set has a call open the next
operation is a resume or a cancel of open instances, when more than STEER_DEAD
has ended it is a reset of ended ones (a matching card leaves the deck when
there is one).

Driver.  run() applies each operation to the model, to the set G under test
and to a twin set H that gets the same sequence lowered to the oldest forms:
every burst, ragged or queue launch one compute(index=) per call step, every
device form its host form.  Results are compared bit-exactly with the model
after every call; at the end G's and H's records are compared instance by
instance.  A second, smaller pair of sets P (150 instances, the other tier)
trades instances with G through snapshot + restore(index=, take=).

Device forms run on one of two caller streams with no host synchronisation
between consecutive device-form operations: inputs go up on the launch's own
stream from pinned memory, results are read at the next host-form operation.
The whole-set call_open() comparison is a synchronous host call, so on G it is
made after host-form operations and whenever results are read; on H (host
forms only) after every operation."""
import contextlib
import ctypes as C
import os
from collections import Counter

import numpy as np

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from test_gpu_parity import assert_same
from test_sessions_indexed import NS, Ref
from test_sessions_queue import _ref_queue
from test_sessions_ragged import _offsets, ref_ragged

NP = 150          # the second set
NOPS = 48
STEER_OPEN = 0.25
STEER_DEAD = 0.30
ENOUGH_PROMOTED = 100  # ... in one sequence; the deck's own promotes go on
STEER_ELIGIBLE = 0.05  # idle, interpreter-held, promotion predictable: a promote finds them before calls do
STEER_DIRTY = 0.40  # instances a cancel left where no promotion can be predicted: reset, so that others get there
RESUME, CANCEL = "r", "c"
CALL_KINDS = ("compute", "seq", "ragged", "queue", "resume")
# one sequence's deck: every kind at least twice in 48 operations
DECK = dict(compute=4, seq=4, ragged=4, queue=4, resume=4, cancel=3, reset=3, call_open=2, snapshot=3, restore=4,
            fork=2, promote=3, refuse=2, migrate=4, pcall=2)
KINDS = tuple(DECK)
# ids that name none of 600 sessions, though the low bits of most do
NO_SESSION = np.array([NS, NS + 1, 5 + (1 << 10), 7 + (1 << 16), 11 + (1 << 31), 599 + (1 << 12), 0xffffffff, 1 << 31],
                      np.uint64)


def compiles_native(nodes, stack_cap=None):
    """Whether the session compiler takes the network (the tier a default set runs on), from the CPU."""
    import schedcheck as sc

    try:
        sc.session_lane(nodes, stack_cap=stack_cap)
        return True
    except sc.NotCompiled:
        return False


@contextlib.contextmanager
def tier_env(native):
    """MK_SESSION_NATIVE as a set of the wanted tier needs it while it is created."""
    old = os.environ.get("MK_SESSION_NATIVE")
    if native:
        os.environ.pop("MK_SESSION_NATIVE", None)
    else:
        os.environ["MK_SESSION_NATIVE"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MK_SESSION_NATIVE", None)
        else:
            os.environ["MK_SESSION_NATIVE"] = old


class Case:
    """One sequence: a network, its session options and input generator, the tier G runs on, a seed."""

    def __init__(self, name, nodes, kw, gen, tier, seed, *, nops=NOPS, zero_every=0, group=None):
        self.name, self.nodes, self.kw, self.gen, self.seed, self.nops = name, nodes, dict(kw), dict(gen), seed, nops
        self.zero_every, self.group = zero_every, group or name
        assert tier in ("native", "interp", "auto")
        self._tier = tier

    @property
    def g_native(self):
        """G runs on the native tier: where the session compiler takes the network, unless told otherwise."""
        if not hasattr(self, "_can"):
            self._can = compiles_native(self.nodes, self.kw.get("stack_cap"))
        return self._can and self._tier != "interp"

    @property
    def p_native(self):
        """P runs on the other tier where the network has two."""
        return not self.g_native and self._can

    @property
    def tier(self):
        return "native" if self.g_native else "interp"

    def __repr__(self):
        return f"{self.name} tier={self.tier} seed={self.seed}"


# ---- the model -----------------------------------------------------------------------
class ModelSnap:
    def __init__(self, owner, hist, open_, held, dead, dirty):
        self.owner, self.hist, self.open, self.held, self.dead, self.dirty = owner, hist, open_, held, dead, dirty

    @property
    def m(self):
        return len(self.hist)


class SessModel(Ref):
    """Ref with histories.  ``held``: the interpreter holds the instance of a native-tier set (all False in a
    set of the interpreter's tier).  ``dirty``: a cancel hit an open call since the last reset -- the
    instances whose promotion the model cannot predict."""

    def __init__(self, nodes, n, budget=None, stack_cap=None, native=True):
        super().__init__(nodes, n, budget=budget, stack_cap=stack_cap)
        self.net, self.stack_cap, self.native = self.o[0]._net, stack_cap, native
        self.hist = [[] for _ in range(n)]
        self.dirty = np.zeros(n, bool)

    def call(self, sel, values):
        sel = np.asarray(sel, np.int64)
        was_open, was_dead = self.open[sel].copy(), self.dead[sel].copy()
        res = super().call(sel, values)
        for t, i in enumerate(sel):
            if was_dead[t]:
                continue  # an ended instance takes nothing
            if values is None:
                if was_open[t]:
                    self.hist[i].append(RESUME)
            elif res[1][t] != N.MK_ST_CALL_OPEN:  # a refused call's input is not taken
                self.hist[i].append(int(values[t]))
        if not self.native:
            self.held[sel] = False
        return res

    def cancel(self, sel):
        for i in sel:
            if self.open[i]:
                self.dirty[i] = True
                self.hist[i].append(CANCEL)
        super().cancel(sel)

    def reset(self, sel):
        super().reset(sel)
        for i in sel:
            self.hist[i] = []
            self.dirty[i] = False

    def snapshot(self, sel):
        sel = np.asarray(sel, np.int64)
        return ModelSnap(self, [tuple(self.hist[i]) for i in sel], self.open[sel].copy(), self.held[sel].copy(),
                         self.dead[sel].copy(), self.dirty[sel].copy())

    def _replay(self, hist):
        o = po.OracleSessions(self.net, 1, stack_cap=self.stack_cap)
        is_open = dead = False
        for e in hist:
            if e == CANCEL:
                o.cancel()
                is_open = False
                continue
            st = int(o.compute(None if e == RESUME else [e], budget=self.budget)[1][0])
            is_open, dead = st == N.MK_ST_BUDGET, dead or st == N.MK_ST_STACK_OVERFLOW
        return o, is_open, dead

    def restore(self, sel, snap, take=None):
        for t, i in enumerate(sel):
            c = t if take is None else int(take[t])
            self.o[i], is_open, dead = self._replay(snap.hist[c])
            assert (is_open, dead) == (bool(snap.open[c]), bool(snap.dead[c])), "the replay left other flags"
            self.hist[i] = list(snap.hist[c])
            self.open[i], self.dead[i], self.dirty[i] = snap.open[c], snap.dead[c], snap.dirty[c]
            # the record's own tier bit within a set; from another set the interpreter's, until promoted
            self.held[i] = self.native and (bool(snap.held[c]) if snap.owner is self else True)

    def fork(self, src, sel):
        self.restore(sel, self.snapshot([src]), np.zeros(len(sel), np.int64))


# ---- operations ------------------------------------------------------------------------
class Op(dict):
    """kind, where ('G' or 'P'), form ('host' or 'dev'), stream (0 or 1), sel (None: every instance through
    the plain form) and what the kind needs.  A plain dict: a literal list of them replays through run()."""

    __getattr__ = dict.get

    def __str__(self):
        def short(v):
            if isinstance(v, np.ndarray):
                a = v.reshape(-1)
                return f"<{a.size}:{','.join(str(x) for x in a[:6])}{'..' if a.size > 6 else ''}>"
            return repr(v)

        return " ".join([self["kind"]] + [f"{k}={short(v)}" for k, v in self.items() if k != "kind"])


def full(sel, n):
    return np.arange(n) if sel is None else np.asarray(sel, np.int64)


class Stats:
    def __init__(self):
        self.ops, self.dev_ops, self.visits, self.status = Counter(), Counter(), Counter(), Counter()
        self.promote_eligible = self.promote_dirty = 0
        self.land_open, self.src_open, self.src_dead = Counter(), Counter(), Counter()
        self.steered = 0

    def add(self, other):
        for k, v in vars(other).items():
            if isinstance(v, Counter):
                getattr(self, k).update(v)
            else:
                setattr(self, k, getattr(self, k) + v)
        return self

    def results(self):
        return sum(v for k, v in self.status.items() if k != "HAS_OUTPUT")

    def share(self, name):
        return self.status[name] / max(self.results(), 1)

    def line(self):
        v = self.visits
        pre = {s: min(v[(k, s)] for k in CALL_KINDS) for s in ("idle_native", "idle_interp", "open", "ended")}
        return (f"ops {sum(self.ops.values())} (device forms {sum(self.dev_ops.values())}, steered {self.steered}) "
                f"min per kind {min(self.ops[k] for k in KINDS)}; least-visited call kind per pre-state {pre}; "
                f"promote eligible {self.promote_eligible} dirty {self.promote_dirty}; landed on open calls "
                f"restore {self.land_open['restore']} fork {self.land_open['fork']}; results {self.results()}: "
                + " ".join(f"{k} {self.status[k]} ({self.share(k):.2f})" for k in
                           ("HAS_OUTPUT", "QUIESCENT", "BUDGET", "STACK_OVERFLOW", "CALL_OPEN")))


ST_NAMES = {N.MK_ST_QUIESCENT: "QUIESCENT", N.MK_ST_BUDGET: "BUDGET", N.MK_ST_STACK_OVERFLOW: "STACK_OVERFLOW",
            N.MK_ST_CALL_OPEN: "CALL_OPEN", 0: "NONE"}


class Generator:
    """Draws operations from the models' state alone."""

    def __init__(self, case, models, *, steer=True):
        self.case, self.M, self.steer = case, models, steer
        self.rng = np.random.default_rng([case.seed, 0x5E55])
        self.seed = 100000 * (case.seed + 1)
        self.nsnap = 0
        self.seen = Counter()
        self.snap_cols = []  # columns of every snapshot of G taken so far
        deck = [k for k, c in DECK.items() for _ in range(c)]
        self.deck = [deck[i] for i in self.rng.permutation(len(deck))]
        self.deck.remove("compute")
        self.deck.insert(0, "compute")  # something to look at first

    def inputs(self, count, seed=None):
        """The next inputs; with ``seed`` the inputs of that fixed place (the last calls, wherever a replay stops)."""
        if seed is None:
            self.seed += 1
        x = po.gen_inputs(self.seed if seed is None else 100000 * (self.case.seed + 1) + seed, max(count, 1),
                          **self.case.gen)[:count]
        if seed is None:
            # calls of every length: as the network's generator gives them, and cut down to 6 and to 4 bits, so
            # that some close within their slice and some after one resume (a countdown from 1023 at 150
            # steps a slice never does, and a set of them is all open calls and cancels)
            c = self.rng.random()
            if c < 0.6:
                x &= 63 if c < 0.3 else 15
            elif c < 0.9:
                x[::2] += 32 if c < 0.75 else 16  # ... and some longer by a few rounds of a loop
        if self.case.zero_every:
            x[::self.case.zero_every] = 0
        return x

    # -- selections: all, a sorted subset of any size, a run that starts mid-block, a handful
    def sel(self, n, allow_all=True):
        r, c = self.rng, self.rng.random()
        if c < 0.25:
            return None if allow_all else np.arange(n)
        if c < 0.55:
            return np.sort(r.choice(n, int(r.integers(0, n + 1)), replace=False))
        if c < 0.80:
            a = int(r.integers(1, n - 1))
            if a % 256 == 0:
                a += 1
            return np.arange(a, int(r.integers(a + 1, n + 1)))
        return np.sort(r.choice(n, int(r.integers(1, 9)), replace=False))

    def _classes(self):
        """The pre-states a call can meet, from the model (held only where dirty does not blur it)."""
        g = self.M["G"]
        is_open = g.open == 1
        idle = ~is_open & ~g.dead & ~g.dirty
        return dict(open=is_open, ended=g.dead, idle_native=idle & ~g.held, idle_interp=idle & g.held)

    def call_sel(self, kind):
        """The selection of a call: any, or -- every other time -- any and the instances in the pre-state this kind of call
        has met least in this sequence."""
        r, cl = self.rng, self._classes()
        some = [k for k, v in cl.items() if v.any()]
        if self.steer and some and r.random() < 0.5:
            idx = np.nonzero(cl[min(some, key=lambda k: self.seen[(kind, k)])])[0]
            sel = np.union1d(full(self.sel(NS), NS), idx)
        else:
            sel = self.sel(NS)
        for k, v in cl.items():
            self.seen[(kind, k)] += int(v[full(sel, NS)].sum())
        return sel

    def _among(self, idx):
        """A selection made of the given instances: all of the set, exactly them, or half of them."""
        r, c = self.rng, self.rng.random()
        if c < 0.3:
            return None
        if c < 0.7 or idx.size < 2:
            return idx
        return np.sort(r.choice(idx, idx.size // 2, replace=False))

    def _take(self, kind):
        if kind in self.deck:
            self.deck.remove(kind)

    def draw(self):
        g, r = self.M["G"], self.rng
        kind = None
        if self.steer:
            ended, opened = np.nonzero(g.dead)[0], np.nonzero(g.open)[0]
            # held is the model's own wherever dirty is not set, so this too looks at the model alone
            eligible = np.nonzero(g.held & (g.open == 0) & ~g.dirty)[0]
            if eligible.size > STEER_ELIGIBLE * g.n and self.seen["promoted"] < ENOUGH_PROMOTED and r.random() < 0.7:
                # half of them and a few others: the other half stays idle and the interpreter's for the calls
                sel = np.union1d(r.choice(eligible, eligible.size // 2, replace=False), r.choice(NS, 20, replace=False))
                self._take("promote")
                self.seen["promoted"] += eligible.size // 2
                return Op(kind="promote", sel=sel, steered=True, **self._form())
            if ended.size > STEER_DEAD * g.n and r.random() < 0.75:
                kind, sel = "reset", self._among(ended)
                if sel is None and r.random() < 0.7:
                    sel = ended
            elif opened.size > STEER_OPEN * g.n and r.random() < 0.75:
                kind, sel = ("resume" if r.random() < 0.6 else "cancel"), self._among(opened)
            elif g.dirty.sum() > STEER_DIRTY * g.n and r.random() < 0.3:
                dirty = np.nonzero(g.dirty)[0]  # half of them: the rest stay, idle and the interpreter's
                kind, sel = "reset", np.sort(r.choice(dirty, dirty.size // 2, replace=False))
            if kind:
                self._take(kind)
                return Op(kind=kind, sel=sel, steered=True)
        kind = self.deck.pop(0) if self.deck else KINDS[int(r.integers(len(KINDS)))]
        return getattr(self, "_" + kind)()

    def _form(self):
        return dict(form="dev", stream=int(self.rng.integers(2))) if self.rng.random() < 0.5 else dict(form="host")

    def _compute(self):
        sel = self.call_sel("compute")
        return Op(kind="compute", sel=sel, x=self.inputs(len(full(sel, NS))), **self._form())

    def _seq(self):
        sel, k = self.call_sel("seq"), int(self.rng.integers(2, 4))
        m = len(full(sel, NS))
        return Op(kind="seq", sel=sel, x=self.inputs(k * m).reshape(k, m), **self._form())

    def _ragged(self):
        sel, r = self.call_sel("ragged"), self.rng
        m = len(full(sel, NS))
        cnt = r.integers(0, 6, m)
        if m and r.random() < 0.5:
            cnt[int(r.integers(m))] = int(r.integers(10, 41))  # the occasional long entry
        return Op(kind="ragged", sel=sel, counts=cnt, x=self.inputs(int(cnt.sum())), **self._form())

    def _queue(self):
        r = self.rng
        pool = full(self.call_sel("queue"), NS)
        if pool.size == 0:
            pool = r.choice(NS, int(r.integers(1, NS + 1)), replace=False)
        # a few requests per instance of the pool: behind a call that stays open a burst only collects refusals
        ids = r.choice(pool, int(r.integers(1, min(1500, 4 * pool.size) + 1))).astype(np.uint64)
        form = self._form()
        if form["form"] == "dev":  # ... which drops ids that name no session
            bad = r.random(ids.size) < 0.1
            ids[bad] = r.choice(NO_SESSION, int(bad.sum()))
        return Op(kind="queue", ids=ids.astype(np.uint32), x=self.inputs(ids.size), **form)

    def _resume(self):
        return Op(kind="resume", sel=self.call_sel("resume"))

    def _cancel(self):
        return Op(kind="cancel", sel=self.sel(NS))

    def _reset(self):
        r = self.rng
        sel = self.sel(NS)
        if sel is None and r.random() < 0.5:  # a reset of everything forgets too much to be common
            sel = np.sort(r.choice(NS, int(r.integers(1, 200)), replace=False))
        return Op(kind="reset", sel=sel)

    def _call_open(self):
        return Op(kind="call_open", sel=self.sel(NS))

    def _snapshot(self):
        sel = self.sel(NS)
        form = self._form()
        self.snap_cols.append(len(full(sel, NS)))
        return Op(kind="snapshot", sel=sel, bytes=bool(form["form"] == "host" and self.rng.random() < 0.4), **form)

    def _restore(self):
        r = self.rng
        if not self.snap_cols:
            return self._snapshot()
        j = int(r.integers(len(self.snap_cols)))
        cols = self.snap_cols[j]
        if cols == 0:
            return Op(kind="restore", snap=j, sel=np.zeros(0, np.int64), take=None, **self._form())
        if r.random() < 0.35:  # without take: instance sel[t] takes column t
            sel = self._onto()
            if len(full(sel, NS)) > cols:
                sel = np.sort(r.choice(NS, int(r.integers(1, cols + 1)), replace=False))
            return Op(kind="restore", snap=j, sel=sel, take=None, **self._form())
        sel = self._onto()
        return Op(kind="restore", snap=j, sel=sel, take=r.integers(0, cols, len(full(sel, NS))), **self._form())

    def _onto(self, p=0.4):
        """Where a restore or a fork lands: any selection, or one among the instances with a call open."""
        opened = np.nonzero(self.M["G"].open)[0]
        if opened.size and self.rng.random() < p:
            sel = self._among(opened)
            return opened if sel is None else sel
        return self.sel(NS)

    def _pick(self, m):
        """An instance, often one with a call open or an ended one."""
        r, c = self.rng, self.rng.random()
        for lo, hi, idx in ((0.0, 0.4, np.nonzero(m.open)[0]), (0.4, 0.65, np.nonzero(m.dead)[0])):
            if lo <= c < hi and idx.size:
                return int(r.choice(idx))
        return int(r.integers(m.n))

    def _fork(self):
        return Op(kind="fork", src=self._pick(self.M["G"]), sel=full(self._onto(0.6), NS))

    def _promote(self):
        return Op(kind="promote", sel=None if self.rng.random() < 0.25 else self.sel(NS), **self._form())

    def _refuse(self):
        r = self.rng
        what = ("index", "take", "queue")[int(r.integers(3))]
        if what == "take" and not any(self.snap_cols):
            what = "index"
        if what == "index":
            a, b = sorted(int(x) for x in r.choice(NS, 2, replace=False))
            bad = ([b, a], [a, a], [a, NS], [a, b, NS + 7])[int(r.integers(4))]
            via = ("step", "cancel", "reset", "promote", "ragged", "snapshot")[int(r.integers(6))]
            return Op(kind="refuse", what=what, bad=np.array(bad), via=via)
        if what == "take":
            j = int(r.choice([k for k, c in enumerate(self.snap_cols) if c]))
            sel = np.sort(r.choice(NS, 3, replace=False))
            take = r.integers(0, self.snap_cols[j], 3)
            take[int(r.integers(3))] = self.snap_cols[j] + int(r.integers(0, 3))
            return Op(kind="refuse", what=what, snap=j, sel=sel, take=take)
        ids = r.integers(0, NS, 5)
        ids[int(r.integers(5))] = int(r.choice(NO_SESSION))
        return Op(kind="refuse", what=what, ids=ids.astype(np.uint32))

    def _migrate(self):
        r = self.rng
        to_p = bool(r.random() < 0.4)
        src, dst = (self.M["G"], self.M["P"]) if to_p else (self.M["P"], self.M["G"])
        k = int(r.integers(1, NP + 1))
        src_sel = np.sort(r.choice(src.n, k, replace=False))
        if r.random() < 0.5:
            src_sel[0] = self._pick(src)
            src_sel = np.unique(src_sel)
            k = src_sel.size
        kd = int(r.integers(1 if to_p else NP // 3, NP + 1))
        return Op(kind="migrate", to_p=to_p, src_sel=src_sel, sel=np.sort(r.choice(dst.n, kd, replace=False)),
                  take=r.integers(0, k, kd), bytes=bool(r.random() < 0.3))

    def _pcall(self):
        return Op(kind="pcall", x=self.inputs(NP))


# ---- the GPU side ----------------------------------------------------------------------
class _DevSnap:
    def __init__(self, layout, rec, m, keep):
        self.layout, self.rec, self.m, self.keep = layout, rec, m, keep


class Side:
    """A pair of sets (G and P) and its snapshots.  ``twin``: everything lowered to compute(index=) and host forms."""

    def __init__(self, case, net, twin):
        self.case, self.twin = case, twin
        kw = case.kw
        with tier_env(case.g_native):
            self.G = net.sessions(NS, **kw)
        with tier_env(case.p_native):
            self.P = net.sessions(NP, **kw)
        for s, native in ((self.G, case.g_native), (self.P, case.p_native)):
            assert s.plan().startswith("tier=native" if native else "tier=interp"), (str(case), s.plan())
        self.snaps, self.pending = [], []
        if not twin:
            import torch

            self.torch = torch
            self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def close(self):
        self.G.close()
        self.P.close()

    # -- device plumbing
    def up(self, a, stream):
        """A host array onto the device on the launch's own stream, from pinned memory."""
        torch = self.torch
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        h = torch.from_numpy(a).pin_memory()
        with torch.cuda.stream(stream):
            return h, h.cuda(non_blocking=True)

    def outs(self, count, stream):
        torch = self.torch
        with torch.cuda.stream(stream):
            return (torch.full((max(count, 1),), -7, dtype=torch.int32, device="cuda"),
                    torch.full((max(count, 1),), 0x55, dtype=torch.uint8, device="cuda"),
                    torch.full((max(count, 1),), -7, dtype=torch.int32, device="cuda"))

    def host_snap(self, j):
        s = self.snaps[j]
        if isinstance(s, _DevSnap):
            self.torch.cuda.synchronize()
            rec = s.rec.cpu().numpy().view(np.uint32)[:s.layout.rows * s.m].reshape(s.layout.rows, s.m).copy()
            s = mk.SessionSnapshot(s.layout, rec)
        return s


def _bufp(a):
    return a.ctypes.data_as(C.c_void_p)


class Run:
    """One sequence on the model and, with ``gpu``, on G, H and their P sets."""

    def __init__(self, case, *, gpu, steer=True):
        self.case, self.gpu = case, gpu
        kw = case.kw
        self.M = {"G": SessModel(case.nodes, NS, native=case.g_native, **kw),
                  "P": SessModel(case.nodes, NP, native=case.p_native, **kw)}
        self.gen = Generator(case, self.M, steer=steer)
        self.msnaps = []
        self.stats = Stats()
        self.log = []
        self.k = -1
        self.sides = []
        if gpu:
            net = mk.Network(case.nodes)
            self.net = net
            self.sides = [Side(case, net, False), Side(case, net, True)]

    def ctx(self, what=""):
        op = self.log[self.k] if 0 <= self.k < len(self.log) else "end"
        return f"{self.case} op {self.k} [{op}] {what}"

    # -- bookkeeping of what an operation met
    def _visit(self, kind, idx):
        m = self.M["G"]
        idx = np.asarray(idx, np.int64)
        is_open, dead = m.open[idx] == 1, m.dead[idx]
        idle = ~is_open & ~dead
        v = self.stats.visits
        v[(kind, "open")] += int(is_open.sum())
        v[(kind, "ended")] += int(dead.sum())
        if m.native:
            v[(kind, "idle_native")] += int((idle & ~m.held[idx]).sum())
            v[(kind, "idle_interp")] += int((idle & m.held[idx]).sum())
        else:
            v[(kind, "idle_interp_tier")] += int(idle.sum())

    def _count(self, st):
        st = np.asarray(st).reshape(-1)
        self.stats.status["HAS_OUTPUT"] += int(((st & N.MK_ST_HAS_OUTPUT) != 0).sum())
        for code, c in zip(*np.unique(st & N.MK_ST_REASON_MASK, return_counts=True)):
            self.stats.status[ST_NAMES.get(int(code), str(code))] += int(c)

    # -- comparisons
    def _same(self, got, want, what):
        got = mk.network.BatchResult(*(np.asarray(a).reshape(-1) for a in (got.out, got.status, got.steps)))
        assert_same(got, tuple(np.asarray(a).reshape(-1) for a in want), self.ctx(what))

    def _open_agrees(self, side, what):
        for w in ("G", "P"):
            got = getattr(side, w).call_open()
            assert np.array_equal(got, self.M[w].open), self.ctx(
                f"{what}: call_open of {w} differs at {np.nonzero(got != self.M[w].open)[0][:8]}")

    def _tier_agrees(self, held, w, what, want=None, live=None):
        m = self.M[w]
        want = ~m.held if want is None else want
        live = ~m.dead if live is None else live
        if not m.native:
            assert not held.any(), self.ctx(f"{what}: a set of the interpreter's tier reports native holds")
            return
        bad = np.nonzero((held != want) & live)[0]
        assert bad.size == 0, self.ctx(f"{what}: tier bit of {w} differs at {bad[:8]} (native holds, got "
                                       f"{held[bad[:8]]})")

    def flush(self):
        """Read what the device forms left behind, in order."""
        side = self.sides[0]
        if not side.pending:
            return
        side.torch.cuda.synchronize()
        k = self.k
        for p in side.pending:
            self.k = p["k"]
            if p["what"] == "call":
                out, st, sp = (t.cpu().numpy()[:p["count"]] for t in p["bufs"])
                self._same(mk.network.BatchResult(out, st, sp.view(np.uint32)), p["want"], "device form")
            elif p["what"] == "promote":
                self._promoted(p["flags"].cpu().numpy()[:p["count"]].astype(bool), p, "device form")
            elif p["what"] == "tier":
                held = p["rec"].cpu().numpy()[:NS] == 1
                self._tier_agrees(held, "G", "device form", want=p["want"], live=p["live"])
        side.pending = []
        self.k = k

    # -- call-type operations
    def _want(self, op):
        m, kind = self.M["G"], op.kind
        sel = full(op.sel, NS)
        if kind == "compute":
            return m.call(sel, op.x)
        if kind == "resume":
            return m.call(sel, None)
        if kind == "seq":
            rows = [m.call(sel, v) for v in op.x]
            return tuple(np.stack([r[i] for r in rows]) for i in range(3))
        if kind == "ragged":
            return ref_ragged(m, sel, op.counts, op.x)
        ids = op.ids.astype(np.int64)
        good = np.nonzero(ids < NS)[0]
        want = [np.zeros(ids.size, np.int32), np.zeros(ids.size, np.uint8), np.zeros(ids.size, np.uint32)]
        for w, a in zip(want, _ref_queue(m, ids[good], op.x[good])):
            w[good] = a
        return tuple(want)

    def _touched(self, op):
        if op.kind == "queue":
            ids = op.ids.astype(np.int64)
            return np.unique(ids[ids < NS])
        sel = full(op.sel, NS)
        return sel[np.asarray(op.counts) > 0] if op.kind == "ragged" else sel

    def _host_call(self, g, op):
        kind, sel = op.kind, op.sel
        if kind == "compute":
            return g.compute(op.x, index=sel, busy_ok=True)
        if kind == "resume":
            return g.resume(index=sel)
        if kind == "seq":
            return g.compute_seq(op.x, index=sel, busy_ok=True)
        if kind == "ragged":
            return g.compute_ragged(op.x, op.counts, index=sel, busy_ok=True)
        return g.compute_queue(op.ids, op.x, busy_ok=True)

    def _lowered_ragged(self, g, sel, cnt, v):
        """ref_ragged's order on a set: call c of every entry that has one, one compute(index=) each."""
        cnt = np.asarray(cnt, np.int64)
        off = _offsets(cnt)
        out, st, sp = np.zeros(off[-1], np.int32), np.zeros(off[-1], np.uint8), np.zeros(off[-1], np.uint32)
        for c in range(int(cnt.max()) if cnt.size else 0):
            ts = np.nonzero(cnt > c)[0]
            at = off[ts] + c
            r = g.compute(v[at], index=sel[ts], busy_ok=True)
            out[at], st[at], sp[at] = r.out, r.status, r.steps
        return mk.network.BatchResult(out, st, sp)

    def _lowered_call(self, g, op):
        kind, sel = op.kind, full(op.sel, NS)
        if kind == "compute":
            return g.compute(op.x, index=sel, busy_ok=True)
        if kind == "resume":
            return g.resume(index=sel)
        if kind == "seq":
            rows = [g.compute(v, index=sel, busy_ok=True) for v in op.x]
            return mk.network.BatchResult(*(np.stack([getattr(r, f) for r in rows]) for f in ("out", "status", "steps")))
        if kind == "ragged":
            return self._lowered_ragged(g, sel, op.counts, op.x)
        ids = op.ids.astype(np.int64)
        good = np.nonzero(ids < NS)[0]
        perm = np.argsort(ids[good], kind="stable")
        qsel, cnt = np.unique(ids[good], return_counts=True)
        r = self._lowered_ragged(g, qsel, cnt, op.x[good][perm])
        res = mk.network.BatchResult(np.zeros(ids.size, np.int32), np.zeros(ids.size, np.uint8),
                                     np.zeros(ids.size, np.uint32))
        for a, b in zip((res.out, res.status, res.steps), (r.out, r.status, r.steps)):
            a[good[perm]] = b
        return res

    def _dev_call(self, side, op, want):
        g, kind = side.G, op.kind
        s = side.streams[op.stream]
        sp = s.cuda_stream
        keep = []

        def up(a):
            h, d = side.up(a, s)
            keep.extend((h, d))
            return d.data_ptr()

        sel = None if op.sel is None else np.asarray(op.sel, np.int64).astype(np.uint32)
        ix = dict(index_ptr=up(sel), m=int(sel.size)) if sel is not None else {}
        count = int(np.asarray(want[0]).size)
        bufs = side.outs(count, s)
        o, st, stp = (b.data_ptr() for b in bufs)
        v = up(np.asarray(op.x, np.int64).reshape(-1))
        if kind == "compute":
            g.compute_device(v, o, st, stp, stream=sp, **ix)
        elif kind == "seq":
            g.compute_seq_device(v, int(op.x.shape[0]), o, st, stp, stream=sp, **ix)
        elif kind == "ragged":
            off = _offsets(np.asarray(op.counts, np.int64))
            g.compute_ragged_device(v, up(off.astype(np.uint32)), int(off[-1]), o, st, stp, stream=sp, **ix)
        else:
            g.compute_queue_device(up(op.ids), v, int(op.ids.size), o, st, stp, stream=sp)
        side.pending.append(dict(what="call", k=self.k, count=count, bufs=bufs, want=want, keep=keep))

    def _call(self, op):
        self._visit(op.kind, self._touched(op))
        want = self._want(op)
        self._count(want[1])
        if not self.gpu:
            return
        a, b = self.sides
        if op.form == "dev":
            self._dev_call(a, op, want)
        else:
            got = self._host_call(a.G, op)
            self.flush()
            self._same(got, want, "host form")
        self._same(self._lowered_call(b.G, op), want, "twin, lowered")

    # -- everything else
    def _simple(self, op):
        m, kind = self.M["G"], op.kind
        sel = full(op.sel, NS)
        if kind == "call_open":
            for side in self.sides:
                assert np.array_equal(side.G.call_open(index=op.sel), m.open[sel]), self.ctx("call_open(index=)")
            return
        getattr(m, kind)(sel)
        for side in self.sides:
            getattr(side.G, kind)(index=op.sel)

    def _snapshot(self, op):
        sel = full(op.sel, NS)
        self.msnaps.append(self.M["G"].snapshot(sel))
        for side in self.sides:
            if side.twin or op.form == "host":
                s = side.G.snapshot(index=op.sel)
                if op.bytes and not side.twin:
                    s = mk.SessionSnapshot.frombytes(s.tobytes())
                side.snaps.append(s)
                continue
            torch, st = side.torch, side.streams[op.stream]
            lay = side.G.layout()
            keep, ix = [], {}
            if op.sel is not None:
                keep = side.up(sel.astype(np.uint32), st)
                ix = dict(index_ptr=keep[1].data_ptr(), m=int(sel.size))
            with torch.cuda.stream(st):
                rec = torch.zeros(max(lay.rows * sel.size, 1), dtype=torch.int32, device="cuda")
            side.G.snapshot_device(rec.data_ptr(), stream=st.cuda_stream, **ix)
            side.snaps.append(_DevSnap(lay, rec, int(sel.size), [keep]))

    def _tier_after(self, op, what):
        """The tier bits after a promote or a restore: from a snapshot, on G through the form the operation took."""
        if not self.gpu:
            return
        m = self.M["G"]
        a, b = self.sides
        self._tier_agrees(b.G.snapshot().held, "G", f"{what} (twin)")
        if op.form != "dev":
            self._tier_agrees(a.G.snapshot().held, "G", what)
            return
        torch, st = a.torch, a.streams[1 - op.stream]  # the other stream: ordered by the set, not by the stream
        with torch.cuda.stream(st):
            rec = torch.zeros(a.G.layout().rows * NS, dtype=torch.int32, device="cuda")
        a.G.snapshot_device(rec.data_ptr(), stream=st.cuda_stream)
        a.pending.append(dict(what="tier", k=self.k, rec=rec, want=~m.held, live=~m.dead))

    def _restore(self, op):
        m = self.M["G"]
        sel = full(op.sel, NS)
        ms = self.msnaps[op.snap]
        cols = np.arange(sel.size) if op.take is None else np.asarray(op.take, np.int64)
        self.stats.land_open["restore"] += int(m.open[sel].sum())
        self.stats.src_open["restore"] += int(ms.open[cols].any()) if sel.size else 0
        self.stats.src_dead["restore"] += int(ms.dead[cols].any()) if sel.size else 0
        m.restore(sel, ms, op.take)
        for side in self.sides:
            if side.twin or op.form == "host":
                side.G.restore(side.host_snap(op.snap), index=op.sel, take=op.take)
                if not side.twin:
                    self.flush()
                continue
            st = side.streams[op.stream]
            s = side.snaps[op.snap]
            if not isinstance(s, _DevSnap):  # a host snapshot goes up once
                keep = side.up(np.ascontiguousarray(s.rec, np.uint32).reshape(-1), st)
                s = side.snaps[op.snap] = _DevSnap(s.layout, keep[1], s.m, [keep])
            keep, ix = [], {}
            if op.sel is not None:
                k = side.up(sel.astype(np.uint32), st)
                keep.append(k)
                ix = dict(index_ptr=k[1].data_ptr(), m=int(sel.size))
            if op.take is not None:
                k = side.up(cols.astype(np.uint32), st)
                keep.append(k)
                ix["take_ptr"] = k[1].data_ptr()
            side.G.restore_device(s.layout, s.rec.data_ptr(), s.m, stream=st.cuda_stream, **ix)
            s.keep.append(keep)
        if m.native:
            self._tier_after(op, "after the restore")

    def _fork(self, op):
        m = self.M["G"]
        sel = full(op.sel, NS)
        self.stats.land_open["fork"] += int(m.open[sel].sum())
        self.stats.src_open["fork"] += int(m.open[op.src])
        self.stats.src_dead["fork"] += int(m.dead[op.src])
        m.fork(op.src, sel)
        for side in self.sides:
            side.G.fork(op.src, op.sel)

    def _promoted(self, flags, p, what):
        """Flags against what the model can say; then the promoted instances are the native tier's."""
        sel, held, is_open, dirty = p["sel"], p["held"], p["open"], p["dirty"]
        bad = np.nonzero(flags & ~(held & ~is_open))[0]
        assert bad.size == 0, self.ctx(f"{what}: promoted what is not interpreter-held and idle: {sel[bad[:8]]}")
        sure = ~is_open & ~dirty
        bad = np.nonzero((flags != held) & sure)[0]
        assert bad.size == 0, self.ctx(f"{what}: promote flags differ from the model at {sel[bad[:8]]} "
                                       f"(got {flags[bad[:8]]})")
        return flags

    def _promote(self, op):
        m = self.M["G"]
        sel = full(op.sel, NS)
        p = dict(sel=sel, held=m.held[sel].copy(), open=m.open[sel] == 1, dirty=m.dirty[sel].copy())
        elig = p["held"] & ~p["open"]
        self.stats.promote_eligible += int((elig & ~p["dirty"]).sum())
        self.stats.promote_dirty += int((elig & p["dirty"]).sum())
        flags = elig & ~p["dirty"]  # without a GPU: the dirty ones stay where they are
        if self.gpu:
            a, b = self.sides
            if op.form == "dev":
                st = a.streams[op.stream]
                keep, ix = [], {}
                if op.sel is not None:
                    keep = a.up(sel.astype(np.uint32), st)
                    ix = dict(index_ptr=keep[1].data_ptr(), m=int(sel.size))
                with a.torch.cuda.stream(st):
                    d_flags = a.torch.full((max(sel.size, 1),), 7, dtype=a.torch.uint8, device="cuda")
                a.G.promote_device(d_flags.data_ptr(), stream=st.cuda_stream, **ix)
                if (elig & p["dirty"]).any():  # the model cannot say: read them now
                    self.flush()
                    a.torch.cuda.synchronize()
                    flags = self._promoted(d_flags.cpu().numpy()[:sel.size].astype(bool), p, "device form")
                else:
                    a.pending.append(dict(p, what="promote", k=self.k, flags=d_flags, count=sel.size, keep=keep))
            else:
                got = a.G.promote(index=op.sel)
                self.flush()
                flags = self._promoted(got, p, "host form")
            twin = self._promoted(b.G.promote(index=op.sel), p, "twin")
            assert np.array_equal(twin, flags), self.ctx(f"the twin promoted other instances: "
                                                         f"{sel[np.nonzero(twin != flags)[0][:8]]}")
        m.held[sel[flags]] = False
        self._tier_after(op, "after the promote")

    def _refuse(self, op):
        """Must be refused with nothing changed: the documented error, and the rest of the sequence as proof."""
        import pytest

        lib = N.lib()
        buf = np.ones(1 << 16, np.int64)  # room for what a call that is wrongly accepted would write
        bp = _bufp(buf)
        for side in self.sides:
            g = side.G
            if op.what == "index":
                bad = op.bad
                sel = bad.astype(np.uint32)
                m = sel.size
                call = dict(step=lambda: g.compute(np.ones(m), index=bad), cancel=lambda: g.cancel(index=bad),
                            reset=lambda: g.reset(index=bad), promote=lambda: g.promote(index=bad),
                            ragged=lambda: g.compute_ragged(np.ones(m), np.ones(m, np.int64), index=bad),
                            snapshot=lambda: g.snapshot(index=bad))[op.via]
                with pytest.raises(ValueError, match="position"):
                    call()
                off = np.arange(m + 1, dtype=np.uint32)
                rc = dict(step=lambda: lib.mk_session_step_indexed(g._h, _bufp(sel), m, bp, bp, bp, bp),
                          cancel=lambda: lib.mk_session_cancel_indexed(g._h, _bufp(sel), m),
                          reset=lambda: lib.mk_session_reset_indexed(g._h, _bufp(sel), m),
                          promote=lambda: lib.mk_session_promote(g._h, _bufp(sel), m, bp, None),
                          ragged=lambda: lib.mk_session_compute_ragged(g._h, _bufp(sel), m, _bufp(off), bp, bp, bp, bp),
                          snapshot=lambda: lib.mk_session_snapshot(g._h, _bufp(sel), m, bp))[op.via]()
                # (a set of the interpreter's tier has nowhere to promote to and answers MK_OK before it looks)
                assert rc == N.MK_EINVAL or (op.via == "promote" and not self.M["G"].native), self.ctx(f"rc {rc}")
            elif op.what == "take":
                s = side.host_snap(op.snap)
                with pytest.raises(ValueError, match="take position"):
                    g.restore(s, index=op.sel, take=op.take)
                sel, col = op.sel.astype(np.uint32), np.asarray(op.take).astype(np.uint32)
                rec = np.ascontiguousarray(s.rec, np.uint32)
                rc = lib.mk_session_restore(g._h, _bufp(sel), sel.size, C.byref(s.layout), _bufp(rec), rec.shape[1],
                                            _bufp(col))
                assert rc == N.MK_EINVAL, self.ctx(f"rc {rc}")
            else:
                with pytest.raises(ValueError, match="ids position"):
                    g.compute_queue(op.ids, np.ones(op.ids.size))
                rc = lib.mk_session_compute_queue(g._h, _bufp(op.ids), bp, op.ids.size, bp, bp, bp)
                assert rc == N.MK_EINVAL, self.ctx(f"rc {rc}")

    def _migrate(self, op):
        ws, wd = ("G", "P") if op.to_p else ("P", "G")
        src, dst = self.M[ws], self.M[wd]
        snap = src.snapshot(op.src_sel)
        dst.restore(op.sel, snap, op.take)
        for side in self.sides:
            s = getattr(side, ws).snapshot(index=op.src_sel)
            if not side.twin:
                self.flush()
            if op.bytes:
                s = mk.SessionSnapshot.frombytes(s.tobytes())
            getattr(side, wd).restore(s, index=op.sel, take=op.take)
            self._tier_agrees(getattr(side, wd).snapshot().held, wd, "after the migration" + " (twin)" * side.twin)

    def _pcall(self, op):
        want = self.M["P"].call(np.arange(NP), op.x)
        for side in self.sides:
            self._same(side.P.compute(op.x, busy_ok=True), want, "call on P" + " (twin)" * side.twin)

    def apply(self, op):
        kind = op.kind
        self.stats.ops[kind] += 1
        self.stats.steered += bool(op.steered)
        if op.form == "dev":
            self.stats.dev_ops[kind] += 1
        if kind in CALL_KINDS:
            self._call(op)
        elif kind in ("cancel", "reset", "call_open"):
            self._simple(op)
        else:
            getattr(self, "_" + kind)(op)
        if self.gpu:
            a, b = self.sides
            if op.form != "dev":
                self.flush()
                self._open_agrees(a, "after the operation")
            self._open_agrees(b, "after the operation (twin)")

    def finish(self):
        """Resume until nothing is open (16 times at most), cancel the rest, one plain call on all of G and of P."""
        self.k = len(self.log)
        if self.gpu:
            self.flush()
        all_g, all_p = np.arange(NS), np.arange(NP)
        for w, idx in (("G", all_g), ("P", all_p)):
            m = self.M[w]
            for _ in range(16):
                if not m.open.any():
                    break
                want = m.call(idx, None)
                for side in self.sides:
                    self._same(getattr(side, w).resume(), want, f"closing resume on {w}" + " (twin)" * side.twin)
            m.cancel(np.nonzero(m.open)[0])
            for side in self.sides:
                getattr(side, w).cancel()
            v = self.gen.inputs(m.n, seed=90000 + m.n)
            want = m.call(idx, v)
            if w == "G":
                self._count(want[1])
            for side in self.sides:
                self._same(getattr(side, w).compute(v, busy_ok=True), want, f"last call on {w}" + " (twin)" * side.twin)
        for side in self.sides:
            self._open_agrees(side, "at the end" + " (twin)" * side.twin)
        if self.gpu:
            a, b = self.sides
            records_equal(a.G.snapshot(), b.G.snapshot(), self.ctx("G and its twin"))
            records_equal(a.P.snapshot(), b.P.snapshot(), self.ctx("P and its twin"))

    def close(self):
        for side in self.sides:
            side.close()
        if self.gpu:
            self.net.close()


def records_equal(a, b, ctx):
    """Two sets' records instance by instance in the terms of SessionSnapshot.canonical: the control and node
    rows, held included, whole; of a stack its depth and the entries below it.  The native section is left
    out: it is the canonical part in the compiled kernel's terms, present only while the native tier holds
    the instance, and canonical() does not read it."""
    lay = a.layout
    assert a.rec.shape[1] == b.rec.shape[1] and (lay.nprog, lay.nstack, lay.stack_cap) == \
        (b.layout.nprog, b.layout.nstack, b.layout.stack_cap), ctx
    head = 9 + 10 * lay.nprog
    diff = (a.rec[:head] != b.rec[:head]).any(axis=0)
    for s in range(lay.nstack):
        base = head + s * (1 + lay.stack_cap)
        da, db = a.rec[base], b.rec[base]
        below = np.arange(lay.stack_cap)[:, None] < da[None, :]
        ea, eb = a.rec[base + 1:base + 1 + lay.stack_cap], b.rec[base + 1:base + 1 + lay.stack_cap]
        diff |= (da != db) | ((ea != eb) & below).any(axis=0)
    if diff.any():
        t = int(np.argmax(diff))
        ca, cb = a.canonical(t), b.canonical(t)
        fields = [k for k in ca if not np.array_equal(ca[k], cb[k])]
        raise AssertionError(f"{ctx}: {int(diff.sum())} records differ; instance {t} in {fields}: "
                             + "; ".join(f"{k} {ca[k]} / {cb[k]}" for k in fields[:4]))


def run(case, *, gpu, upto=None, ops=None, steer=True):
    """The sequence of ``case`` (or the literal ``ops``) on the model and, with ``gpu``, on the sets; ``upto``
    stops after that many operations (a failing prefix replayed by hand).  Returns the Run: .stats, .log."""
    import time

    t0 = time.perf_counter()
    r = Run(case, gpu=gpu, steer=steer)
    r.t_setup = time.perf_counter() - t0  # the sets: on the GPU, mostly the network's run-time compile
    try:
        nops = case.nops if ops is None else len(ops)
        for k in range(nops if upto is None else min(upto, nops)):
            op = r.gen.draw() if ops is None else Op(ops[k])
            r.log.append(op)
            r.k = k
            r.apply(op)
        r.finish()
    finally:
        r.close()
        r.t_total = time.perf_counter() - t0
    return r
