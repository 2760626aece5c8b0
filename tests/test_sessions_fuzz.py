"""Every call form of a SessionSet interleaved on one set, against the CPU
oracle (tests/sessfuzz.py: the model, the state-aware generator, the driver
and the twin set).

The feature files (test_sessions_indexed, _ragged, _queue, _snapshot,
_promote) script one form each on six fixed networks.  Here random sequences
of 48 operations mix all of them -- plain, indexed, burst, ragged and queue
calls in host and device form, resumes, cancels, resets, snapshots, restores,
forks, promotions, refused calls and migration to a second set on the other
tier -- on n = 600 instances (two full blocks and a partial one) of those
networks and of 34 more.

The CPU tests run the very sequences of the GPU tests on the model alone: they
check the model's replay against itself and that the sequences meet what they
are for (FLOORS below: conditions that keep the GPU tests from going vacuous,
not measurements).  Sequences are grouped for that: each non-trivial network
of test_sessions_indexed.NETS with its 12 sequences (6 seeds on either tier),
the 24 random networks, and the 10 stack networks (stack loops, deep stacks);
48 operations of one sequence cannot hold 10 of each of 15 kinds.  ``example``
never leaves a call open, hands nothing off and cannot end, so no pre-state
but "idle and native" exists for it: its two sequences run, and are checked
for their one status only."""
import functools

import numpy as np
import pytest

import sessfuzz as sf
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from test_sessions_indexed import NETS, NS, tier  # noqa: F401  (tier: a fixture)
from tisgen import deep_stack_network, random_network, stack_loop_network

SEEDS = range(6)
# stack_loop_network seeds with the capacity and budget at which the oracle, on four plain calls of 600
# instances each with a resume in between, shows hand-offs (MK_ST_BUDGET) and overflows both:
# BUDGET / STACK_OVERFLOW of 2400 results 264 / 1392, 547 / 1752, 1240 / 61, 484 / 1775, 995 / 722, 600 / 1479
STACK_LOOPS = {4: (17, 40), 6: (17, 40), 9: (17, 40), 13: (8, 40), 19: (17, 40), 21: (17, 40)}
DEEP_BUDGET = 3000  # test_gpu_parity.test_deep_stack_sessions


def nets_case(name, tier, seed):  # noqa: F811
    nodes, kw, gen = NETS[name]()
    return sf.Case(name, nodes, kw, gen, tier, seed)


def random_case(seed):
    # test_gpu_parity.test_sessions_random_networks' rotation; full-range inputs as there
    kw = dict(budget=[37, 200, 1000][seed % 3], stack_cap=[1, 3, 8, 16, 17, 40, 1024][seed % 7])
    return sf.Case(f"random_network({seed})", random_network(seed), kw, {}, "auto", seed, group="random")


def stack_loop_case(seed):
    rows, gen = stack_loop_network(seed)
    cap, budget = STACK_LOOPS[seed]
    return sf.Case(f"stack_loop_network({seed})", rows, dict(budget=budget, stack_cap=cap), gen, "auto", seed,
                   group="stack")


def deep_case(seed):
    # tisgen.deep_stack_inputs: full-range inputs, every seventh 0
    return sf.Case(f"deep_stack_network({seed})", deep_stack_network(seed, session=True), dict(budget=DEEP_BUDGET), {},
                   "auto", seed, zero_every=7, group="stack")


GROUPS = {name: [(nets_case, (name, t, s)) for t in ("native", "interp") for s in SEEDS] for name in NETS
          if name != "example"}
GROUPS["random"] = [(random_case, (s,)) for s in range(24)]
GROUPS["stack"] = [(stack_loop_case, (s,)) for s in STACK_LOOPS] + [(deep_case, (s,)) for s in range(4)]


@functools.lru_cache(maxsize=None)
def model_run(make, args, steer=True):
    return sf.run(make(*args), gpu=False, steer=steer)


@functools.lru_cache(maxsize=None)
def group_stats(group, steer=True):
    total = sf.Stats()
    for make, args in GROUPS[group]:
        total.add(model_run(make, args, steer).stats)
    return total


@functools.lru_cache(maxsize=None)
def can_produce(group):
    """Which statuses the oracle shows the group's networks producing at all: plain calls on 600 instances
    with a resume in between, no fuzz involved; a status counts from 2 % of the results."""
    seen = sf.Counter()
    done = set()
    for make, args in GROUPS[group]:
        case = make(*args)
        if case.name in done:
            continue
        done.add(case.name)
        o = po.OracleSessions(po.OracleNet(case.nodes), NS, stack_cap=case.kw.get("stack_cap"))
        for k in range(4):
            x = po.gen_inputs(77 + k, NS, **case.gen)
            for st in (o.compute(x, budget=case.kw.get("budget"))[1], o.compute(None, budget=case.kw.get("budget"))[1]):
                for code, c in zip(*np.unique(st & N.MK_ST_REASON_MASK, return_counts=True)):
                    seen[sf.ST_NAMES.get(int(code))] += int(c)
    return {k for k, v in seen.items() if v >= 0.02 * sum(seen.values())}


# ---- CPU: the model against itself ---------------------------------------------------------
def _drive(m, rng, gen, nops, seed):
    """A few calls, resumes and cancels on random subsets."""
    out = []
    for k in range(nops):
        sel = np.sort(rng.choice(m.n, int(rng.integers(1, m.n + 1)), replace=False))
        c = rng.random()
        if c < 0.6:
            out.append(m.call(sel, po.gen_inputs(seed + k, sel.size, **gen)))
        elif c < 0.8:
            out.append(m.call(sel, None))
        elif c < 0.9:
            m.cancel(sel)
        else:
            m.reset(sel[:5])
    return out


def _same_answers(a, b, ctx):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for p, q in zip(x, y):
            assert np.array_equal(p, q), (ctx, k)


@pytest.mark.parametrize("name", list(NETS))
def test_model_restore_replays_the_history(name):
    nodes, kw, gen = NETS[name]()
    n = 40
    a, b = sf.SessModel(nodes, n, **kw), sf.SessModel(nodes, n, **kw)
    for m in (a, b):
        _drive(m, np.random.default_rng(1), gen, 8, 100)
    assert all(x == y for x, y in zip(a.hist, b.hist)) and max(len(h) for h in a.hist) >= 2
    sel = np.arange(3, 33)
    snap = a.snapshot(sel)
    _drive(a, np.random.default_rng(2), gen, 8, 200)  # a goes elsewhere ...
    assert any(x != y for x, y in zip(a.hist, b.hist))
    a.restore(sel, snap)  # ... and comes back
    rest = np.setdiff1d(np.arange(n), sel)
    a.restore(rest, b.snapshot(rest))
    for f in ("open", "dead", "dirty", "held"):
        assert np.array_equal(getattr(a, f)[sel], getattr(b, f)[sel]), f
    _same_answers(_drive(a, np.random.default_rng(3), gen, 8, 300), _drive(b, np.random.default_rng(3), gen, 8, 300),
                  f"{name}: restored and never-left instances answer differently")
    # take: every instance the same column
    a.restore(sel, snap, np.full(sel.size, 7))
    one = a.call(sel, po.gen_inputs(9, 1, **gen).repeat(sel.size))
    assert all(np.unique(x).size == 1 for x in one)


@pytest.mark.parametrize("name", list(NETS))
def test_model_fork_equals_replaying_the_source(name):
    nodes, kw, gen = NETS[name]()
    n = 30
    a, b = sf.SessModel(nodes, n, **kw), sf.SessModel(nodes, n, **kw)
    every = np.arange(n)
    for k in range(4):
        v = po.gen_inputs(50 + k, 1, **gen)
        if k == 2:
            a.call([17], None)
            b.call(every, None)
        a.call([17], v)
        b.call(every, v.repeat(n))  # every instance of b replays 17's calls, as test_fork builds its reference
    a.fork(17, np.setdiff1d(every, [17]))
    for f in ("open", "dead", "dirty", "held"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    v = po.gen_inputs(60, n, **gen)
    _same_answers([a.call(every, v), a.call(every, None)], [b.call(every, v), b.call(every, None)], name)


def test_generator_is_a_function_of_the_case():
    a = sf.run(nets_case("stackloop7", "native", 3), gpu=False)
    b = sf.run(nets_case("stackloop7", "native", 3), gpu=False)
    assert [str(x) for x in a.log] == [str(x) for x in b.log] and len(a.log) == sf.NOPS
    c = sf.run(nets_case("stackloop7", "native", 4), gpu=False)
    assert [str(x) for x in a.log] != [str(x) for x in c.log]
    # a prefix replayed by hand, and a literal list of operations
    d = sf.run(nets_case("stackloop7", "native", 3), gpu=False, upto=10)
    assert [str(x) for x in d.log] == [str(x) for x in a.log[:10]]
    e = sf.run(nets_case("stackloop7", "native", 3), gpu=False, ops=[dict(x) for x in a.log[:10]])
    assert e.stats.status == d.stats.status


# ---- CPU: what the sequences of the GPU tests meet ---------------------------------------------
FLOOR_KIND, FLOOR_VISITS, FLOOR_RESULTS, CAP_SHARE = 10, 200, 500, 0.40


@pytest.mark.parametrize("group", list(GROUPS))
def test_sequences_cover_what_they_are_for(group):
    s = group_stats(group)
    can = can_produce(group)
    print(f"{group}: {s.line()}")
    print(f"{group}: operations {dict(s.ops)}")
    print(f"{group}: the oracle alone shows {sorted(can)}")
    for k in sf.KINDS:
        assert s.ops[k] >= FLOOR_KIND, (group, k, s.ops[k])
    states = ["idle_native", "idle_interp", "open"] + (["ended"] if "STACK_OVERFLOW" in can else [])
    for k in sf.CALL_KINDS:
        for state in states:
            assert s.visits[(k, state)] >= FLOOR_VISITS, (group, k, state, s.visits[(k, state)])
    assert s.promote_eligible >= FLOOR_VISITS and s.promote_dirty >= 20, (group, s.promote_eligible, s.promote_dirty)
    for k in ("restore", "fork"):
        assert s.land_open[k] >= FLOOR_VISITS, (group, k, s.land_open[k])
        assert s.src_open[k] >= 2, (group, k, "sources with a call open", s.src_open[k])
        if "STACK_OVERFLOW" in can:
            assert s.src_dead[k] >= 2, (group, k, "ended sources", s.src_dead[k])
    assert s.share("CALL_OPEN") <= CAP_SHARE and s.share("STACK_OVERFLOW") <= CAP_SHARE, (group, s.line())
    for name in ("HAS_OUTPUT", "BUDGET", "CALL_OPEN"):
        assert s.status[name] >= FLOOR_RESULTS, (group, name, s.status[name])
    for name in ("QUIESCENT", "STACK_OVERFLOW"):
        if name in can:
            assert s.status[name] >= FLOOR_RESULTS, (group, name, s.status[name])


def test_example_sequences_only_ever_answer():
    for t in ("native", "interp"):
        s = model_run(nets_case, ("example", t, 0)).stats
        # every call answers; a resume finds nothing open (reason 0 without an output)
        assert s.status["HAS_OUTPUT"] >= FLOOR_RESULTS and set(s.status) <= {"HAS_OUTPUT", "NONE"}, s.line()


# ---- GPU ---------------------------------------------------------------------------------------
def _fuzz(case, want_tier=None):
    if want_tier:
        assert case.tier == want_tier
    r = sf.run(case, gpu=True)
    print(f"{case}: sets {r.t_setup:.2f} s, all {r.t_total:.2f} s; {r.stats.line()}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", [k for k in NETS if k != "example"])
def test_fuzz_nets(gpu, name, tier, seed):  # noqa: F811
    _fuzz(nets_case(name, tier, seed), tier)


@pytest.mark.gpu
def test_fuzz_example(gpu, tier):  # noqa: F811
    _fuzz(nets_case("example", tier, 0), tier)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_fuzz_random_networks(gpu, seed):
    # native where plan() says so: the case's tier is the session compiler's word taken on the CPU, and
    # sessfuzz.Side asserts every set's plan() against it
    _fuzz(random_case(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(STACK_LOOPS))
def test_fuzz_stack_loop_networks(gpu, seed):
    _fuzz(stack_loop_case(seed), "native")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_fuzz_deep_stack_sessions(gpu, seed):
    _fuzz(deep_case(seed), "native")
