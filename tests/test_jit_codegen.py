"""Tier 3 (native kernel per network, misaka-net_amd/csrc/tis_jit.cpp) on CPU.

The generator emits the lane function as portable C++; here it is compiled
with g++ (all networks of a case list into one shared object) and run lane by
lane against the oracle -- bit-exact out/status/steps.  The GPU runs the same
function inside the hiprtc-compiled kernel (tests/test_gpu_parity.py, mode
"jit"); that the full module compiles for gfx950 is checked here too (hiprtc
needs no GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd.network import NodeSpec
from oracle import pyoracle as po
import schedcheck as sc
from tisgen import (census_classes, deep_seed_kwargs, deep_stack_inputs, deep_stack_network, deep_stack_peaks,
                    stack_loop_network, loop_cases, random_network, rotated_seed_kwargs, rotated_stack_loop_cases,
                    rotated_stack_loop_network, SELF_LOOP_STEPS, SELF_LOOP_EXITS, self_loop_budgets,
                    self_loop_gpu_programs, self_loop_inputs, self_loop_meta, self_loop_programs)

SEED = 0x4D49534B41

HEADER = """#include <cstdint>
#include <cstddef>
#include <vector>
#define MK_FN static inline
#define MK_LANE_CHECKED 1
#define MK_LOOP_NEED(pol) 0u
#define MK_KEEP(m, need) (m)
#define MK_ALL(p) (p)
#define MK_SLOT_ST(b, ss, s, v) ((b)[(uint64_t)(s) * (ss)] = (v))
#define MK_SLOT_LD(b, ss, s) ((b)[(uint64_t)(s) * (ss)])
#define MK_SLOT_STX(b, ss, s, v) ((b)[(uint64_t)(s) * (ss)] = (v))
#define MK_SLOT_LDX(b, ss, s) ((b)[(uint64_t)(s) * (ss)])
#define MK_FLAG_GT(x) ((int32_t)((x) > 0))
#define MK_FLAG_LT(x) ((int32_t)((x) < 0))
#define MK_FLAG_NZ(x) ((int32_t)((x) != 0))
#define MK_FLAG_MIN(x, f) ((int32_t)((uint32_t)(x) < (uint32_t)(f) ? (uint32_t)(x) : (uint32_t)(f)))
#define MK_MAD24(f, k, x) ((int32_t)((uint32_t)(x) + (uint32_t)(f) * (uint32_t)(k)))
#define MK_SATDEC(x) ((int32_t)((uint32_t)(x) ? (uint32_t)(x) - 1u : 0u))
#define MK_OPAQUE1() 1u
#define MK_SATSUB(x, o) ((int32_t)((uint32_t)(x) >= (o) ? (uint32_t)(x) - (o) : 0u))
"""


def build_lanes(cases, path):
    """cases: [(lane source, nslots)] -> CDLL exporting run<i>(in, n, budget, out, st, steps)."""
    parts = [HEADER]
    for i, (src, nslots) in enumerate(cases):
        parts.append(f"namespace n{i} {{\n{src}\n}}\n")
        parts.append(
            f'extern "C" void run{i}(const int64_t *in, size_t n, uint32_t budget, int32_t *out, uint8_t *st,'
            f" uint32_t *sp) {{\n"
            f"    std::vector<int32_t> slots({nslots} + 1, 0x5A5A5A5A);\n"
            f"    for (size_t i = 0; i < n; i++) {{\n"
            f"        uint32_t s, t;\n"
            f"#if MK_JIT_MACHINE == 0\n"  # the kernel's dispatch: unguarded lane when no path reaches the budget
            f"        const int32_t o = budget > MK_MAX_STEPS ? n{i}::mk_lane_ng(in[i], budget, slots.data(), 1, &s, &t)\n"
            f"                                                : n{i}::mk_lane(in[i], budget, slots.data(), 1, &s, &t);\n"
            f"#else\n"
            f"        const int32_t o = n{i}::mk_lane(in[i], budget, slots.data(), 1, &s, &t);\n"
            f"#endif\n"
            f"        out[i] = (t & 0x10) ? o : 0; st[i] = (uint8_t)t; sp[i] = s;\n"
            f"    }}\n}}\n")
    src = path + ".cpp"
    with open(src, "w") as f:
        f.write("".join(parts))
    so = path + ".so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-w", "-o", so, src])
    return C.CDLL(so)


def run_lane(lib, i, xs, budget):
    v = np.ascontiguousarray(np.asarray(xs, dtype=np.int64))
    out = np.zeros(v.size, np.int32)
    st = np.zeros(v.size, np.uint8)
    sp = np.zeros(v.size, np.uint32)
    getattr(lib, f"run{i}")(C.c_void_p(v.ctypes.data), C.c_size_t(v.size), C.c_uint32(budget),
                            C.c_void_p(out.ctypes.data), C.c_void_p(st.ctypes.data), C.c_void_p(sp.ctypes.data))
    return out, st, sp


def check_cases(tmp_path, cases, machine=False):
    """cases: [(label, nodes, xs, kw)] -- every case compiled and compared.
    ``machine``: the resumable (machine-shape) lane for every case."""
    srcs, keep, lane = [], [], {}
    emitted, nets = {}, {}  # cases that share their nodes object (a budget sweep): one lane source, one oracle net
    for label, nodes, xs, kw in cases:
        key = (id(nodes), kw.get("stack_cap"), kw.get("stop_on_output", False))
        try:
            if key not in emitted:
                emitted[key] = sc.jit_lane(nodes, stack_cap=key[1], stop_on_output=key[2], machine=machine)
            src, ns = emitted[key]
        except sc.NotCompiled:
            continue  # tier 1 handles it; covered elsewhere
        if (src, ns) not in lane:  # cases that differ in the budget only share a lane
            lane[(src, ns)] = len(srcs)
            srcs.append((src, ns))
        keep.append((label, nodes, xs, kw, lane[(src, ns)]))
    assert keep, "no case compiled"
    lib = build_lanes(srcs, str(tmp_path / "lanes"))
    for label, nodes, xs, kw, i in keep:
        got = run_lane(lib, i, xs, kw.get("budget") or (1 << 20))
        if id(nodes) not in nets:
            nets[id(nodes)] = po.OracleNet(nodes)
        ref = nets[id(nodes)].compute_batch(xs, **kw)
        bad = np.nonzero((got[0] != ref[0]) | (got[1] != ref[1]) | (got[2] != ref[2]))[0]
        assert not bad.size, (label, int(bad[0]), [g[bad[0]] for g in got], [r[bad[0]] for r in ref])
    return [k[0] for k in keep]


@pytest.mark.parametrize("machine", [False, True])
def test_configs(tmp_path, machine):
    cases = []
    for name in sorted(mk.networks.CONFIGS):
        kind = 1 if name.startswith("c5") else 0
        cases.append((name, mk.networks.CONFIGS[name](), po.gen_inputs(SEED, 2000, kind=kind, mask=1023), {}))
    cases.append(("c4_d1024", mk.networks.pipeline_network(1024), po.gen_inputs(SEED, 40), {}))
    for d in (64, 256):  # every node's stack order reaches the output (networks.pipeline_program)
        cases.append((f"c4_observe_d{d}", mk.networks.pipeline_network(d, observe=True), po.gen_inputs(SEED, 200), {}))
    cases.append(("c5_all_trips", mk.networks.countdown_network(), np.arange(0, 1024, dtype=np.int64), {}))
    for b in (1, 11, 12, 13):
        cases.append((f"c2_budget{b}", mk.networks.example_network(), po.gen_inputs(SEED, 300), {"budget": b}))
        cases.append((f"c5_budget{b}", mk.networks.countdown_network(),
                      po.gen_inputs(SEED, 300, kind=1, mask=1023), {"budget": b * 37}))
    done = check_cases(tmp_path, cases, machine)
    # every config fits the native tier (the deep pipelines once their
    # constant-bound PUSH/POP loops are rolled back into loops)
    assert set(c[0] for c in cases) == set(done)


@pytest.mark.parametrize("machine", [False, True])
def test_wide_immediates_and_stop(tmp_path, machine):
    prog = ("IN ACC\nADD 2147483648\nADD 4294967295\nSUB 2147483649\nADD -4294967296\n"
            "ADD 9223372036854775807\nSUB -9223372036854775808\nMOV ACC, n:R1\nMOV R1, ACC\n"
            "JRO 2147483648\nNOP\nOUT ACC\nJLZ L\nOUT 1\nL: OUT 2")
    loop = [("a", "program", "JRO 0"), ("b", "program", "OUT 3\nJRO 0")]
    cases = [("wide", [("n", "program", prog)], po.gen_inputs(SEED, 2048), {}),
             ("budget", loop, [0] * 8, {"budget": 11}),
             ("stop", loop, [0] * 8, {"stop_on_output": True})]
    assert len(check_cases(tmp_path, cases, machine)) == 3


def test_paired_dispatch_marker(monkeypatch):
    # Two lanes per thread in the tile-sorted kernel (round 6, MK_PAIR in
    # kMachineSortKernel): networks without stack slots, one sweep pass for
    # two sorted chunks; the lanes' own code is the one-lane form, so every
    # machine-shape parity test here and on the GPU covers it.  Stack slots
    # (one column per thread) and MK_JIT_PAIR=0 keep one lane per thread.
    src, ns = sc.jit_lane(mk.networks.countdown_network(), machine=True)
    assert ns == 0 and "#define MK_PAIR 1" in src
    src, ns = sc.jit_lane(mk.networks.pipeline_network(64), machine=True)
    assert ns > 0 and "#define MK_PAIR 1" not in src
    monkeypatch.setenv("MK_JIT_PAIR", "0")
    src, _ = sc.jit_lane(mk.networks.countdown_network(), machine=True)
    assert "#define MK_PAIR 1" not in src


def test_loop_phases(tmp_path):
    # every path of the machine shape's self-loops (tisgen.loop_cases)
    cases = [(lbl, nodes, np.asarray(xs, np.int64), kw) for lbl, nodes, xs, kw in loop_cases()]
    assert len(check_cases(tmp_path, cases, machine=True)) == len(cases)


# ---- the self-loop family (tisgen.self_loop_programs) ---------------------------
# Every step, exit test and body that moves emit_self_loop to another form, at
# every budget that walks the unguarded iterations T across its chunk
# boundaries.  Lane by lane here (MK_KEEP and MK_ALL are the lane's own, the
# flag and bump macros plain C); tests/test_gpu_parity.py runs the curated
# rows on the hardware, where the asm, the wave-uniform T and the waves whose
# lanes disagree about the 2^30 range check are.

SL_LANES = 64
SL_BLOCK = 78  # programs per block of test_self_loop_family
SL_KNOBS = {"count0": {"MK_JIT_SAT_COUNT": "0"}, "unroll1": {"MK_JIT_LOOP_UNROLL": "1"},
            "unroll3": {"MK_JIT_LOOP_UNROLL": "3"}, "unroll64": {"MK_JIT_LOOP_UNROLL": "64"}}


def _self_loop_cases(rows, uf=None):
    cases = []
    for label, nodes, _ in rows:
        xs = np.asarray(self_loop_inputs(label, SL_LANES), np.int64)
        cases += [(f"{label} budget {b}", nodes, xs, {"budget": b}) for b in self_loop_budgets(label, uf=uf)]
    return cases


@pytest.mark.parametrize("which", [f"all-{b}" for b in range((len(self_loop_programs()) + SL_BLOCK - 1) // SL_BLOCK)] +
                         [f"{k}-gpu" for k in SL_KNOBS])
def test_self_loop_family(tmp_path, monkeypatch, which):
    # all-<block>: every row at every budget, default knobs; <knob>-gpu: the
    # GPU's rows without the counter form, and with other chunk sizes (the
    # budgets then walk that chunk size)
    knob, part = which.split("-")
    uf = None
    if knob == "all":
        rows = self_loop_programs()[int(part) * SL_BLOCK:(int(part) + 1) * SL_BLOCK]
    else:
        rows = self_loop_gpu_programs()
        for name, value in SL_KNOBS[knob].items():
            monkeypatch.setenv(name, value)
        uf = int(SL_KNOBS[knob].get("MK_JIT_LOOP_UNROLL", 0)) or None
    cases = _self_loop_cases(rows, uf)
    assert len(check_cases(tmp_path, cases, machine=True)) == len(cases)  # none declined


def emitted_loop_forms(src):
    """[(form, uf, inc, T32's bound or None, inverted exit)] of the self-loops
    in a machine lane's source, read off the text emit_self_loop writes."""
    found = []
    for case in re.split(r"\n    case \d+u: \{\n", src[src.index("MK_FN void mk_run"):])[1:]:
        if "const uint32_t T = smax" not in case:
            continue
        uf = int(re.search(r"while \(more && T - it >= (\d+)u\)", case).group(1))
        inc = int(re.search(r"const uint32_t T = .* / (\d+)u : 0u;", case).group(1))
        t32 = re.search(r"const uint32_t T32 = T < (\d+)u", case)
        inverted = re.search(r"L\.sb = \(a \|\| \(!", case) is not None
        if "uint32_t k = 0u;" in case:  # the per-lane counter
            assert "L.steps = s0 + %du * k;" % inc in case and t32 is None
            found.append(("k", uf, inc, None, inverted))
            continue
        ind = re.search(r"const int64_t i0 = L\.r(\d+);", case).group(1)
        assert t32
        trip = "inverse" if re.search(r"L\.steps = s0 \+ \d+u \* \(\(uint32_t\)\(.* >> \d+\) \* \d+u\);", case) else "shift"
        if trip == "shift":
            assert re.search(r"L\.steps = s0 \+ \d+u \* \(uint32_t\)\(.* >> \d+\);", case)
        phase = [name for name, mark in (("counter", "const uint32_t z0 = f0 ?"), ("satdown", "const int32_t f0 = MK_FLAG_GT(x), x0 = x;"),
                                         ("mad24", "x = MK_MAD24(f, "), ("pm1", "(uint32_t)f);"),
                                         ("narrow", "    int64_t n%s = (int64_t)x;\n" % ind)) if mark in case]
        assert len(phase) == 1, (phase, case)
        found.append((f"{phase[0]}/{trip}", uf, inc, int(t32.group(1)), inverted))
    return found


SL_FORMS = {"satdown/shift", "counter/shift", "counter/inverse", "pm1/shift", "mad24/shift", "mad24/inverse",
            "narrow/shift", "narrow/inverse", "k"}


def test_self_loop_forms_are_pinned():
    # each row reaches the form its generator names; a change in
    # emit_self_loop that moves a row to another form fails here
    seen, t32_zero, polar = set(), 0, set()
    for label, nodes, want in self_loop_programs():
        loops = emitted_loop_forms(sc.jit_lane(nodes, machine=True)[0])
        assert "+".join(sorted(f[0] for f in loops)) == want, (label, loops)
        m = self_loop_meta(label)
        assert len(loops) == m["nloops"] and (m["uf"], m["inc"]) in [(f[1], f[2]) for f in loops], (label, loops, m)
        seen |= {f[0] for f in loops}
        t32_zero += any(f[3] == 0 for f in loops)
        polar |= {f[4] for f in loops}
        if m["nloops"] == 1:
            assert loops[0][4] == label.split("/")[2].startswith("i"), (label, loops)
    assert seen == SL_FORMS, seen ^ SL_FORMS
    assert t32_zero >= 12 and polar == {False, True}  # |step| > 2^30 - 1: the narrow phase entered for no iteration


def test_self_loop_gpu_subset_covers_forms_and_steps():
    rows, few = self_loop_gpu_programs(), self_loop_gpu_programs(few=True)
    assert len(rows) == 48 and len(few) == 12 and {r[0] for r in few} <= {r[0] for r in rows}
    assert {f for r in rows for f in r[2].split("+")} == SL_FORMS
    single = [r[0].split("/") for r in rows if not r[0].startswith("chain/")]
    assert {abs(int(s[1])) for s in single} == set(SELF_LOOP_STEPS)
    assert {s[2] for s in single} == set(SELF_LOOP_EXITS)
    assert {s[0] for s in single} == {"bump", "bak", "twice", "neg", "other", "addacc"}
    assert {f.split("/")[0] for r in few for f in r[2].split("+")} >= {"satdown", "counter", "mad24", "narrow", "k"}


def self_loop_endings(label, nodes, lanes=SL_LANES):
    """Which ways the row's lanes end in its last loop over its inputs and
    budgets, from the oracle alone: steps at the loop's entry from the row's
    `head` program, iterations from the steps beyond them."""
    m = self_loop_meta(label)
    xs = np.asarray(self_loop_inputs(label, lanes), np.int64)
    net = po.OracleNet(nodes)
    entry = po.OracleNet([("n", "program", m["head"])]).compute_batch(xs)[2].astype(np.int64) - 1  # less its OUT
    _, st, sp = net.compute_batch(xs, budget=6000)
    done = (st & mk._native.MK_ST_REASON_MASK) != mk._native.MK_ST_BUDGET
    tail = len(nodes[0][2].splitlines()) - len(m["head"].splitlines()) + 1 - m["inc"]  # lines behind the loop
    trips = -(-(sp.astype(np.int64) - tail - entry) // m["inc"])
    ends = set()
    if (done & (trips >= 2 * m["uf"])).any():
        ends.add("late")
    if (done & (trips == 1)).any():
        ends.add("first")   # the block ahead of the loop runs its first iteration: such a lane never enters it
    if (done & (trips == 2)).any():
        ends.add("second")  # ... and this one leaves at the first test the loop's own code makes

    def cut_by(b):  # iterations completed by the lanes budget b stops inside the loop
        _, stb, spb = net.compute_batch(xs, budget=b)
        cut = ((stb & mk._native.MK_ST_REASON_MASK) == mk._native.MK_ST_BUDGET) & (spb > entry) & \
            (~done | (spb < sp - tail))
        return (spb.astype(np.int64) - entry)[cut] // m["inc"]

    budgets = self_loop_budgets(label)
    if any((cut_by(b) >= m["uf"]).any() for b in reversed(budgets)):
        ends.add("budget-unguarded")  # behind one unguarded chunk or more
    if any((cut_by(b) < m["uf"]).any() for b in budgets):
        ends.add("budget-guarded")    # the budget leaves the loop no unguarded chunk
    return ends


def test_self_loop_cases_end_every_way():
    # A row whose lanes all ended one way would pass the family test without
    # running the rest of its loop's code.  Rows that cannot leave by the
    # branch after 2 uf iterations, or at the first test, by name and reason;
    # the other three ways are asked of them too.
    reasons = {"JEZ": "stays only while the register is 0", "iJNZ": "stays only while the register is 0"}
    cannot = {}
    for label, _, _ in self_loop_programs():
        m = self_loop_meta(label)
        if m["late"] and m["first"]:
            continue
        body, step, exit_ = label.split("/")
        cannot[label] = ({"first"}, "a != 0 loop leaves at its first test from x = step: 512 times the input is "
                         "never an odd step") if m["late"] else \
            ({"late", "budget-unguarded"} if body == "bump" and exit_ in reasons else  # two trips at the most
             {"late", "second"},  # one trip or no end (2 x + s: it doubles away from 0)
             "the exit test reads a register the body does not write" if body == "other" else
             "2 x + s leaves 2^63 within 64 iterations" if body == "addacc" else
             reasons.get(exit_, "the bump runs away from the exit test"))
    assert len(cannot) * 5 <= len(self_loop_programs()), len(cannot)
    for label, nodes, _ in self_loop_programs():
        want = {"late", "first", "second", "budget-unguarded", "budget-guarded"} - cannot.get(label, (set(),))[0]
        if "first" not in want:
            want.discard("second")  # x = 2 step is as far from 512 times an input
        ends = self_loop_endings(label, nodes)
        assert want <= ends, (label, want - ends, cannot.get(label))


# The countdown's saturating decrements in asm blocks of MK_JIT_SAT_BLOCK
# (default 4) and the counter form of countdowns by other steps
# (MK_JIT_SAT_COUNT, default on; "count0" turns it off): every loop path, and
# C5 over all trip counts and at budgets inside its loops.
@pytest.mark.parametrize("mode", ["count0", "b8", "b32", "default"])
def test_countdown_forms(tmp_path, monkeypatch, mode):
    if mode == "count0":
        monkeypatch.setenv("MK_JIT_SAT_COUNT", "0")
    elif mode.startswith("b"):  # other asm block sizes
        monkeypatch.setenv("MK_JIT_SAT_BLOCK", mode[1:])
    cases = [(lbl, nodes, np.asarray(xs, np.int64), kw) for lbl, nodes, xs, kw in loop_cases()]
    cases.append(("c5_all_trips", mk.networks.countdown_network(), np.arange(-3, 1024, dtype=np.int64), {}))
    for b in (1, 2, 3, 37, 400, 1500):
        cases.append((f"c5_budget{b}", mk.networks.countdown_network(),
                      po.gen_inputs(SEED, 300, kind=1, mask=1023), {"budget": b}))
    assert len(check_cases(tmp_path, cases, machine=True)) == len(cases)


@pytest.mark.parametrize("machine", [False, True])
@pytest.mark.parametrize("block", range(4))
def test_random_networks(tmp_path, block, machine):
    cases = []
    for seed in range(block * 40, block * 40 + 40):
        kw = dict(budget=[37, 200, 1000][seed % 3], stack_cap=[1, 3, 8, 16, 17, 40, 1024][seed % 7],
                  stop_on_output=(seed % 5 == 4))
        cases.append((f"seed{seed}", random_network(seed), po.gen_inputs(seed * 7919 + 1, 256), kw))
    assert len(check_cases(tmp_path, cases, machine)) >= 30


@pytest.mark.parametrize("machine", [False, True])
@pytest.mark.parametrize("block", range(3))
def test_dynamic_stack_networks(tmp_path, block, machine):
    # stack depths that follow the data (tisgen.stack_loop_network): dynamic
    # stacks (STX/LDX, in-line OVF, the empty-check branch), capacities and
    # budgets that end lanes inside pushes and pops
    cases = []
    for seed in range(block * 30, block * 30 + 30):
        rows, gen = stack_loop_network(seed)
        kw = dict(budget=[None, 57, 300, 2000][seed % 4], stack_cap=[None, 3, 17, 64, 200][seed % 5])
        kw = {k: v for k, v in kw.items() if v is not None}
        cases.append((f"seed{seed}", rows, po.gen_inputs(seed + 5, 96, **gen), kw))
    for cls in ("data_dependent_stack_depth", "two_stacks_independent_depths"):
        nodes = census_classes()[cls][0][1]
        for cap in (None, 5, 200):
            xs = po.gen_inputs(3, 256, kind=1, mask=255)
            cases.append((f"{cls}_{cap}", nodes, xs, {"stack_cap": cap} if cap else {}))
    assert len(check_cases(tmp_path, cases, machine)) >= 24


def overflowed(status):
    """Lanes the oracle ended by a stack overflow."""
    return (status & mk._native.MK_ST_REASON_MASK) == mk._native.MK_ST_STACK_OVERFLOW


def rotated_case_groups(cases, ref_of):
    """{program: [(label, overflowing lanes, their largest oracle step count)]}
    and the check that no program passes by never overflowing: some capacity
    and budget of each has lanes that overflow, and one of them overflows past
    the unguarded phases' largest chunk (32 iterations; an iteration retires
    at most every line of the network once)."""
    groups = {}
    for label, nodes, xs, kw in cases:
        st, sp = ref_of(label, nodes, xs, kw)[1:3]
        ov = overflowed(st)
        lines = sum(len([ln for ln in n[2].splitlines() if ln.strip()]) for n in nodes if n[1] == "program")
        row = (label, int(ov.sum()), int(sp[ov].max()) if ov.any() else 0, lines)
        groups.setdefault(label.split("/")[0], []).append(row)
    for name, rows in groups.items():
        over = [r for r in rows if r[1] > 0]
        assert over, f"{name}: no capacity / budget with an overflowing lane"
        assert any(steps > 33 * lines for _, _, steps, lines in over), f"{name}: no overflow past 32 iterations"
    return groups


# Loops that count before they push (tisgen.rotated_stack_loop_cases): the
# induction register's bump ahead of a capacity exit.  A lane that overflows
# inside an unguarded chunk reported its steps one iteration too high
# (sub_push-rot at capacity 64, input 65: 197 for the oracle's 194; two PUSHes
# per iteration, input 33: 134 for 130; the counter and the pushed value both
# bumped first, capacities 33 / 64 / 200: 209 / 395 / 1211 for 203 / 389 /
# 1205) until emit_self_loop took only bumps behind the last exit.
@pytest.mark.parametrize("machine", [False, True])
def test_rotated_stack_loops(tmp_path, machine):
    cases = [(lbl, nodes, np.asarray(xs, np.int64), kw) for lbl, nodes, xs, kw in rotated_stack_loop_cases()]
    groups = rotated_case_groups(cases, lambda lbl, nodes, xs, kw: po.OracleNet(nodes).compute_batch(xs, **kw))
    assert len(groups) == 14 and all(len(rows) == 32 for rows in groups.values())
    assert len(check_cases(tmp_path, cases, machine)) == len(cases)


@pytest.mark.parametrize("machine", [False, True])
@pytest.mark.parametrize("block", range(2))
def test_rotated_stack_networks(tmp_path, block, machine):
    # tisgen.rotated_stack_loop_network: the counter bump first, in the
    # middle or last in every loop body of the seeded dynamic-stack networks
    cases, overflowing = [], 0
    for seed in range(block * 30, block * 30 + 30):
        rows, gen = rotated_stack_loop_network(seed)
        kw = rotated_seed_kwargs(seed)
        xs = po.gen_inputs(seed + 5, 512, **gen)
        overflowing += bool(overflowed(po.OracleNet(rows).compute_batch(xs, **kw)[1]).any())
        cases.append((f"seed{seed}", rows, xs, kw))
    assert overflowing >= 4, overflowing  # of 30 seeds: the test is about lanes that overflow
    assert len(check_cases(tmp_path, cases, machine)) >= 24  # the others are tier 1's


def test_stack_loop_network_rows_are_pinned():
    # rotate= must not move what the seeded dynamic-stack tests have always
    # checked: the rows and input kinds of seeds 0..89 without it, by digest
    import hashlib

    rows = repr([stack_loop_network(s) for s in range(90)]).encode()
    assert hashlib.sha256(rows).hexdigest() == "c7bec21879c3f33f3cb32ee71035eee4e5d4111df6767554632db88fe89e8bf5"
    moved = sum(rotated_stack_loop_network(s)[0] != stack_loop_network(s)[0] for s in range(90))
    assert moved >= 45, moved  # and rotate=True does move the counter


# ---- deep static stacks (tisgen.deep_stack_network): spilled entries, shared slots

def test_deep_stack_network_rows_are_pinned():
    # the rows of seeds 0..59 in every form, by digest: the share / interfere
    # fractions below and the GPU tests' shape coverage are properties of
    # these programs
    import hashlib

    rows = repr([deep_stack_network(s, **kw) for kw in ({}, {"session": True}, {"big": True}) for s in range(60)])
    digest = hashlib.sha256(rows.encode()).hexdigest()
    assert digest == "df7ec14c93433940320bcdb30c8fb446602e0e5d680a58a8e48b3483f07a88bf"


def _deep_slots(rows, monkeypatch):
    """(slots with sharing on, slots with it off)"""
    monkeypatch.setenv("MK_SCHED_SHARE", "1")
    on = sc.jit_lane(rows)[1]
    monkeypatch.setenv("MK_SCHED_SHARE", "0")
    off = sc.jit_lane(rows)[1]
    monkeypatch.delenv("MK_SCHED_SHARE")
    return on, off


def test_deep_stack_networks_reach_the_placement_machinery(monkeypatch):
    # What the generator is for: every seed on the native tier with static
    # slots; at least a fifth of the seeds with stacks that share slots, and
    # at least a fifth with spilled stacks that may not (the same count
    # either way, and more slots than the deepest stack has entries: two or
    # more stacks spill); both stream kernels.  Seeds 0..59 measure 28 %
    # sharing and 53 % interfering.
    shared = interfering = 0
    shapes = set()
    for seed in range(60):
        rows = deep_stack_network(seed)
        tier, shape = sc.tier(rows)  # raises nothing, declines nothing
        assert tier == "native", (seed, tier, shape)
        shapes.add(shape)
        on, off = _deep_slots(rows, monkeypatch)
        assert on <= off < 1024, (seed, on, off)  # static: a dynamic stack takes the capacity
        shared += on < off
        interfering += on == off and off > max(deep_stack_peaks(seed).values())
    assert shared >= 12 and interfering >= 12, (shared, interfering)  # 20 % of 60
    assert {"stream", "stream-heavy"} <= shapes, shapes


def _deep_cases(seeds, n=60):
    """[(label, nodes, inputs, kwargs)]: the seeded inputs (every seventh 0)
    and 0, 1, -1, 2^31 - 1, so both arms of every branch run."""
    return [(f"deep{seed}", deep_stack_network(seed),
             np.concatenate([deep_stack_inputs(seed, n), np.asarray([0, 1, -1, 2**31 - 1], np.int64)]),
             deep_seed_kwargs(seed)) for seed in seeds]


def test_deep_stack_cases_end_every_way():
    # across the seed set the capacities and budgets of deep_seed_kwargs end
    # lanes by stack overflow and by budget, and leave others quiescent
    reasons = set()
    for _, nodes, xs, kw in _deep_cases(range(120)):
        st = po.OracleNet(nodes).compute_batch(xs, **kw)[1]
        reasons |= set((st & mk._native.MK_ST_REASON_MASK).tolist())
    assert {mk._native.MK_ST_STACK_OVERFLOW, mk._native.MK_ST_BUDGET, mk._native.MK_ST_QUIESCENT} <= reasons, reasons


# The generated lanes of seeds 0..119, stream and machine shape, with slot
# sharing on and off: a miscoloured pair of stacks, a rolled run whose slot
# expression is wrong after renumbering or a branch arm using a shared range
# for the other stack shows here as a wrong output.
@pytest.mark.parametrize("share", ["1", "0"])
@pytest.mark.parametrize("machine", [False, True])
@pytest.mark.parametrize("block", range(4))
def test_deep_stack_networks(tmp_path, monkeypatch, block, machine, share):
    monkeypatch.setenv("MK_SCHED_SHARE", share)
    cases = _deep_cases(range(block * 30, block * 30 + 30))
    assert len(check_cases(tmp_path, cases, machine)) == len(cases)  # none declined


# The spill thresholds the loader's register plans choose among
# (MK_SCHED_SOFT_REGS; tune_lds_auto and more_waves recompile with them).
@pytest.mark.parametrize("soft", [8, 16, 40, 64])
def test_deep_stack_networks_spill_thresholds(tmp_path, monkeypatch, soft):
    monkeypatch.setenv("MK_SCHED_SOFT_REGS", str(soft))
    cases = _deep_cases(range(40))
    assert len(check_cases(tmp_path, cases)) == len(cases)


def test_shapes():
    # acyclic schedules stream; data-dependent loops get the machine shape
    assert sc.jit_lane(mk.networks.example_network(), with_shape=True)[2] == "stream"
    assert sc.jit_lane(mk.networks.sample_network(), with_shape=True)[2] == "stream"
    src, _, shape = sc.jit_lane(mk.networks.countdown_network(), with_shape=True)
    assert shape == "machine" and "do {" in src


@pytest.mark.parametrize("which", ["countdown", "example", "sample"])
def test_module_compiles_for_gfx950(which):
    # hiprtc in-process, no GPU: the product library reports the native tier
    # for both shapes (machine: countdown; light stream: example, sample)
    net = mk.Network(getattr(mk.networks, f"{which}_network")())
    plan = net.plan(mode="jit")
    assert plan.startswith("tier=native "), plan
    src = net.jit_source()
    assert "mk_jit_exec" in src and "mk_lane" in src


# The machine shape of the deep pipelines (C4) used to hand hiprtc a 1.4 MB
# function whose checked variant had one early exit per round end (5,643 at
# D=64); it now looks the budget exit up after the body (tis_jit.cpp
# emit_budget_exit) and every C4 depth compiles well inside the bound, with
# the pipelined POP loops on.
COMPILE_BOUND_S = 60


@pytest.mark.parametrize("depth", [64, 256, 1024])
def test_machine_shape_pipeline_compiles_in_bound(depth, monkeypatch):
    monkeypatch.setenv("MK_JIT_SHAPE", "machine")
    net = mk.Network(mk.networks.pipeline_network(depth))
    plan = net.plan(mode="jit")
    assert plan.startswith("tier=native ") and "shape=machine" in plan, plan
    secs = float(plan.split("compile=")[1].split("s")[0])
    assert secs < COMPILE_BOUND_S, plan
    src = net.jit_source()
    assert len(src) < (1 << 20) and "mk_jit_exec" in src


def test_pipeline_stacks_share_slots(monkeypatch):
    # node k drains its stack before node k+1 pushes: the eight stacks share
    # one slot range (tis_sched.cpp share_slots); MK_SCHED_SHARE=0 gives each
    # its own.  D=64's shared range fits LDS: the heavy kernel keeps it there
    # (its default plan: round 6 also plans eight waves per SIMD, with 16
    # slots -- test_lds_occupancy_tunes_register_count).
    for depth, shared, own in ((64, 41, 328), (256, 233, 1864), (1024, 1001, 8008)):
        assert sc.jit_lane(mk.networks.pipeline_network(depth))[1] == shared
        monkeypatch.setenv("MK_SCHED_SHARE", "0")
        assert sc.jit_lane(mk.networks.pipeline_network(depth))[1] == own
        monkeypatch.delenv("MK_SCHED_SHARE")
    monkeypatch.setenv("MK_JIT_VGPR_FILE", "256")  # the eight-wave plan rejected: the default
    plan = mk.Network(mk.networks.pipeline_network(64)).plan(mode="jit")
    assert "slots=41 " in plan and "shape=stream-heavy-lds " in plan, plan
    monkeypatch.delenv("MK_JIT_VGPR_FILE")
    monkeypatch.setenv("MK_JIT_LDS_SLOTS", "0")
    plan = mk.Network(mk.networks.pipeline_network(64)).plan(mode="jit")
    assert "shape=stream-heavy " in plan, plan


def test_lds_occupancy_tunes_register_count(monkeypatch):
    # The loader's policy for heavy networks (mk_exec.hip tune_lds_auto):
    # D=64's 41 slots fit LDS at four waves per CU, yet eight per SIMD take
    # 49 registers (16 slots in a 5 KiB share, round 6); D=256
    # gets eight waves per SIMD (more_waves): 241 registers leave 16 slots,
    # all in a 5 KiB LDS share, and the compiled module holds eight waves
    # (its VGPRs are checked: stack_plans=w8:...); D=300 cannot reach eight
    # within 256 registers and gets two (80 slots in 20 KiB); D=400 reaches
    # neither and keeps 64 registers, four waves per CU, 160 of 337 slots in
    # LDS; D=1024 (961 slots at 64 registers) stays in HBM
    def fields(depth):
        plan = mk.Network(mk.networks.pipeline_network(depth)).plan(mode="jit")
        return dict(w.split("=", 1) for w in plan.split() if "=" in w)

    f = fields(64)  # round 6: eight waves per SIMD too (49 registers, 16 slots in a 5 KiB share)
    assert f["shape"] == "stream-heavy-lds" and f["regs"] == "49" and f["slots"] == "16", f
    assert f["stack_plans"].startswith("w8:") and "rejected" not in f["stack_plans"], f
    f = fields(256)
    assert f["shape"] == "stream-heavy-lds" and f["regs"] == "241" and f["slots"] == "16", f
    assert f["stack_plans"].startswith("w8:") and "rejected" not in f["stack_plans"], f
    assert f["waves_per_simd"] == "8" if "waves_per_simd" in f else True
    f = fields(300)
    assert f["shape"] == "stream-heavy-lds" and int(f["slots"]) <= 80 and f["stack_plans"].startswith("w2:"), f
    f = fields(400)
    assert f["shape"] == "stream-heavy-split" and f["regs"] == "64" and f["slots"] == "337", f
    f = fields(1024)
    assert f["shape"] == "stream-heavy" and f["regs"] == "64" and f["slots"] == "961", f
    # a fixed LDS budget (MK_JIT_LDS_SLOTS): registers for the most waves
    # with every slot in LDS -- D=256 reaches three (<= 208 slots of 256 B in
    # 2-KiB granules)
    monkeypatch.setenv("MK_JIT_LDS_SLOTS", "81920")
    f = fields(256)
    assert f["shape"] == "stream-heavy-lds" and int(f["slots"]) <= 208 and int(f["regs"]) > 24, f
    monkeypatch.setenv("MK_JIT_TUNE_REGS", "0")
    f = fields(256)
    assert f["slots"] == "233" and f["regs"] == "24", f


def test_stack_plan_rejection_falls_back(monkeypatch):
    # The plan-rejection path of jit_compile: a more_waves plan
    # whose module cannot hold its waves gives way to the next plan, and last
    # to the default.  MK_JIT_VGPR_FILE lowers the register file the check
    # prices against, so the path runs on purpose: at 256 VGPRs D=256's
    # eight-wave module (38 VGPRs x 8 = 304) is rejected and the two-wave
    # plan (80 slots in LDS) compiles and holds; at 128 both are rejected and
    # the default (64 registers, 160 of 193 slots in LDS) runs.
    def fields(depth, mode="jit"):
        plan = mk.Network(mk.networks.pipeline_network(depth)).plan(mode=mode)
        return dict(w.split("=", 1) for w in plan.split() if "=" in w)

    monkeypatch.setenv("MK_JIT_VGPR_FILE", "256")
    f = fields(256)
    assert f["stack_plans"].startswith("w8:") and f["stack_plans"].split(";")[0].endswith("-rejected"), f
    assert f["stack_plans"].split(";")[1].startswith("w2:") and "rejected" not in f["stack_plans"].split(";")[1], f
    assert int(f["slots"]) <= 80 and f["shape"] == "stream-heavy-lds", f
    monkeypatch.setenv("MK_JIT_VGPR_FILE", "128")
    f = fields(256)
    assert f["stack_plans"].count("-rejected") == 2, f
    assert f["regs"] == "64" and f["slots"] == "193" and f["shape"] == "stream-heavy-split", f
    f = fields(64)  # D=64's eight-wave plan rejected: the 24-register default (41 slots, 15 waves per CU)
    assert f["stack_plans"].endswith("-rejected") and f["regs"] == "24" and f["slots"] == "41", f
    # tier 2 keeps the default plan whichever plan the native tier runs: its
    # LDS register file would hold one block per CU at 241 registers
    monkeypatch.delenv("MK_JIT_VGPR_FILE")
    assert fields(256)["regs"] == "241"
    t2 = fields(256, mode="tile")
    assert t2["regs"] == "64" and t2["slots"] == "193" and t2["B"] == "64", t2


def test_compile_bounds_fall_back_with_reason(monkeypatch):
    # over the source bound: tier 2 runs it, mk_net_plan names the bound
    monkeypatch.setenv("MK_JIT_MAX_SRC", "1000")
    net = mk.Network(mk.networks.pipeline_network(64))
    plan = net.plan()
    assert plan.startswith("tier=compiled ") and "compile bound" in plan, plan
    assert mk.Network(mk.networks.pipeline_network(64)).plan(mode="jit").startswith("tier=none"), plan
    # over the time bound: the compile is abandoned, tier 2 runs it
    monkeypatch.delenv("MK_JIT_MAX_SRC")
    monkeypatch.setenv("MK_JIT_COMPILE_S", "0.001")
    # (one bound for all its stack plans' compiles together: the first one
    # abandoned, none is started for the next)
    plan = mk.Network(mk.networks.pipeline_network(256)).plan()
    assert plan.startswith("tier=compiled ") and "did not finish" in plan, plan
    assert "no time left for the next stack plan" in plan and "regs=64" in plan, plan


@pytest.mark.parametrize("cls", ["data_dependent_stack_depth", "two_stacks_independent_depths"])
@pytest.mark.parametrize("heavy", [False, True])
def test_dynamic_stack_module_compiles_for_gfx950(cls, heavy, monkeypatch):
    # the census classes whose stack depths follow the data run natively
    # (machine shape; forced stream + heavy: the buffer-op form of the
    # per-lane slot numbers, MK_SLOT_STX/LDX)
    if heavy:
        monkeypatch.setenv("MK_JIT_SHAPE", "stream")
        monkeypatch.setenv("MK_JIT_HEAVY_OPS", "1")
    net = mk.Network(mk.networks.census_classes()[cls][0][1])
    plan = net.plan(mode="jit")
    assert plan.startswith("tier=native "), plan
    src = net.jit_source()
    assert "MK_SLOT_STX" in src and "MK_SLOT_LDX" in src


def test_knobs_are_snapshotted_per_network(monkeypatch):
    # a network keeps the knobs of its load: plan, source and module agree
    monkeypatch.setenv("MK_JIT_SHAPE", "machine")
    net = mk.Network(mk.networks.example_network())
    monkeypatch.setenv("MK_JIT_SHAPE", "stream")
    assert "shape=machine" in net.plan(mode="jit")
    assert "#define MK_JIT_MACHINE 1" in net.jit_source()
    assert "knobs=shape=machine" in net.plan(mode="jit")


# The native tier's modules are code object v5 whichever hiprtc builds them
# (mk_rtc.cpp kCodeObjectVersion): ROCm 7.2's default v6 modules
# corrupted the host heap inside PyTorch's bundled HIP runtime (r03c-r03k).
# The module of a dynamic-stack network (the shape that showed it), dumped by
# MK_JIT_DUMP, read with llvm-readelf: ELF ABI version 3 = code object v5.
def test_modules_are_code_object_v5(tmp_path, monkeypatch):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not installed")
    rows, _ = stack_loop_network(6)  # two dynamic stacks, machine shape
    co = str(tmp_path / "m.co")
    monkeypatch.setenv("MK_JIT_DUMP", co)
    plan = mk.Network(rows).plan()
    assert plan.startswith("tier=native"), plan
    hdr = subprocess.run([readelf, "-h", co], capture_output=True, text=True, check=True).stdout
    assert any(l.split() == ["ABI", "Version:", "3"] for l in hdr.splitlines()), hdr


def _pop_chain_program(accum: str, depth: int, tail: str = "SWP\nOUT ACC") -> str:
    """One node: push x + 7k (k = 1..depth), then pop every value into an
    accumulator kept in BAK through `accum` (ACC holds the running value, R2
    the popped one), the loop counter in the node's own port R1."""
    return "\n".join([
        "IN ACC", "SAV", f"MOV {depth}, ACC",
        "L: SWP", "ADD 7", "PUSH ACC, s", "SWP", "SUB 1", "JGZ L",
        "MOV 0, ACC", "SAV", f"MOV {depth}, ACC", "MOV ACC, a:R1",
        "Q: POP s, ACC", "MOV ACC, a:R2", "SWP", accum, "SAV",
        "MOV R1, ACC", "SUB 1", "MOV ACC, a:R1", "JGZ Q",
        "MOV R1, NIL", tail, ""])


POP_CHAINS = {
    "mul3": "MOV ACC, a:R3\nADD ACC\nADD R3\nADD R2",      # C4's sum = 3 * sum + v
    "add": "ADD R2",                                       # sum + v
    "sub": "SUB R2",                                       # sum - v
    "mul2": "ADD ACC\nADD R2",                             # 2 * sum + v
    "mul4c": "ADD ACC\nADD ACC\nADD R2\nADD 5",            # 4 * sum + v + 5
    "neg": "NEG\nADD R2",                                  # v - sum
    "mul5": "MOV ACC, a:R3\nADD ACC\nADD ACC\nADD R3\nSUB R2",  # 5 * sum - v
}


@pytest.mark.parametrize("tail", ["out", "sign"])
def test_pop_chains(tmp_path, tail):
    """Pipelined pop runs (emit_prefetched_run) feeding linear accumulations,
    read through hops (narrow registers) or by a sign test (wide), bit-exact
    against the oracle on full-range inputs (INT32_MIN/MAX included)."""
    t = "SWP\nOUT ACC" if tail == "out" else "SWP\nJGZ P\nOUT 1\nJMP E\nP: OUT ACC\nE: NOP"
    cases = []
    for name, accum in POP_CHAINS.items():
        nodes = [NodeSpec("a", "program", _pop_chain_program(accum, 100, t)), NodeSpec("s", "stack", "")]
        cases.append((f"{name}-{tail}", nodes, po.gen_inputs(SEED, 300), {}))
    check_cases(tmp_path, cases)
