"""Seeded random TIS programs / networks for parity fuzzing.

Two generators:
  * ``random_network`` -- loadable networks exercising every instruction
    form, every source, edge immediates (int32/int64 bounds, Atoi range
    errors), ports, stacks, unknown hosts, wrong-service targets and the
    master name.  Used for oracle-vs-GPU bit-exact tests.
  * ``mutated_line`` -- text-level mutations of valid lines (whitespace
    classes incl. \\v and \\f, case, commas, signs, labels, comments) for
    parser accept/reject/error-text parity.

Further down: loop shapes of the native machine kernel, networks whose stack
depths follow the data (``stack_loop_network``) and deep static stacks
(``deep_stack_network``: spilled entries, shared and interfering slots); last,
the self-loop family (``self_loop_programs``: steps, exit tests, bodies and
chains around every form the native tier's loop generator can emit).
"""
from __future__ import annotations

import functools
import random

IMM_EDGES = [
    "0", "1", "-1", "2", "-2", "7", "100", "-100", "1000",
    "2147483647", "-2147483648", "2147483648", "-2147483649", "4294967296", "4294967301",
    "9223372036854775807", "-9223372036854775808",
    "9223372036854775808", "-9223372036854775809", "99999999999999999999",  # Atoi range errors
    "007", "-0",
]
SRCS = ["ACC", "NIL", "R0", "R1", "R2", "R3"]
REGS = ["R0", "R1", "R2", "R3"]


def rand_imm(r: random.Random) -> str:
    if r.random() < 0.6:
        return str(r.randint(-20, 20))
    return r.choice(IMM_EDGES)


def random_program(r: random.Random, progs, stacks, others, nlines=None, allow_in=True, allow_out=True):
    nlines = nlines or r.randint(1, 12)
    labels = [f"L{i}" for i in range(r.randint(0, 3))]
    label_lines = r.sample(range(nlines), min(len(labels), nlines))
    labels = labels[: len(label_lines)]
    lines = []
    for i in range(nlines):
        kind = r.random()
        targets_prog = progs + others
        targets_stack = stacks + others + progs[:1]
        if kind < 0.05:
            body = ""
        elif kind < 0.08:
            body = "# comment " + str(r.randint(0, 9))
        else:
            f = r.choice(
                ["NOP", "SWP", "SAV", "NEG", "MOVL", "MOVL", "MOVN", "MOVN", "ADD", "ADD", "SUB", "JMP", "JCC",
                 "JCC", "JRO", "PUSH", "POP", "IN", "OUT", "OUT"]
            )
            if f in ("NOP", "SWP", "SAV", "NEG"):
                body = f
            elif f == "MOVL":
                src = rand_imm(r) if r.random() < 0.4 else r.choice(SRCS)
                body = f"MOV {src}, {r.choice(['ACC', 'NIL'])}"
            elif f == "MOVN":
                src = rand_imm(r) if r.random() < 0.3 else r.choice(SRCS)
                body = f"MOV {src}, {r.choice(targets_prog)}:{r.choice(REGS)}"
            elif f in ("ADD", "SUB"):
                src = rand_imm(r) if r.random() < 0.5 else r.choice(SRCS)
                body = f"{f} {src}"
            elif f in ("JMP", "JCC"):
                if not labels:
                    body = "NOP"
                else:
                    op = "JMP" if f == "JMP" else r.choice(["JEZ", "JNZ", "JGZ", "JLZ"])
                    lab = r.choice(labels)
                    body = f"{op} {lab.lower() if r.random() < 0.2 else lab}"
            elif f == "JRO":
                src = str(r.randint(-4, 4)) if r.random() < 0.4 else (rand_imm(r) if r.random() < 0.2 else r.choice(SRCS))
                body = f"JRO {src}"
            elif f == "PUSH":
                src = rand_imm(r) if r.random() < 0.3 else r.choice(SRCS)
                body = f"PUSH {src}, {r.choice(targets_stack)}"
            elif f == "POP":
                body = f"POP {r.choice(targets_stack)}, {r.choice(['ACC', 'NIL'])}"
            elif f == "IN":
                body = f"IN {r.choice(['ACC', 'NIL'])}" if allow_in else "NOP"
            else:
                src = rand_imm(r) if r.random() < 0.3 else r.choice(SRCS)
                body = f"OUT {src}" if allow_out else "NOP"
        if i in label_lines:
            lab = labels[label_lines.index(i)]
            sep = r.choice([" ", "", "  ", "\t"])
            body = f"{lab}:{sep}{body}"
        if r.random() < 0.15:
            body = r.choice([" ", "\t", "  "]) + body
        lines.append(body)
    text = "\n".join(lines)
    if r.random() < 0.5:
        text += "\n"
    return text


def random_network(seed: int, max_prog=5, max_stack=3):
    """Returns a list of (name, kind, program) rows."""
    r = random.Random(seed)
    pool = ["a", "b", "c", "node1", "node2", "Z9", "x_y", "misaka1", "misaka2", "p", "q", "ACC", "R0"]
    r.shuffle(pool)
    nprog = r.randint(1, max_prog)
    nstack = r.randint(0, max_stack)
    progs = pool[:nprog]
    stacks = pool[nprog: nprog + nstack]
    master = "master" if r.random() < 0.5 else None
    others = ["ghost"] + ([master] if master else [])
    rows = []
    in_node = r.choice(progs)
    for p in progs:
        text = random_program(r, progs, stacks, others, allow_in=(p == in_node or r.random() < 0.3))
        rows.append((p, "program", text))
    for s in stacks:
        rows.append((s, "stack", ""))
    if master:
        rows.append((master, "master", ""))
    r.shuffle(rows)
    return rows


WS = [" ", "\t", "  ", "\f", "\r", "\v", ""]


def mutated_line(r: random.Random) -> str:
    base = r.choice(
        [
            "NOP", "SWP", "SAV", "NEG", "MOV 1, ACC", "MOV -5, NIL", "MOV 3, a:R0", "MOV ACC, a:R1",
            "MOV R2, ACC", "MOV R3, b:R3", "ADD 1", "SUB -2", "ADD ACC", "SUB R1", "JMP L", "JEZ l", "JNZ L",
            "JGZ M", "JLZ L", "JRO 2", "JRO -1", "JRO R0", "PUSH 5, s", "PUSH ACC, s", "POP s, ACC",
            "POP s, NIL", "IN ACC", "IN NIL", "OUT 1", "OUT ACC", "OUT R2", "L:", "L: NOP", "# c", "",
            "MOV ACC, ACC", "MOV NIL, NIL", "MOV 9223372036854775808, ACC",
        ]
    )
    ops = r.randint(0, 3)
    s = base
    for _ in range(ops):
        m = r.random()
        if m < 0.2 and " " in s:  # change a whitespace run
            i = s.index(" ")
            s = s[:i] + r.choice(WS) + s[i + 1:]
        elif m < 0.3 and ", " in s:
            s = s.replace(", ", r.choice([",", " ,", " , ", ",\t", ",  ", ",\v"]), 1)
        elif m < 0.4:
            s = s.lower() if r.random() < 0.5 else s.capitalize()
        elif m < 0.5:
            s = r.choice(WS) + s
        elif m < 0.6:
            s = s + r.choice(WS + ["#", " # c", "x", ","])
        elif m < 0.7:
            s = r.choice(["L:", "L: ", "l:", "  L:\t", "M:", "1:", "_:"]) + s
        elif m < 0.8:
            s = s.replace("1", r.choice(["+1", "--1", "1a", "01", "- 1", "1 2"]), 1)
        elif m < 0.9:
            s = s.replace("R", r.choice(["R", "r", "R4", "RR"]), 1)
        else:
            s = s.replace("a:", r.choice(["a :", "a: ", ":", "a::", "a-b:"]), 1)
    return s


def mutated_program(seed: int) -> str:
    r = random.Random(seed)
    lines = [mutated_line(r) for _ in range(r.randint(1, 6))]
    if r.random() < 0.3:
        lines.append("L:")
    return "\n".join(lines)


# ---- self-loop shapes of the native machine kernel -----------------------------
# Each targets one path of the generated loop (tis_jit.cpp emit_self_loop):
# the 32-bit induction phase and its range check (values near +-2^30, steps
# of 1 and of ~2^30), the 64-bit phase (int64 wrap), loops with no induction
# register (step counter), JMP-only loops that only the budget ends, and
# budgets that end inside a loop (guarded phase).
def _edge_inputs(rng: random.Random, n: int, lo: int, hi: int) -> list:
    edges = [0, 1, -1, 2**30, -(2**30), 2**30 + 1, -(2**30) - 1, 2**31 - 1, -(2**31), 2**31 - 2, -(2**31) + 1]
    return [rng.choice(edges) if rng.random() < 0.2 else rng.randint(lo, hi) for _ in range(n)]


def loop_cases(n: int = 512, seed: int = 7):
    """[(label, nodes, inputs, kwargs)] for the oracle-vs-native loop tests."""
    rng = random.Random(seed)
    P = lambda text: [("n", "program", text)]  # noqa: E731
    return [
        ("up_by_1", P("IN ACC\nL: ADD 1\nJLZ L\nOUT ACC"), _edge_inputs(rng, n, -3000, 50), {}),
        ("up_by_1_budget", P("IN ACC\nL: ADD 1\nJLZ L\nOUT ACC"), _edge_inputs(rng, n, -3000, 50),
         {"budget": 2500}),
        ("down_by_7", P("IN ACC\nL: SUB 7\nJGZ L\nOUT ACC"), _edge_inputs(rng, n, -50, 20000), {"budget": 5000}),
        ("down_by_2pow30", P("IN ACC\nL: SUB 1073741823\nJGZ L\nOUT ACC"), _edge_inputs(rng, n, -5, 2**31 - 1), {}),
        ("swap_loop", P("IN ACC\nSAV\nL: SWP\nADD 1\nSWP\nSUB 1\nJGZ L\nSWP\nOUT ACC"),
         _edge_inputs(rng, n, -5, 900), {"budget": 6000}),
        ("jmp_forever", P("IN ACC\nL: ADD 3\nJMP L"), _edge_inputs(rng, n, -100, 100), {"budget": 999}),
        ("int64_wrap", P("IN ACC\nADD 9223372036854775000\nL: ADD 100\nJGZ L\nOUT ACC"),
         _edge_inputs(rng, n, -2000, 2000), {}),
        ("two_loops", [("a", "program", "IN ACC\nL: SUB 1\nJGZ L\nMOV 500, ACC\nM: SUB 2\nJGZ M\nOUT ACC")],
         _edge_inputs(rng, n, -10, 3000), {}),
        ("down_nz", P("IN ACC\nL: SUB 1\nJNZ L\nOUT ACC"), _edge_inputs(rng, n, -20, 2000), {"budget": 3000}),
        ("up_to_zero_jez", P("IN ACC\nL: ADD 2\nJEZ E\nJMP L\nE: OUT ACC"), _edge_inputs(rng, n, -2000, 20),
         {"budget": 3000}),
        ("doubling", P("IN ACC\nL: ADD ACC\nJGZ L\nOUT ACC"), _edge_inputs(rng, n, -5, 2**31 - 1), {}),
        ("neg_sub", P("IN ACC\nL: NEG\nSUB 1\nJLZ L\nOUT ACC"), _edge_inputs(rng, n, -99, 99), {"budget": 777}),
        ("loop_with_stack", [("a", "program", "IN ACC\nL: PUSH ACC, s\nSUB 1\nJGZ L\nPOP s, ACC\nOUT ACC"),
                             ("s", "stack", "")], _edge_inputs(rng, n, -3, 40), {"stack_cap": 64}),
    ]


# ---- census classes: network shapes that stress the schedule compiler -----------
from misaka_net_amd.networks import census_classes  # noqa: E402,F401  (defined with the bench workloads)


def stack_loop_network(seed: int, rotate: bool = False):
    """Networks whose stack depths follow the data (the schedule compiler's
    dynamic stacks): loops with input-dependent trip counts that push and pop
    on 1-3 stacks, pops that may outnumber pushes (the POP then blocks), a
    second node popping what the first pushes (cross-node blocking), and
    values that reach the output (sums of popped values).  Returns
    (rows, gen kwargs for oracle.gen_inputs).

    ``rotate``: the counter's ``SUB step`` lands at a random place among the
    body's pushes and pops -- first, in the middle or last -- instead of
    always last, so loops count before they push (the native tier's induction
    register is then bumped ahead of a capacity exit).  Without it the rows
    of a seed are the ones they always were
    (test_jit_codegen.py test_stack_loop_network_rows_are_pinned)."""
    r = random.Random(seed)
    ns = r.randint(1, 3)
    stacks = [f"s{k}" for k in range(ns)]
    lines = ["IN ACC"]
    if r.random() < 0.5:
        lines.append(f"ADD {r.randint(-3, 3)}")
    lines.append("SAV")
    consumer = r.random() < 0.35
    for k in range(r.randint(1, 3)):
        s = r.choice(stacks)
        lab = f"L{k}"
        body = []  # groups of lines; ACC is the counter between groups
        for _ in range(r.randint(1, 3)):
            c = r.random()
            if c < 0.45:
                body.append([f"PUSH ACC, {r.choice(stacks)}"])
            elif c < 0.6:
                body.append([f"PUSH {r.randint(-5, 5)}, {r.choice(stacks)}"])
            elif c < 0.8 and not consumer:
                body.append([f"POP {r.choice(stacks)}, NIL"])
            else:
                # accumulate a popped value into BAK (ACC is the counter)
                body.append(["SWP", f"PUSH ACC, {s}", f"POP {r.choice(stacks)}, ACC", "SWP"])
        step = r.choice([1, 1, 2, 3])
        jump = r.choice(["JGZ", "JGZ", "JNZ"]) if step == 1 else "JGZ"
        at = len(body)
        if rotate:
            at = r.choice([0, len(body) // 2, len(body)])  # first, middle, last
        body.insert(at, [f"SUB {step}"])
        flat = [ln for grp in body for ln in grp]
        lines += [f"{lab}: " + flat[0]] + flat[1:] + [f"{jump} {lab}"]
        if r.random() < 0.5:
            lines += ["SWP", "SAV"]  # the next loop counts from the running value
    if consumer:
        lines += [f"PUSH -1, {stacks[0]}", "MOV R0, ACC", "OUT ACC"]
        cons = (f"MOV 0, ACC\nSAV\nC: POP {stacks[0]}, ACC\nJLZ E\nSWP\nADD 1\nSWP\nJMP C\n"
                f"E: SWP\nMOV ACC, a:R0")
        rows = [("a", "program", "\n".join(lines)), ("b", "program", cons)]
    else:
        tail = r.choice(["SWP\nOUT ACC", "OUT ACC", f"POP {stacks[-1]}, ACC\nOUT ACC", "MOV 9, ACC\nOUT ACC"])
        rows = [("a", "program", "\n".join(lines) + "\n" + tail)]
    rows += [(s, "stack", "") for s in stacks]
    r.shuffle(rows)
    return rows, dict(kind=1, mask=r.choice([15, 63, 255]))


# ---- deep static stacks: constant trip counts, spilled entries, shared slots ------
# Run lengths and depths around every threshold of the placement machinery:
# the register-resident entries (24), the pipelined POP loop (64 pops, tails
# of reps % 2) and, with big=True, slot counts past a two-wave LDS share.
DEEP_DEPTHS = (3, 23, 24, 25, 40, 63, 64, 65, 95, 96, 97, 130)
DEEP_BIG_DEPTHS = (160, 200)
DEEP_WIDE = ("2147483647", "-2147483648", "4294967301", "1073741824")


class _DeepGen:
    """One node's program text.  The running value lives in BAK, the loop
    counter in ACC; ``hi`` / ``lo`` bound each stack's depth over every path
    to here (they differ only behind a branch whose arms end at different
    depths)."""

    def __init__(self, r, me, stacks, limit, depths):
        self.r, self.me, self.limit, self.depths = r, me, limit, depths
        self.lines, self.nlab = [], 0
        self.hi = {s: 0 for s in stacks}
        self.lo = dict(self.hi)
        self.peak = dict(self.hi)

    def label(self):
        self.nlab += 1
        return f"T{self.nlab}"

    def push(self, s, d=None):
        r = self.r
        room = self.limit - self.hi[s]
        fits = [x for x in self.depths if x <= room]
        if d is None:
            if not fits:
                return False
            d = r.choice(fits + [x for x in fits if x >= 40])  # spilling depths twice as often
        t = self.label()
        c = r.random()
        # wide steps: the pushed values truncate to int32, a POP must sign-extend
        k = r.choice(DEEP_WIDE) if 0.2 <= c < 0.45 else str(r.choice([1, 1, 3, 7, -2, -11]))
        src = "ACC"
        if c < 0.2:  # U_STI (the running value still moves: a loop of constants alone would be generalised)
            src = r.choice(["-1", "5", "2147483647", "-2147483648", str(r.randint(-99, 99))])
        self.lines += [f"MOV {d}, ACC", f"{t}: SWP", f"ADD {k}", f"PUSH {src}, {s}", "SWP", "SUB 1", f"JGZ {t}"]
        self.hi[s] += d
        self.lo[s] += d
        self.peak[s] = max(self.peak[s], self.hi[s])
        return True

    def pop(self, s, d=None, nil=None):
        """run = 3 * run + popped (odd multiplier: every popped value, in its
        order, stays in the low 32 bits -- networks.pipeline_program); no
        store in the loop, so it may become the pipelined POP loop."""
        r = self.r
        if self.lo[s] == 0:
            return False
        if d is None:
            d = self.lo[s] if r.random() < 0.6 else r.randint(1, self.lo[s])
        if nil is None:
            nil = r.random() < 0.15
        t, me = self.label(), self.me
        if nil:
            self.lines += [f"MOV {d}, ACC", f"{t}: SWP", "ADD 1", f"POP {s}, NIL", "SWP", "SUB 1", f"JGZ {t}"]
        else:
            self.lines += [f"MOV {d}, ACC", f"{t}: SWP", f"MOV ACC, {me}:R3", f"POP {s}, ACC", f"MOV ACC, {me}:R2",
                           "MOV R3, ACC", f"MOV ACC, {me}:R3", "ADD ACC", "ADD R3", "ADD R2", "SWP", "SUB 1",
                           f"JGZ {t}"]
        self.hi[s] -= d
        self.lo[s] -= d
        return True

    def block(self, stacks):
        """2-3 runs: one stack filled and drained (sequential), or random
        pushes and pops over ``stacks`` (nested, interleaved, half-drained)."""
        r = self.r
        if r.random() < 0.35:
            s = r.choice(stacks)
            if self.push(s):
                self.pop(s, d=self.lo[s] if r.random() < 0.7 else None)
            return
        for _ in range(r.randint(2, 3)):
            s = r.choice(stacks)
            if self.lo[s] == 0 or r.random() < 0.45:
                if not self.push(s):
                    self.pop(s)
            else:
                self.pop(s)

    def branch(self, stacks, level):
        """A branch on the input (stashed in the node's own R1): the arms use
        the stacks in different orders and to different depths.  ``level``:
        both arms pop down to common depths before they join."""
        r = self.r
        a1, j = self.label(), self.label()
        self.lines += ["MOV R1, ACC", f"{r.choice(['JGZ', 'JLZ', 'JEZ'])} {a1}"]
        hi0, lo0 = dict(self.hi), dict(self.lo)
        order = list(stacks)
        r.shuffle(order)
        ends = []
        for arm in range(2):
            self.hi, self.lo = dict(hi0), dict(lo0)
            if arm:
                self.lines += [f"JMP {j}", f"{a1}: NOP"]
                order = order[::-1]
            for s in order[:r.randint(1, len(order))]:
                if self.lo[s] and r.random() < 0.4:
                    self.pop(s)
                elif self.push(s) and r.random() < 0.5:
                    self.pop(s)
            ends.append((len(self.lines), dict(self.hi)))
        if level:
            low = {s: min(e[1][s] for e in ends) for s in self.hi}
            tail = self.lines[ends[0][0]:]
            del self.lines[ends[0][0]:]
            for e, rest in ((ends[0], tail), (ends[1], [])):
                self.hi, self.lo = dict(e[1]), dict(e[1])
                for s in stacks:
                    if self.hi[s] > low[s]:
                        self.pop(s, d=self.hi[s] - low[s])
                self.lines += rest
            self.hi, self.lo = dict(low), dict(low)
        else:
            self.hi = {s: max(e[1][s] for e in ends) for s in hi0}
            self.lo = {s: min(e[1][s] for e in ends) for s in hi0}
        self.lines.append(f"{j}: NOP")


def _deep_stack(seed: int, session: bool, big: bool):
    """(rows, deepest depth of each stack) of deep_stack_network."""
    r = random.Random(0x5EED0000 + 4 * seed + 2 * bool(session) + bool(big))
    ns = r.randint(3, 4) if big else r.randint(2, 4)
    stacks = [f"s{k}" for k in range(ns)]
    depths = DEEP_DEPTHS + (DEEP_BIG_DEPTHS if big else ())
    g = _DeepGen(r, "a", stacks, 200 if big else 130, depths)
    two = not session and r.random() < 0.34
    branch = r.random() < 0.5
    nseg = r.randint(2, 3) if session else 1
    branch_seg = r.randrange(nseg) if branch else -1
    rows = []
    for seg in range(nseg):
        g.lines += ["IN ACC", "SAV"]
        if seg == branch_seg:
            g.lines.append("MOV ACC, a:R1")  # the input, for the branch
        mine = stacks
        if two:
            d0 = r.choice([x for x in depths if x >= 24])
            g.push("s0", d=d0)
            g.lines += ["SWP", "MOV ACC, b:R0", "SWP"]
            b = _DeepGen(r, "b", ["s0", "t0"], g.limit, depths)
            b.lines += ["MOV R0, ACC", "SAV"]
            b.lo["s0"] = b.hi["s0"] = d0
            b.pop("s0", nil=False)
            if r.random() < 0.5:
                b.push("t0")
                b.pop("t0", d=b.lo["t0"], nil=False)
                rows.append(("t0", "stack", ""))
            b.lines += ["SWP", "MOV ACC, a:R0"]
            g.peak["t0"] = b.peak["t0"]
            rows.append(("b", "program", "\n".join(b.lines)))
            g.lo["s0"] = g.hi["s0"] = b.lo["s0"]
            mine = stacks[1:]
        for _ in range(r.randint(1, 2) if session or two else r.randint(1, 3)):
            g.block(mine)
        if two:  # b's fold joins the running value
            g.lines += ["SWP", "ADD R0", "SAV"]
        if seg == branch_seg:
            g.branch(stacks, level=session)
        for _ in range(r.randint(1, 2)):
            g.block(stacks)
        last = seg == nseg - 1
        for s in stacks:
            if g.lo[s] and (session and last or not session and r.random() < 0.5):
                g.pop(s, d=g.lo[s], nil=False if session else None)
        g.lines += ["SWP", "OUT ACC"]
    rows.append(("a", "program", "\n".join(g.lines)))
    rows += [(s, "stack", "") for s in stacks]
    r.shuffle(rows)
    names = {row[0] for row in rows}
    return rows, {s: d for s, d in g.peak.items() if s in names}


def deep_stack_network(seed: int, *, session: bool = False, big: bool = False):
    """Networks whose stack depths the schedule compiler knows (every trip
    count is a constant), deep enough to spill to numbered slots: 2-4 stacks,
    push runs (PUSH ACC with small and wide steps, PUSH imm) and pop runs
    (folded in order, to NIL, partial) of lengths around every threshold
    (DEEP_DEPTHS), in blocks that use the stacks one after the other, nested,
    interleaved and half-drained, so that some stacks may share slots and
    others interfere; about half the seeds branch on the input (JGZ / JLZ /
    JEZ) into arms that use the stacks in different orders and to different
    depths, and stacks may stay non-empty.  About a third are two nodes: ``a``
    fills s0 and signals ``b``, which pops it (and may use a stack of its
    own) while ``a`` works on other stacks, then hands its fold back and ends
    blocked on a read.

    ``session``: one node cut into 2-3 calls by ``SWP / OUT ACC / IN ACC /
    SAV``; stacks may stay filled across a call, and every stack is drained
    before the program wraps.  ``big``: depths up to 200.

    Returns the rows.  Seeds 0..59 are pinned by digest
    (test_jit_codegen.py test_deep_stack_network_rows_are_pinned)."""
    return _deep_stack(seed, session, big)[0]


def deep_stack_peaks(seed: int, *, session: bool = False, big: bool = False) -> dict:
    """{stack: its deepest depth on any path} of deep_stack_network(seed)."""
    return _deep_stack(seed, session, big)[1]


def deep_seed_kwargs(seed: int) -> dict:
    """Budget and capacity of a seeded deep-stack case: budgets that end lanes
    inside runs, capacities at and around the register-resident entries."""
    kw = dict(budget=[None, 300, 1000, 2500][seed % 4], stack_cap=[None, 24, 64, 100][seed // 4 % 4])
    return {k: v for k, v in kw.items() if v is not None}


def deep_stack_inputs(seed: int, n: int = 613):
    """gen_inputs(seed + 5, n) with every seventh input 0: each wave mixes the
    three sign classes of the branch."""
    from oracle import pyoracle as po

    xs = po.gen_inputs(seed + 5, n)
    xs[::7] = 0
    return xs


# ---- stack loops that count before they push ----------------------------------
# The native tier reads a lane's trip count off an induction register
# (tis_jit.cpp emit_self_loop).  A loop whose counter bump comes before a PUSH
# that can overflow has taken the bump when the capacity exit drops the lane:
# only bumps after the last exit count iterations completed.  Every program
# here comes in two orders -- "rot" (the counter first) and "ctl" (the
# counter last, what loop_cases and stack_loop_network emit).
ROT_CAPS = (3, 8, 16, 17, 33, 64, 65, 200)  # around every unguarded chunk size (4..32, and twice that)
ROT_BUDGETS = (None, 57, 300, 1000)         # none, inside the guarded part, inside the unguarded part


def _rot_programs():
    S = ("s", "stack", "")
    T = ("t", "stack", "")
    one = lambda text, *st: [("a", "program", text)] + list(st)  # noqa: E731
    fill = "IN ACC\nSAV\nF: PUSH ACC, s\nSUB 1\nJGZ F\nSWP\n"
    pusher = ("b", "program", "M: MOV R0, ACC\nPUSH ACC, s\nJMP M")
    return [
        ("sub_push", "rot", one("IN ACC\nL: SUB 1\nPUSH ACC, s\nJGZ L\nPOP s, ACC\nOUT ACC", S)),
        ("sub_push", "ctl", one("IN ACC\nL: PUSH ACC, s\nSUB 1\nJGZ L\nPOP s, ACC\nOUT ACC", S)),
        ("add2_push_jlz", "rot", one("IN ACC\nL: ADD 2\nPUSH ACC, s\nJLZ L\nPOP s, ACC\nOUT ACC", S)),
        ("add2_push_jlz", "ctl", one("IN ACC\nL: PUSH ACC, s\nADD 2\nJLZ L\nPOP s, ACC\nOUT ACC", S)),
        ("sub_push_push", "rot", one("IN ACC\nL: SUB 1\nPUSH ACC, s\nPUSH 3, s\nJGZ L\nPOP s, ACC\nOUT ACC", S)),
        ("sub_push_push", "ctl", one("IN ACC\nL: PUSH ACC, s\nPUSH 3, s\nSUB 1\nJGZ L\nPOP s, ACC\nOUT ACC", S)),
        # two registers bumped ahead of the PUSH: the counter and, in BAK, the value pushed
        ("swp_counter", "rot", one("IN ACC\nSAV\nL: SUB 1\nSWP\nADD 1\nPUSH ACC, s\nSWP\nJGZ L\nSWP\nOUT ACC", S)),
        ("swp_counter", "ctl", one("IN ACC\nSAV\nL: SWP\nADD 1\nPUSH ACC, s\nSWP\nSUB 1\nJGZ L\nSWP\nOUT ACC", S)),
        # a POP loop (the empty-check exit) behind a fill loop that overflows
        ("fill_pop", "rot", one(fill + "L: SUB 1\nPOP s, NIL\nJGZ L\nOUT ACC", S)),
        ("fill_pop", "ctl", one(fill + "L: POP s, NIL\nSUB 1\nJGZ L\nOUT ACC", S)),
        # the counter in node a, the PUSH in node b
        ("two_nodes", "rot", [("a", "program", "IN ACC\nL: SUB 1\nMOV ACC, b:R0\nJGZ L\nOUT ACC"), pusher, S]),
        ("two_nodes", "ctl", [("a", "program", "IN ACC\nL: MOV ACC, b:R0\nSUB 1\nJGZ L\nOUT ACC"), pusher, S]),
        # two stacks, the second three entries ahead: it overflows first, after
        # the first one's depth register took its bump
        ("two_stacks", "rot", one("IN ACC\nPUSH 1, t\nPUSH 1, t\nPUSH 1, t\nL: SUB 1\nPUSH ACC, s\nPUSH ACC, t\nJGZ L\n"
                                  "POP s, ACC\nOUT ACC", S, T)),
        ("two_stacks", "ctl", one("IN ACC\nPUSH 1, t\nPUSH 1, t\nPUSH 1, t\nL: PUSH ACC, s\nPUSH ACC, t\nSUB 1\nJGZ L\n"
                                  "POP s, ACC\nOUT ACC", S, T)),
    ]


def rotated_stack_inputs(n: int | None = None, seed: int = 11):
    """-5..259 dense, +-1000 and the _edge_inputs edges: with ROT_CAPS every
    wave mixes lanes that overflow, lanes that leave by the branch and lanes
    that never enter the loop.  ``n``: that many lanes, every value present,
    in a seeded shuffle."""
    edges = [0, 1, -1, 2**30, -(2**30), 2**30 + 1, -(2**30) - 1, 2**31 - 1, -(2**31), 2**31 - 2, -(2**31) + 1]
    xs = list(range(-5, 260)) + [1000, -1000] + edges
    if n is not None:
        assert n >= len(xs)
        xs = (xs * (n // len(xs) + 1))[:n]
        random.Random(seed).shuffle(xs)
    return xs


def rotated_stack_loop_programs():
    """[(name, nodes)]: name is '<program>-rot' or '<program>-ctl'."""
    return [(f"{name}-{order}", nodes) for name, order, nodes in _rot_programs()]


def rotated_stack_loop_cases(n: int | None = None, caps=ROT_CAPS, budgets=ROT_BUDGETS):
    """[(label, nodes, inputs, kwargs)] like loop_cases: every program of
    rotated_stack_loop_programs at every capacity and budget; the label is
    '<program>-<order>/cap<capacity>/b<budget>'."""
    xs = rotated_stack_inputs(n)
    cases = []
    for name, nodes in rotated_stack_loop_programs():
        for cap in caps:
            for budget in budgets:
                kw = {"stack_cap": cap}
                if budget is not None:
                    kw["budget"] = budget
                cases.append((f"{name}/cap{cap}/b{budget}", nodes, xs, kw))
    return cases


def rotated_stack_loop_network(seed: int):
    """stack_loop_network with the counter bump at a random place in each
    loop's body, and inputs 0..255 whatever mask the seed drew: trip counts
    then pass every capacity of rotated_seed_kwargs."""
    rows, gen = stack_loop_network(seed, rotate=True)
    return rows, dict(gen, mask=255)


def rotated_seed_kwargs(seed: int) -> dict:
    """Capacity and budget of a seeded rotated network: the rotation of the
    seeded dynamic-stack tests, with capacity 33 (just past the largest
    unguarded chunk) added."""
    kw = dict(budget=[None, 57, 300, 2000][seed % 4], stack_cap=[None, 3, 17, 33, 64, 200][seed % 6])
    return {k: v for k, v in kw.items() if v is not None}


# ---- the self-loop family: steps, exit tests, bodies and chains ----------------
# emit_self_loop (tis_jit.cpp) picks the form of a data-dependent loop from its
# step, its exit test and its body.  Every row here names the form it is meant
# to reach (test_jit_codegen.py test_self_loop_forms_are_pinned reads the form
# back from the emitted lane):
#
#   "<phase>/<trip count>"   phase: satdown (step -1, JGZ: saturating countdown),
#       counter (JGZ with step <= -2, JLZ with step >= 1: z0 = ceil(|x1| / k)),
#       pm1 / mad24 (int-flag loop, the bump x +- f or MK_MAD24), narrow (the
#       generic 32-bit phase); trip count: shift (the step a power of two) or
#       inverse (a multiply by the inverse of its odd part)
#   "k"                      no induction register: the per-lane counter
#
# a chain's form is its loops' forms, sorted, joined by "+".
SELF_LOOP_STEPS = (1, 2, 3, 5, 6, 12, 48, 255, 8388607, 8388608, 8388609, 1073741823, 1073741824, 1073741825,
                   2147483647, 2147483648, 4294967296)
# "JGZ": `Jcc L` at the loop's bottom; "iJGZ": `Jcc E / JMP L / E:`
SELF_LOOP_EXITS = ("JGZ", "JLZ", "JNZ", "JEZ", "iJGZ", "iJLZ", "iJNZ", "iJEZ")
# the sign of the bump under which the exit test can end a long loop ("" never:
# the loop stays only while the register is 0)
_ENDS = {"JGZ": "-", "iJLZ": "-", "JLZ": "+", "iJGZ": "+", "JNZ": "+-", "iJEZ": "+-", "JEZ": "", "iJNZ": ""}
SELF_LOOP_BODIES = ("bump", "bak", "twice", "neg", "other", "addacc")
# unguarded iterations per exit test (tis_jit.cpp fast_unroll of the body's
# micro-ops; SWP is a renaming, NEG and ADD ACC are not bumps)
_BODY_UF = {"bump": 32, "bak": 32, "twice": 32, "neg": 16, "other": 32, "addacc": 16}
_BIG = 2**30 - 1   # from this step on the input is scaled by 512 ahead of the loop: 64 trips need |x| > 2^31
_SCALE = 9         # `ADD ACC` lines of that prelude
# steps of the rows that cannot leave by the branch late (below): a sample, not the product
_FEW = (1, 255, 8388607, 1073741824)


def _body_lines(body: str, s: int) -> list:
    """The loop body for the signed step ``s``."""
    bump = f"ADD {s}" if s > 0 else f"SUB {-s}"
    back = f"SUB {s}" if s > 0 else f"ADD {-s}"
    return {
        "bump": [bump],
        "bak": [bump, "SWP", "ADD 3", "SWP"],        # work on BAK beside the counter: the generic narrow phase
        "twice": [bump, bump],                       # the register written twice: no induction register
        "neg": ["NEG", back, "NEG"],                 # -(-x - s) = x + s
        "other": ["SWP", bump, "SWP"],               # the counter in BAK, the exit test on ACC
        "addacc": ["ADD ACC", bump],                 # 2 x + s: no constant bump at all
    }[body]


def _loop_lines(lab: str, body: list, exit_: str) -> list:
    """One loop; a line that starts with ':' carries the label of whatever follows."""
    lines = [f"{lab}: {body[0]}"] + body[1:]
    if exit_.startswith("i"):
        return lines + [f"{exit_[1:]} E{lab}", f"JMP {lab}", f":E{lab}"]
    return lines + [f"{exit_} {lab}"]


def _join(lines: list) -> str:
    out, pend = [], ""
    for ln in lines:
        if ln.startswith(":"):
            pend = ln[1:] + ": "
        else:
            out.append(pend + ln)
            pend = ""
    assert not pend
    return "\n".join(out)


def _loop_form(body: str, s: int, exit_: str) -> str:
    """The form emit_self_loop is meant to pick (the rules of int_flag_fn and
    of the induction register, restated)."""
    ad = abs(s)
    if body in ("twice", "neg", "addacc"):
        return "k"
    if ad >= 2**31:  # no induction register on the counter; `bak` still has BAK's += 3
        return "narrow/inverse" if body == "bak" else "k"
    trip = "shift" if ad & (ad - 1) == 0 else "inverse"
    flag = {"JGZ": "GT", "JLZ": "LT", "JNZ": "NZ", "iJEZ": "NZ"}.get(exit_)
    if body != "bump" or ad >= 2**23 or flag is None:
        return f"narrow/{trip}"
    if s == -1 and flag == "GT":
        return f"satdown/{trip}"
    if (flag == "GT" and s <= -2) or (flag == "LT" and s >= 1):
        return f"counter/{trip}"
    return f"{'pm1' if ad == 1 else 'mad24'}/{trip}"


def _single(body: str, s: int, exit_: str):
    big = abs(s) >= _BIG
    pre = ["IN ACC"] + ["ADD ACC"] * (_SCALE if big else 0) + (["SAV"] if body in ("bak", "other") else [])
    blines = _body_lines(body, s)
    tail = {"bak": ["MOV ACC, n:R0", "SWP", "ADD R0", "OUT ACC"], "other": ["SWP", "OUT ACC"]}.get(body, ["OUT ACC"])
    label = f"{body}/{'+' if s > 0 else '-'}{abs(s)}/{exit_}"
    eff = 2 * s if body == "twice" else s
    meta = dict(uf=_BODY_UF[body], inc=len(blines) + (2 if exit_.startswith("i") else 1), prelude=len(pre),
                mult=2**_SCALE if big else 1, step=eff, head=_join(pre + ["OUT ACC"]),
                late=("+" if s > 0 else "-") in _ENDS[exit_] and body not in ("other", "addacc"),
                # leaving at the first test of a != 0 loop takes x = the step: 512 times the input is never an odd one
                first=not (big and eff % 2**_SCALE and exit_ in ("JNZ", "iJEZ")), nloops=1)
    text = _join(pre + _loop_lines("L", blines, exit_) + tail)
    return label, [("n", "program", text)], _loop_form(body, s, exit_), meta


def _chains():
    """A prelude whose step count follows the input (6, 8 or 9 steps), then
    two or three loops of different forms: the lanes of a wave reach the later
    loops with different step counts, and the unguarded iterations T follow
    the wave's largest.  The last loop is the one the budgets are aimed at."""
    pre = ["IN ACC", "SAV", "JGZ P", "NOP", "NOP", "NOP", ":P", "JLZ Q", "NOP", ":Q", "NOP"]
    rows = []

    def chain(name, loops, step):
        # loops: [(lines between the loops, body, step, exit)]
        lines, forms = list(pre), []
        for k, (between, body, s, exit_) in enumerate(loops):
            lines += between
            if k == len(loops) - 1:
                head = _join(lines + ["OUT ACC"])
            lines += _loop_lines(f"L{k}", _body_lines(body, s), exit_)
            forms.append(_loop_form(body, s, exit_))
        body, s, exit_ = loops[-1][1:]
        meta = dict(uf=_BODY_UF[body], inc=len(_body_lines(body, s)) + (2 if exit_.startswith("i") else 1),
                    prelude=6, mult=1, step=step, head=head, late=True, first=True, nloops=len(loops))
        rows.append((f"chain/{name}", [("n", "program", _join(lines + ["OUT ACC"]))], "+".join(sorted(forms)), meta))

    again = ["SWP", "SAV"]  # ACC = the input again (BAK keeps it)
    chain("down1-up6-nz7", [([], "bump", -1, "JGZ"), (again, "bump", 6, "JLZ"), (again, "bump", -7, "JNZ")], 7)
    chain("up1-down3", [([], "bump", 1, "JLZ"), (again, "bump", -3, "JGZ")], 3)
    chain("nz1-bak5", [([], "bump", -1, "JNZ"), (again, "bak", -5, "JGZ")], 5)
    chain("twice2-inv12", [([], "twice", -2, "JGZ"), (again, "bump", 12, "iJGZ")], 12)
    chain("down1-const-down2", [([], "bump", -1, "JGZ"), (["MOV 100, ACC"], "bump", -2, "JGZ"),
                                (again, "bump", -1, "iJLZ")], 1)
    chain("down255-neg48", [([], "bump", -255, "JGZ"), (again, "neg", 48, "JLZ")], 48)
    chain("wide-down1", [([], "bump", 2**30 + 1, "JLZ"), (again, "bump", -1, "JGZ")], 1)
    chain("k-narrow", [([], "addacc", -5, "JGZ"), (again, "bump", -8388608, "JGZ")], 8388608)
    return rows


@functools.lru_cache(maxsize=None)
def _self_loop_table():
    rows = []
    for body in ("bump", "bak", "twice", "neg"):  # the product: every step, both signs, every exit that can end it
        for step in SELF_LOOP_STEPS:
            for s in (step, -step):
                for exit_ in SELF_LOOP_EXITS:
                    if ("+" if s > 0 else "-") in _ENDS[exit_]:
                        rows.append(_single(body, s, exit_))
    # Rows that leave at the first test or never (the bump runs away from the
    # exit test, or the loop stays only while the register is 0), the test on
    # a register the body does not write, and 2 x + s: a sample of the steps.
    # With MK_JIT_SAT_COUNT on these are the only MAD24 loops under the > 0
    # and < 0 flags.
    for step in _FEW:
        for s in (step, -step):
            for exit_ in SELF_LOOP_EXITS:
                if ("+" if s > 0 else "-") not in _ENDS[exit_]:
                    rows.append(_single("bump", s, exit_))
    for step in (1, 8388609, 2147483648):
        for s in (step, -step):
            for exit_ in ("JGZ", "JLZ", "iJEZ", "iJNZ"):
                rows.append(_single("other", s, exit_))
    for s in (-5, 5, -255, 1073741825):
        for exit_ in ("JGZ", "JLZ", "iJLZ", "iJGZ"):
            rows.append(_single("addacc", s, exit_))
    rows += _chains()
    assert len({r[0] for r in rows}) == len(rows)
    return {r[0]: r for r in rows}


def self_loop_programs():
    """[(label, nodes, expected_form)]: single loops '<body>/<signed step>/<exit>'
    and chains 'chain/<name>'.

    The product of SELF_LOOP_STEPS, both signs and SELF_LOOP_EXITS is taken
    where the bump moves towards the exit (JNZ and the inverted JEZ: both
    signs), over the bodies whose loops can then run long (bump, bak, twice,
    neg).  The other half of the plain product -- a bump that runs away from
    its exit test, and JEZ / inverted JNZ, which stay only while the register
    is 0 -- leaves at the first test or never: of those, and of the `other`
    and `addacc` bodies, a sample of steps is kept (under a fifth of the
    rows, test_self_loop_cases_end_every_way lists them)."""
    return [r[:3] for r in _self_loop_table().values()]


def self_loop_meta(label: str) -> dict:
    """What the tests need to know of a row: uf and inc (unguarded iterations
    per exit test, steps per iteration) of its last loop, the static steps
    ahead of the first loop, the factor between an input and the register at
    the loop, and `head`: the program up to the last loop, then OUT ACC."""
    return dict(_self_loop_table()[label][3])


def _i32(v: int) -> int:
    return max(-(2**31), min(2**31 - 1, v))


def self_loop_inputs(label: str, n: int):
    """Seeded by the label.  Multiples of the step up to 110 trips on both
    sides of 0 (JNZ loops end only on those), values between, the edges of
    _edge_inputs -- scaled down as well where the program scales its input up,
    so that the loop sees +-2^30 -- and small values.  With a budget of 6,000
    no lane walks further than that."""
    import zlib

    m = self_loop_meta(label)
    rng = random.Random(zlib.crc32(label.encode()))
    mult, ad = m["mult"], abs(m["step"])
    span = 110
    hi = _i32(span * ad // mult)
    edges = [0, 1, -1, 2**30, -(2**30), 2**30 + 1, -(2**30) - 1, 2**31 - 1, -(2**31), 2**31 - 2, -(2**31) + 1]
    if mult > 1:
        edges += [2**30 // mult, -(2**30 // mult), 2**30 // mult + 1, -(2**30 // mult) - 1]

    import math

    q = mult // math.gcd(ad, mult)  # k * step is `mult` times an input for every q-th k

    def multiple(k):
        """The input for k trips to 0, or the nearest count an int32 input can give."""
        sign = -1 if k < 0 else 1
        k = max(q, (abs(k) + q // 2) // q * q)
        while k and not -(2**31) <= sign * k * ad // mult < 2**31:
            k -= q
        return sign * k * ad // mult

    # one and two trips (exactly to 0, and past it), just past two chunks of 32 and the longest, on both
    # sides, and 0; then the seeded mix
    half = [_i32(sign * k * ad // (2 * mult)) for k in (1, 3) for sign in (1, -1)]  # between the multiples
    xs = ([multiple(k) for k in (1, -1, 2, -2, 70, -70, span, -span)] + [0] + half + [3, -3, 4, -4])[:n]
    while len(xs) < n:
        c = rng.random()
        if c < 0.15:
            xs.append(rng.choice(edges))
        elif c < 0.25:
            xs.append(rng.randint(-3, 3))
        elif c < 0.65:
            xs.append(multiple(rng.randint(-span, span)))
        else:
            xs.append(rng.randint(-hi, hi))
    return xs


def self_loop_budgets(label: str, uf: int | None = None) -> list:
    """Every budget from 1 to prelude + 2 uf inc + inc + 8: the unguarded
    iterations T of the loop pass 0, uf - 1, uf, uf + 1, 2 uf - 1, 2 uf and
    2 uf + 1, at every position inside an iteration; then 997 and 6000.
    ``uf``: another chunk size than the default (MK_JIT_LOOP_UNROLL).
    Chains: up to 400, which walks the later loops' T for the step counts
    their lanes arrive with."""
    m = self_loop_meta(label)
    top = m["prelude"] + 2 * (uf or m["uf"]) * m["inc"] + m["inc"] + 8
    if m["nloops"] > 1:
        top = max(top, 400)
    return list(range(1, top + 1)) + [997, 6000]


def _pick(rows, want):
    """Rows by label, in the order asked."""
    have = {r[0]: r for r in rows}
    return [have[w] for w in want]


# The GPU's subset: every form and every step at least once (both checked by
# test_jit_codegen.py test_self_loop_gpu_subset_covers_forms_and_steps).
SELF_LOOP_GPU = (
    "bump/-1/JGZ", "bump/+1/JLZ", "bump/-2/JNZ", "bump/+3/JLZ", "bump/-5/JNZ", "bump/+6/iJEZ", "bump/-12/iJLZ",
    "bump/+48/iJGZ", "bump/-255/JGZ", "bump/+255/JNZ", "bump/-8388607/JGZ", "bump/+8388607/iJEZ",
    "bump/-8388607/JNZ", "bump/+8388608/JLZ", "bump/-8388608/JNZ", "bump/+8388609/iJEZ", "bump/-1073741823/JGZ",
    "bump/+1073741824/JLZ", "bump/-1073741824/iJLZ", "bump/+1073741825/JNZ", "bump/-2147483647/JGZ",
    "bump/+2147483647/iJGZ", "bump/-2147483648/JGZ", "bump/+4294967296/JLZ", "bump/+1/JNZ", "bump/-1/iJEZ",
    "bump/+255/JGZ", "bump/-255/JLZ", "bump/+8388607/JGZ", "bump/-1/JEZ", "bump/+255/iJNZ", "bump/+1/JGZ",
    "bak/-5/JGZ", "bak/+1/JLZ", "bak/-4294967296/JGZ", "bak/+1073741825/iJGZ", "twice/-3/JGZ", "twice/+2/JNZ",
    "neg/-48/JGZ", "neg/+6/iJEZ", "other/-8388609/JGZ", "other/+1/iJEZ", "addacc/-5/JGZ",
    "chain/down1-up6-nz7", "chain/up1-down3", "chain/nz1-bak5", "chain/down1-const-down2", "chain/wide-down1",
)
# ... and of those, the rows every machine variant and knob runs
SELF_LOOP_GPU_FEW = (
    "bump/-1/JGZ", "bump/+3/JLZ", "bump/-255/JGZ", "bump/-8388607/JNZ", "bump/+8388608/JLZ", "bump/-12/iJLZ",
    "bump/+255/JGZ", "bump/-1073741823/JGZ", "bump/+4294967296/JLZ", "bak/-5/JGZ", "neg/-48/JGZ",
    "chain/down1-up6-nz7",
)


def self_loop_gpu_programs(few: bool = False):
    """The curated rows of self_loop_programs for the GPU (48; few: 12)."""
    return _pick(self_loop_programs(), SELF_LOOP_GPU_FEW if few else SELF_LOOP_GPU)
