"""Session snapshots (mk_session_snapshot / _restore, SessionSet.snapshot /
restore / fork): a session's state out of a set and back -- rewind, subsets,
migration to another set and another tier, the record read by the CPU oracle,
forks, bad blocks and the device forms -- against n single-instance oracle
sets (test_sessions_indexed.Ref); out, status and steps bit-exact.

n = 600 is two full blocks and a partial one.  The prefix is two plain calls
on all sessions (inputs of seeds 1001 and 1002); after it stackloop7 has idle
sessions, sessions with a call open (handed to the interpreter on the native
tier) and ended ones, countdown1000 idle and open ones."""
import ctypes as C

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from schedcheck import OrcFlat
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, SEL, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)

ALL = SEL["all"]
# idle / open / ended after the prefix, from the reference's statuses; measured 382 / 159 / 59 and 84 / 516 / 0
MIX = {"stackloop7": (50, 50, 50), "countdown1000": (50, 50, 0)}


def _set(name, tier=None, n=NS):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(n, **kw)
    if tier:
        assert g.plan().startswith("tier=" + tier), g.plan()
    return g, nodes, kw, gen


def _prefix(g, refs, gen, name):
    """Two plain calls on all sessions; g is compared with refs[0], the other references replay them."""
    x = _Inputs(gen, 1000)
    for k in range(2):
        v = x(NS)
        want = [r.call(ALL, v) for r in refs]
        if g is not None:
            assert_same(g.compute(v, busy_ok=True), want[0], f"{name} prefix call {k}")
    r = refs[0]
    idle, opened, ended = ~r.open.astype(bool) & ~r.dead, r.open.astype(bool), r.dead
    if name in MIX:
        lo = MIX[name]
        assert idle.sum() >= lo[0] and opened.sum() >= lo[1] and ended.sum() >= lo[2], \
            (name, int(idle.sum()), int(opened.sum()), int(ended.sum()))


def _open_agrees(g, r, ctx):
    assert np.array_equal(g.call_open(), r.open), ctx


# ---- 4 and 5: rewind, and the round trip is exact -----------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_snapshot_rewind(gpu, name, tier):
    g, nodes, kw, gen = _set(name, tier)
    ra, rb = Ref(nodes, NS, **kw), Ref(nodes, NS, **kw)
    _prefix(g, [ra, rb], gen, name)
    snap = g.snapshot()
    assert snap.rec.shape == (snap.layout.rows, NS) and snap.rec.dtype == np.uint32
    live = ~ra.dead
    if tier == "native":
        assert np.array_equal(snap.held[live], ~ra.held[live]), "held is not the reference's"
        assert snap.layout.native_rows > 0 and snap.layout.native_hash != 0
    else:
        assert not snap.held.any() and snap.layout.native_rows == 0 and snap.layout.native_hash == 0
    # suffix A: resume, cancel, two calls
    xa = _Inputs(gen, 1100)
    assert_same(g.resume(), ra.call(ALL, None), f"{name} A resume")
    g.cancel()
    ra.cancel(ALL)
    for k in range(2):
        v = xa(NS)
        assert_same(g.compute(v, busy_ok=True), ra.call(ALL, v), f"{name} A call {k}")
    _open_agrees(g, ra, "after suffix A")
    g.restore(snap)
    again = g.snapshot()
    assert np.array_equal(again.rec, snap.rec), "a snapshot right after the restore differs from the one restored"
    _open_agrees(g, rb, "after the restore")
    # suffix B: resume, a call, cancel, two calls with other seeds
    xb = _Inputs(gen, 1200)
    assert_same(g.resume(), rb.call(ALL, None), f"{name} B resume")
    v = xb(NS)
    assert_same(g.compute(v, busy_ok=True), rb.call(ALL, v), f"{name} B busy call")
    g.cancel()
    rb.cancel(ALL)
    for k in range(2):
        v = xb(NS)
        assert_same(g.compute(v, busy_ok=True), rb.call(ALL, v), f"{name} B call {k}")
    _open_agrees(g, rb, "after suffix B")
    g.close()


# ---- 6: a subset ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_snapshot_subset(gpu, name, tier):
    g, nodes, kw, gen = _set(name, tier)
    took, skipped = Ref(nodes, NS, **kw), Ref(nodes, NS, **kw)
    _prefix(g, [took, skipped], gen, name)
    sel = SEL["random257"]
    listed = np.zeros(NS, bool)
    listed[sel] = True
    snap = g.snapshot(index=sel)
    assert snap.m == sel.size
    x = _Inputs(gen, 1300)
    for k in range(2):
        v = x(NS)
        assert_same(g.compute(v, busy_ok=True), took.call(ALL, v), f"{name} call {k} in between")
    g.restore(snap, index=sel)
    want_open = np.where(listed, skipped.open, took.open)
    assert np.array_equal(g.call_open(), want_open)
    v = x(NS)
    a, b = took.call(ALL, v), skipped.call(ALL, v)
    assert_same(g.compute(v, busy_ok=True), tuple(np.where(listed, q, p) for p, q in zip(a, b)), f"{name} plain call")
    assert np.array_equal(g.call_open(), np.where(listed, skipped.open, took.open))
    g.close()


# ---- 7: migration, across sets and tiers ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pairing", ["native-native", "native-interp", "interp-native", "native-bytes-native"])
@pytest.mark.parametrize("name", ["example", "countdown1000", "stackloop7"])
def test_snapshot_migration(gpu, name, pairing, monkeypatch):
    src_tier, dst_tier = pairing.split("-")[0], pairing.split("-")[-1]

    def make(t, n):
        if t == "interp":
            monkeypatch.setenv("MK_SESSION_NATIVE", "0")
        else:
            monkeypatch.delenv("MK_SESSION_NATIVE", raising=False)
        return _set(name, t, n)

    g, nodes, kw, gen = make(src_tier, NS)
    r = Ref(nodes, NS, **kw)
    _prefix(g, [r], gen, name)
    run = SEL["run"]
    snap = g.snapshot(index=run)
    if "bytes" in pairing:
        snap = mk.SessionSnapshot.frombytes(snap.tobytes())
    h = make(dst_tier, run.size)[0]
    h.restore(snap)
    after = h.snapshot()
    if pairing.startswith("native") and dst_tier == "native":
        assert np.array_equal(after.held, snap.held)
        assert np.array_equal(after.rec, snap.rec)
    else:
        assert not after.held.any()
    assert np.array_equal(h.call_open(), r.open[run])
    x = _Inputs(gen, 1400)
    for k in range(3):
        v = x(run.size)
        assert_same(h.compute(v, busy_ok=True), r.call(run, v), f"{name} {pairing} call {k} on the target")
    assert np.array_equal(h.call_open(), r.open[run])
    g.close()
    h.close()


# ---- 8: the oracle reads the record ----------------------------------------------
def _flat(c, lay):
    """A record's canonical part (SessionSnapshot.canonical) in the oracle's terms.  The oracle counts an
    imported call's steps as retired by the CURRENT slice (it imports hand-offs, which stand mid-slice); a
    record's open call stands between slices, so it is imported with 0 steps and c['csteps'] added to what
    the oracle then reports for that call."""
    f = OrcFlat()
    for n in range(lay.nprog):
        f.acc[n], f.bak[n] = int(c["acc"][n]), int(c["bak"][n])
        f.ip[n], f.pendv[n] = int(c["ip"][n]), int(c["pendv"][n])
        for k in range(4):
            f.port[4 * n + k] = int(c["port"][n, k])
    f.pfull, f.pend, f.hung = c["pfull"], c["pend"], c["hung"]
    f.in_full, f.out_full, f.in_val, f.out_val = c["in_full"], c["out_full"], c["in_val"], c["out_val"]
    ent = np.ascontiguousarray(c["entries"].reshape(-1).astype(np.int32))
    if ent.size == 0:
        ent = np.zeros(1, np.int32)
    for s in range(lay.nstack):
        f.depth[s] = int(c["depth"][s])
    f.entries = ent.ctypes.data
    f.deposited, f.pin, f.pos, f.changed, f.csteps = 0 if c["undeposited"] else 1, c["pin"], 0, 0, 0
    return f, ent


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_oracle_reads_the_record(gpu, name):
    g, nodes, kw, gen = _set(name, "native")
    r = Ref(nodes, NS, **kw)
    _prefix(g, [r], gen, name)
    snap = g.snapshot()
    net = po.OracleNet(nodes)
    probes, carry = {}, np.zeros(NS, np.uint32)
    for t in np.nonzero(~r.dead)[0]:
        c = snap.canonical(int(t))
        assert c["dead"] == 0 and c["call_open"] == r.open[t] and c["held"] == (0 if r.held[t] else 1), (name, t)
        f, ent = _flat(c, snap.layout)
        o = po.OracleSessions(net, 1, stack_cap=kw.get("stack_cap"))
        o.import_state(0, f)
        if c["call_open"]:
            carry[t] = c["csteps"]
        else:
            o.cancel()
        probes[int(t)] = (o, f, ent)
    for t in np.nonzero(r.dead)[0]:
        assert snap.canonical(int(t))["dead"] == N.MK_ST_STACK_OVERFLOW
    assert len(probes) == int((~r.dead).sum()) >= 100
    x = _Inputs(gen, 1500)
    for k in range(3):
        v = None if k == 0 else x(NS)
        got = g.resume() if k == 0 else g.compute(v, busy_ok=True)
        for t, (o, _, _) in probes.items():
            out, st, sp = (int(a[0]) for a in o.compute(None if v is None else [v[t]], budget=kw.get("budget")))
            if k == 0 and st != 0:
                sp += int(carry[t])  # the resumed call's earlier slices
            assert (int(got.out[t]), int(got.status[t]), int(got.steps[t])) == (out, st, sp), (name, k, t)
    g.close()


# ---- 9: fork ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["example", "countdown1000", "stackloop7"])
def test_fork(gpu, name, tier):
    g, nodes, kw, gen = _set(name, tier)
    r = Ref(nodes, NS, **kw)
    x = _Inputs(gen, 1600)
    for k in range(4):
        v = x(1)
        want = r.call(ALL, np.repeat(v, NS))  # every reference instance replays session 17's calls
        assert_same(g.compute(v, index=[17], busy_ok=True), tuple(a[17:18] for a in want), f"{name} call {k} on 17")
    g.fork(17, np.setdiff1d(ALL, [17]))
    assert np.array_equal(g.call_open(), r.open)
    v = x(NS)
    assert np.unique(v).size >= 8  # each fork takes its own input (stackloop7's generator has 16 values)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), f"{name} call after the fork")
    assert_same(g.resume(), r.call(ALL, None), f"{name} resume after the fork")
    g.close()


def test_fork_and_restore_argument_errors():
    import types

    s = types.SimpleNamespace(n=10)
    s._index = lambda index: mk.SessionSet._index(s, index)
    with pytest.raises(ValueError, match="fork source 10"):
        mk.SessionSet.fork(s, 10, [1])
    with pytest.raises(ValueError, match=r"position 1\b"):
        mk.SessionSet.fork(s, 0, [2, 2])


# ---- 10: bad blocks change nothing ------------------------------------------------
@pytest.mark.gpu
def test_bad_blocks_change_nothing(gpu, tier):
    name = "stackloop7"
    g, nodes, kw, gen = _set(name, tier)
    r = Ref(nodes, NS, **kw)
    _prefix(g, [r], gen, name)
    snap = g.snapshot()
    lay = snap.layout
    lib = N.lib()

    def refused(s, field=None, index=None):
        with pytest.raises(ValueError, match=field):
            g.restore(s, index=index)
        sel = None if index is None else np.asarray(index, np.uint32)
        rec = np.ascontiguousarray(s.rec)
        rc = lib.mk_session_restore(g._h, sel.ctypes.data_as(C.c_void_p) if sel is not None else None,
                                    NS if sel is None else sel.size, C.byref(s.layout),
                                    rec.ctypes.data_as(C.c_void_p), rec.shape[1], None)
        assert rc == N.MK_EINVAL, rc

    def edited(row, col, value):
        rec = snap.rec.copy()
        rec[row, col] = value
        return mk.SessionSnapshot(lay, rec)

    other = mk.Network(mk.networks.countdown_network()).sessions(NS, budget=1000)
    refused(other.snapshot(), "net_hash")
    other.close()
    capped = mk.Network(nodes).sessions(NS, budget=kw["budget"], stack_cap=kw["stack_cap"] + 1)
    refused(capped.snapshot(), "stack_cap")
    capped.close()
    node0, stack0 = 9, 9 + 10 * lay.nprog
    refused(edited(node0 + 4, 300, 100000), "out of range")  # an ip past its program
    refused(edited(node0 + 4, 599, 0xFFFFFFFF), "out of range")  # ... and a negative one
    refused(edited(stack0, 0, kw["stack_cap"] + 1), "out of range")  # a depth above the cap
    refused(edited(0, 257, 2), "out of range")  # held > 1
    if tier == "native":
        t = int(np.nonzero(snap.held & ~r.dead)[0][3])
        sb_row = lay.rows - lay.native_rows
        for sb in (0xFFFFFF00, snap.rec[sb_row, t] | 1, 2 * 100000):  # no superblock, a checked variant, past the last
            refused(edited(sb_row, t, sb), "out of range")
    refused(snap, r"position 1\b", index=[5, 4])
    # the set is what it was: a plain call on all sessions matches the reference
    v = _Inputs(gen, 1700)(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), "plain call after the refused restores")
    assert np.array_equal(g.call_open(), r.open)
    g.close()


# ---- 11: the device forms across streams --------------------------------------------
@pytest.mark.gpu
def test_device_forms_across_streams(gpu, tier):
    import torch

    name = "countdown1000"
    g, nodes, kw, gen = _set(name, tier)
    ra, rb = Ref(nodes, NS, **kw), Ref(nodes, NS, **kw)
    x = _Inputs(gen, 1000)
    bursts = [np.stack([x(NS), x(NS)]) for _ in range(3)]  # the prefix, then two calls each for A and for B
    want = [[r.call(ALL, v) for v in bursts[0]] for r in (ra, rb)][0]
    want += [ra.call(ALL, v) for v in bursts[1]] + [rb.call(ALL, v) for v in bursts[2]]
    lay = g.layout()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    rec = torch.zeros(lay.rows * NS, dtype=torch.int32, device="cuda")
    bufs = [(torch.from_numpy(v).cuda(), torch.empty((2, NS), dtype=torch.int32, device="cuda"),
             torch.empty((2, NS), dtype=torch.uint8, device="cuda"),
             torch.empty((2, NS), dtype=torch.int32, device="cuda")) for v in bursts]
    torch.cuda.synchronize()

    def burst(k):
        d_in, out, st, sp = bufs[k]
        g.compute_seq_device(d_in.data_ptr(), 2, out.data_ptr(), st.data_ptr(), sp.data_ptr(), stream=sa.cuda_stream)

    burst(0)
    g.snapshot_device(rec.data_ptr(), stream=sb.cuda_stream)
    burst(1)
    g.restore_device(lay, rec.data_ptr(), NS, stream=sb.cuda_stream)
    burst(2)
    torch.cuda.synchronize()
    for k, (_, out, st, sp) in enumerate(bufs):
        for c in range(2):
            got = mk.network.BatchResult(out[c].cpu().numpy(), st[c].cpu().numpy(),
                                         sp[c].cpu().numpy().astype(np.uint32))
            assert_same(got, want[2 * k + c], f"burst {k} call {c}")
    assert np.array_equal(g.call_open(), rb.open)
    host = g.snapshot()
    assert np.array_equal(host.held, ~rb.held if tier == "native" else np.zeros(NS, bool))
    g.close()
