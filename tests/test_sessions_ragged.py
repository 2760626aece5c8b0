"""Ragged session bursts (mk_session_compute_ragged, SessionSet.compute_ragged):
one launch in which every listed instance makes its own number of /compute
calls, against the CPU oracle.

The reference is test_sessions_indexed's: n single-instance oracle sets, entry
t stepped cnt[t] times; out, status and steps are compared bit-exactly, in the
launch's entry-major order (call c of entry t at off[t] + c).  n = 600 is two
full blocks and a partial one.  The counts of the main scenario put 0, 1, 5
and 40 calls into one wave, so the kernels' wave-wide call loop runs past most
lanes' own counts."""
import ctypes as C
import hashlib
import subprocess

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from oracle import pyoracle as po
from test_gpu_parity import assert_same
from test_sessions_indexed import NETS, NS, SEL, Ref, _Inputs, tier  # noqa: F401  (tier: a fixture)
from tisgen import stack_loop_network

ALL = SEL["all"]
RAGGED = ["mk_session_compute_ragged", "mk_session_compute_ragged_device"]
# sha256 of the generated text of the plain entry, from `extern "C" __global__
# ... mk_sess_exec(SessK p)` up to the next `extern "C"`, on the commit before
# ragged bursts: the selected entry changed, the plain one must not
PLAIN_ENTRY_SHA256 = "7938f5be9a48e89b441b852d948917b4453340b2a696677629ffecdcb5e7b988"
PLAIN_ENTRY = 'extern "C" __global__ void __launch_bounds__(256) mk_sess_exec(SessK p)'
SEL_ENTRY = 'extern "C" __global__ void __launch_bounds__(256) mk_sess_exec_sel(SessKSel q)'


def _reason(st):
    return np.asarray(st) & N.MK_ST_REASON_MASK


# ---- CPU ----------------------------------------------------------------------
def test_ragged_symbols_resolve_and_refuse_null_session():
    import torch  # noqa: F401  before the library, as everywhere: PyTorch's HIP runtime is the process's one

    lib = N.lib()
    for name in RAGGED:
        assert name in N.SIGNATURES, name
        assert getattr(lib, name) is not None
    sel = np.zeros(1, np.uint32)
    off = np.array([0, 1], np.uint32)
    buf = np.zeros(8, np.int64)
    sp, op, bp = (a.ctypes.data_as(C.c_void_p) for a in (sel, off, buf))
    assert lib.mk_session_compute_ragged(None, sp, 1, op, bp, bp, bp, bp) == N.MK_EINVAL
    assert lib.mk_session_compute_ragged_device(None, sp, 1, op, 1, bp, bp, bp, bp, None) == N.MK_EINVAL


def test_count_errors_name_the_first_offending_position():
    ragged = mk.network.SessionSet._ragged
    v, off = ragged([5, 6, 7, 8], [1, 0, 3])
    assert off.dtype == np.uint32 and off.tolist() == [0, 1, 1, 4]
    assert v.dtype == np.int64 and v.tolist() == [5, 6, 7, 8]
    v, off = ragged([[5], [], [6, 7, 8]], None)
    assert off.tolist() == [0, 1, 1, 4] and v.tolist() == [5, 6, 7, 8]
    v, off = ragged([], [])
    assert off.tolist() == [0] and v.size == 0
    for values, counts, pos in (
            ([1, 2, 3], [1, 2, -1, 4], 2),        # a negative count
            ([1, 2, 3], [2, -3, -1], 1),          # the first of two
            ([1, 2, 3], [1, 2.0], 1),             # a float, even a whole one
            ([1, 2, 3], [1.5, 2], 0),
            ([1, 2, 3], np.array([1.0, 2.0]), 0),
            ([1, 2, 3, 4], [1, 2, 3], 2),         # too few values: they end inside entry 2's calls
            ([1, 2, 3], [1, 2, 0, 5], 3),         # ... inside entry 3's (entry 2 has none)
            ([1, 2, 3, 4], [1, 2], 2)):           # too many: past the last entry
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            ragged(values, counts)


def _entry(src, head):
    a = src.index(head)
    b = src.find('extern "C"', a + 1)
    return src[a:b if b >= 0 else len(src)]


def test_plain_entry_text_unchanged_and_selected_entry_has_offsets():
    import schedcheck as sc

    for nodes, kw in ((mk.networks.example_network(), {}), (mk.networks.countdown_network(), {}),
                      (stack_loop_network(7)[0], dict(stack_cap=8))):
        src = sc.session_module(nodes, **kw)
        assert hashlib.sha256(_entry(src, PLAIN_ENTRY).encode()).hexdigest() == PLAIN_ENTRY_SHA256
        sel = _entry(src, SEL_ENTRY)
        assert "q.off" in sel and "q.total" in sel and "MK_WAVE_MAX(cnt)" in sel
        assert "q.off" not in _entry(src, PLAIN_ENTRY)
        assert src.count('extern "C" __global__') == 2  # no third entry: each one inlines the whole lane code


def test_ragged_session_modules_compile_for_gfx950(tmp_path):
    import schedcheck as sc

    rtc = sc.rtc_tool()
    for name, nodes, kw in (("stackloop7", stack_loop_network(7)[0], dict(stack_cap=8)),
                            ("countdown", mk.networks.countdown_network(), {})):
        p = tmp_path / f"{name}.hip"
        p.write_text(sc.session_module(nodes, **kw))
        r = subprocess.run([rtc, str(p), str(tmp_path / f"{name}.co")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stdout[-2000:])
        assert (tmp_path / f"{name}.co").stat().st_size > 0


# ---- the reference: entry t stepped cnt[t] times --------------------------------
def _offsets(cnt):
    off = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    return off


def ref_ragged(r, sel, cnt, v, *, never_offer_refused=False):
    """The launch on the reference, flat and entry-major.  The instances are
    independent, so call c goes to every entry that has one before call c + 1
    does.  never_offer_refused: a call on an instance with a call open is not
    made at all -- the reference never sees its input -- and is expected to
    report MK_ST_CALL_OPEN, out 0, steps 0."""
    sel, cnt = np.asarray(sel, np.int64), np.asarray(cnt, np.int64)
    off = _offsets(cnt)
    out, st, sp = np.zeros(off[-1], np.int32), np.zeros(off[-1], np.uint8), np.zeros(off[-1], np.uint32)
    for c in range(int(cnt.max()) if cnt.size else 0):
        ts = np.nonzero(cnt > c)[0]
        at = off[ts] + c
        if never_offer_refused:
            refused = r.open[sel[ts]] == 1
            st[at[refused]] = N.MK_ST_CALL_OPEN
            ts, at = ts[~refused], at[~refused]
        out[at], st[at], sp[at] = r.call(sel[ts], v[at])
    return out, st, sp


def _pair(name, tier):
    nodes, kw, gen = NETS[name]()
    g = mk.Network(nodes).sessions(NS, **kw)
    assert g.plan().startswith("tier=" + tier), g.plan()
    return g, Ref(nodes, NS, **kw), gen


def _open_agrees(g, r, ctx):
    assert np.array_equal(g.call_open(), r.open), ctx
    sel = SEL["random257"]
    assert np.array_equal(g.call_open(index=sel), r.open[sel]), ctx


def _first_counts(rng):
    cnt = rng.integers(0, 6, NS)
    cnt[37] = 40
    return cnt


def _before_last(st, cnt, reason):
    """Entries with a call of status `reason` before their last call."""
    off = _offsets(cnt)
    return sum(bool((_reason(st[off[t]:off[t + 1] - 1]) == reason).any()) for t in range(len(cnt)) if cnt[t] > 1)


# entries of the first launch with MK_ST_BUDGET / MK_ST_STACK_OVERFLOW before their last call: at least
# (the oracle alone, with exactly these counts and inputs, gives 390, 336, 208, 301 and 90 / 121)
MIX = {"countdown150": (100, 0), "countdown1000": (100, 0), "random6": (100, 0), "random19": (100, 0),
       "stackloop7": (40, 40)}


def _first_launch(g, r, gen, name, rng):
    """Launch 1 of the rounds, on every session, and what the reference says it exercised."""
    cnt = _first_counts(rng)
    assert 0 in cnt[:64] and 1 in cnt[:64] and 5 in cnt[:64] and cnt[:64].max() == 40  # one wave, its bound diverging
    v = po.gen_inputs(9001, 1543, **gen)
    assert cnt.sum() == 1543
    want = ref_ragged(r, ALL, cnt, v)
    if name == "example":
        assert ((want[1] & N.MK_ST_HAS_OUTPUT) != 0).sum() == 1543
    else:
        got = (_before_last(want[1], cnt, N.MK_ST_BUDGET), _before_last(want[1], cnt, N.MK_ST_STACK_OVERFLOW))
        print(f"{name}: entries with BUDGET / STACK_OVERFLOW before their last call: {got}")
        assert got[0] >= MIX[name][0] and got[1] >= MIX[name][1], (name, got)
        # ... and so with refused calls after it
        assert (_reason(want[1]) == N.MK_ST_CALL_OPEN).sum() >= MIX[name][0]
    res = g.compute_ragged(v, cnt, busy_ok=True)
    assert res.out.shape == res.status.shape == res.steps.shape == (1543,)
    assert_same(res, want, f"{name} ragged launch on all")
    _open_agrees(g, r, "after the launch on all")


# ---- 5: rounds ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_ragged_rounds_then_plain_call(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    rng = np.random.default_rng(4242)
    _first_launch(g, r, gen, name, rng)
    x = _Inputs(gen, 9100)
    for k in ("random257", "run", "empty"):
        sel = SEL[k]
        cnt = rng.integers(0, 6, len(sel))
        v = x(int(cnt.sum()))
        assert_same(g.compute_ragged(v, cnt, index=sel, busy_ok=True), ref_ragged(r, sel, cnt, v), f"{name} ragged {k}")
        _open_agrees(g, r, f"after ragged {k}")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), f"{name} plain call")
    _open_agrees(g, r, "after the plain call")
    g.close()


# ---- 6: a second burst on sessions the interpreter now holds ----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown1000", "stackloop7"])
def test_ragged_second_burst_after_cancel(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    rng = np.random.default_rng(4242)
    _first_launch(g, r, gen, name, rng)
    assert r.held.sum() >= 40 and (~r.held & ~r.dead).sum() >= 40  # both tiers hold sessions (native set)
    g.cancel()
    r.cancel(ALL)
    x = _Inputs(gen, 9200)
    cnt = rng.integers(0, 6, NS)
    cnt[300] = 23
    v = x(int(cnt.sum()))
    assert_same(g.compute_ragged(v, cnt, busy_ok=True), ref_ragged(r, ALL, cnt, v), f"{name} second burst")
    _open_agrees(g, r, "after the second burst")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), f"{name} plain call")
    _open_agrees(g, r, "after the plain call")
    g.close()


# ---- 7: uniform equals ragged -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown150", "stackloop7"])
def test_uniform_burst_equals_ragged(gpu, name, tier):
    g, _, gen = _pair(name, tier)
    h, _, _ = _pair(name, tier)
    x = _Inputs(gen, 9300)
    sel = SEL["random257"]
    m = len(sel)
    v = x(3 * m).reshape(3, m)  # [call][entry]
    a = g.compute_ragged(np.ascontiguousarray(v.T).reshape(-1), np.full(m, 3), index=sel, busy_ok=True)
    b = h.compute_seq(v, index=sel, busy_ok=True)
    assert (_reason(b.status) == N.MK_ST_BUDGET).sum() >= 20 and (_reason(b.status) == N.MK_ST_CALL_OPEN).sum() >= 20
    assert_same(mk.network.BatchResult(a.out.reshape(m, 3).T, a.status.reshape(m, 3).T, a.steps.reshape(m, 3).T),
                (b.out, b.status, b.steps), f"{name} cnt 3")
    assert np.array_equal(g.snapshot().rec, h.snapshot().rec), "the two sets differ after equal bursts"
    # cnt 1 on the identity: the indexed layout
    v = x(NS)
    a = g.compute_ragged(v, np.ones(NS, np.int64), index=ALL, busy_ok=True)
    b = h.compute(v, index=ALL, busy_ok=True)
    assert_same(a, (b.out, b.status, b.steps), f"{name} cnt 1")
    assert np.array_equal(g.snapshot().rec, h.snapshot().rec)
    g.close()
    h.close()


# ---- 8: waves with nothing to do ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["countdown150", "stackloop7"])
def test_ragged_waves_without_calls(gpu, name, tier):
    g, r, gen = _pair(name, tier)
    x = _Inputs(gen, 9400)
    cnt = np.ones(NS, np.int64)
    cnt[0:64] = 0
    cnt[192:256] = 0
    off = _offsets(cnt)
    assert off[NS - 1] < off[NS] == NS - 128
    for k in range(2):  # the second finds calls open
        v = x(NS - 128)
        assert_same(g.compute_ragged(v, cnt, busy_ok=True), ref_ragged(r, ALL, cnt, v), f"{name} launch {k}")
    assert not r.open[:64].any() and r.open[64:192].any()
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), f"{name} plain call")
    _open_agrees(g, r, "after the plain call")
    g.close()


# ---- 9: open calls --------------------------------------------------------------------
@pytest.mark.gpu
def test_ragged_open_calls_busy(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 9500)
    a = SEL["even"]
    v = x(len(a))
    assert_same(g.compute(v, index=a), r.call(a, v), "call on A")
    busy, idle = np.nonzero(r.open)[0], np.nonzero(r.open == 0)[0]
    assert busy.size >= 20 and idle.size >= 20
    zero = np.zeros(8, np.int64)  # countdown from 0 closes within the slice
    # raised for a listed open session with a call to make ...
    d, cnt = np.sort(np.array([busy[0], idle[0]])), np.array([2, 2])
    with pytest.raises(N.MkError) as e:
        g.compute_ragged(zero[:4], cnt, index=d)
    assert e.value.code == N.MK_EBUSY
    ref_ragged(r, d, cnt, zero[:4])
    # ... not for one listed without, nor for an unlisted one
    cnt = np.where(r.open[d] == 1, 0, 3)
    assert_same(g.compute_ragged(zero[:3], cnt, index=d), ref_ragged(r, d, cnt, zero[:3]), "open session with cnt 0")
    d = idle[1:5]
    cnt = np.array([1, 0, 2, 1])
    assert_same(g.compute_ragged(zero[:4], cnt, index=d), ref_ragged(r, d, cnt, zero[:4]), "idle sessions only")
    _open_agrees(g, r, "after the busy checks")
    # busy_ok: the statuses match and the refused calls' inputs are not taken --
    # the reference is never offered them, and a resume of everything agrees
    sel = SEL["random257"]
    cnt = np.random.default_rng(95).integers(0, 5, len(sel))
    v = x(int(cnt.sum()))
    was_open = r.open[sel].copy()
    want = ref_ragged(r, sel, cnt, v, never_offer_refused=True)
    got = g.compute_ragged(v, cnt, index=sel, busy_ok=True)
    assert_same(got, want, "busy_ok launch")
    first = _offsets(cnt)[:-1][cnt > 0]
    assert np.array_equal(got.status[first] == N.MK_ST_CALL_OPEN, was_open[cnt > 0] == 1) and was_open[cnt > 0].any()
    assert (got.status == N.MK_ST_CALL_OPEN).sum() > (was_open[cnt > 0] == 1).sum()  # refused after a BUDGET too
    _open_agrees(g, r, "after the busy_ok launch")
    assert_same(g.resume(), r.call(ALL, None), "resume of everything")
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), "plain call")
    _open_agrees(g, r, "at the end")
    g.close()


# ---- 10: the device form across streams ---------------------------------------------
@pytest.mark.gpu
def test_ragged_device_calls_across_streams(gpu, tier):
    import torch

    g, r, gen = _pair("countdown1000", tier)
    x = _Inputs(gen, 9600)
    rng = np.random.default_rng(96)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # every session (no list), a run, and a list that ends on the last session
    plan = [(None, s1.cuda_stream), (SEL["run"], s2.cuda_stream),
            (np.union1d(SEL["random257"], [NS - 1]), None)]
    bufs, refs = [], []
    for sel, _ in plan:
        m = NS if sel is None else len(sel)
        cnt = rng.integers(0, 5, m)
        cnt[-1] = 2  # the last entry's calls end at off[m] == total
        off = _offsets(cnt)
        total = int(off[-1])
        v = x(total)
        refs.append(ref_ragged(r, ALL if sel is None else sel, cnt, v))
        d_sel = None if sel is None else torch.from_numpy(sel.astype(np.int32)).cuda()  # int32 bits, read as uint32
        bufs.append((d_sel, m, torch.from_numpy(off.astype(np.int32)).cuda(), total, torch.from_numpy(v).cuda(),
                     torch.empty(total, dtype=torch.int32, device="cuda"),
                     torch.empty(total, dtype=torch.uint8, device="cuda"),
                     torch.empty(total, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for (_, stream), (d_sel, m, d_off, total, d_in, out, st, sp) in zip(plan, bufs):
        if d_sel is None:
            g.compute_ragged_device(d_in.data_ptr(), d_off.data_ptr(), total, out.data_ptr(), st.data_ptr(),
                                    sp.data_ptr(), stream=stream)
        else:
            g.compute_ragged_device(d_in.data_ptr(), d_off.data_ptr(), total, out.data_ptr(), st.data_ptr(),
                                    sp.data_ptr(), stream=stream, index_ptr=d_sel.data_ptr(), m=m)
    v = x(NS)
    host = g.compute(v, index=ALL, busy_ok=True)
    torch.cuda.synchronize()
    for k, ((_, _, _, _, _, out, st, sp), ref) in enumerate(zip(bufs, refs)):
        got = mk.network.BatchResult(out.cpu().numpy(), st.cpu().numpy(), sp.cpu().numpy().astype(np.uint32))
        assert_same(got, ref, f"device launch {k}")
    assert_same(host, r.call(ALL, v), "host call")
    _open_agrees(g, r, "at the end")
    g.close()


# ---- 11: refused input changes nothing ------------------------------------------------
@pytest.mark.gpu
def test_ragged_bad_input_changes_nothing(gpu, tier):
    g, r, gen = _pair("countdown150", tier)
    x = _Inputs(gen, 9700)
    sel = SEL["even"]
    cnt = np.random.default_rng(97).integers(0, 4, len(sel))
    v = x(int(cnt.sum()))
    assert_same(g.compute_ragged(v, cnt, index=sel, busy_ok=True), ref_ragged(r, sel, cnt, v), "round")
    lib = N.lib()
    buf = np.ones(64, np.int64)
    bp = buf.ctypes.data_as(C.c_void_p)

    def host(sel, off):
        sel = None if sel is None else np.array(sel, np.uint32)
        off = np.array(off, np.uint32)
        return lib.mk_session_compute_ragged(g._h, None if sel is None else sel.ctypes.data_as(C.c_void_p),
                                             len(off) - 1, off.ctypes.data_as(C.c_void_p), bp, bp, bp, bp)

    assert host([1, 2, 3], [1, 2, 3, 4]) == N.MK_EINVAL      # off[0] != 0
    assert host([1, 2, 3], [0, 3, 2, 4]) == N.MK_EINVAL      # a decreasing pair
    assert host([1, 2, 3], [0, 2, 4, 3]) == N.MK_EINVAL      # ... at the end
    assert host([3, 3], [0, 1, 2]) == N.MK_EINVAL            # a bad list: repeated,
    assert host([5, 4], [0, 1, 2]) == N.MK_EINVAL            # decreasing,
    assert host([0, NS], [0, 1, 2]) == N.MK_EINVAL           # no session,
    assert host(None, [0, 1, 2]) == N.MK_EINVAL              # and none at all with m != n
    for bad in ([3, 3], [5, 4], [0, NS]):
        with pytest.raises(ValueError):
            g.compute_ragged([1, 2], [1, 1], index=bad)
    with pytest.raises(ValueError):
        g.compute_ragged([1, 2], [1, 1])  # two entries for n sessions
    v = x(NS)
    assert_same(g.compute(v, busy_ok=True), r.call(ALL, v), "plain call")
    _open_agrees(g, r, "after the plain call")
    g.close()
