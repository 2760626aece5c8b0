"""Degenerate calls of every compute form of a session set, host and device:
nothing to do (ncalls = 0, m = 0, total = 0, an all-zero off), null arrays
with and without work to do, bad lists with nothing to do, on a set of n = 3
and on a set of n = 0.  Each row asserts the exact return code of the C ABI;
on the set of 3, which has made one call, the state is compared with a
snapshot taken before the rows: a refusal and a call with nothing to do leave
every record as it was."""
import ctypes as C

import numpy as np
import pytest

import misaka_net_amd as mk
from misaka_net_amd import _native as N
from test_sessions_indexed import tier  # noqa: F401  (a fixture)

OK, EINVAL = N.MK_OK, N.MK_EINVAL


def _u32(*a):
    return np.array(a, np.uint32)


def _rows(n, H, D):
    """(label, entry point, arguments after the set, expected code).  H, D: a
    valid host / device array of 64 bytes, standing for in, out, status and
    steps alike; no row with valid arrays makes more than 4 calls."""
    z = None
    good = _u32(0, 2) if n else _u32()          # a valid list (of every n)
    m = good.size
    bad = _u32(1, 1) if n else _u32(0)          # not increasing / not an instance
    ones = _u32(*([1] * (n + 1)))               # off[0] = 1
    zeros = _u32(*([0] * (n + 1)))
    down = _u32(0, 2, 1, 3)
    work = _u32(0, 1, 1, 2) if n else _u32(0)
    dn = n or 1
    rows = [
        # ---- plain, seq, step / resume: host
        ("compute null", "mk_session_compute", (z, z, z, z), EINVAL if n else OK),
        ("seq ncalls=0", "mk_session_compute_seq", (H, 0, H, H, H), OK),
        ("seq ncalls=0 null", "mk_session_compute_seq", (z, 0, z, z, z), OK),
        ("seq null in", "mk_session_compute_seq", (z, 1, H, H, H), EINVAL if n else OK),
        ("seq null out", "mk_session_compute_seq", (H, 1, z, H, H), EINVAL if n else OK),
        ("seq null status", "mk_session_compute_seq", (H, 1, H, z, H), EINVAL if n else OK),
        ("step null out", "mk_session_step", (H, z, H, H), EINVAL if n else OK),
        ("resume null out", "mk_session_step", (z, z, H, H), EINVAL if n else OK),
        ("resume null status", "mk_session_step", (z, H, z, z), EINVAL if n else OK),
        # ---- device
        ("compute_device null", "mk_session_compute_device", (z, z, z, z, z), EINVAL if n else OK),
        ("seq_device ncalls=0", "mk_session_compute_seq_device", (D, 0, D, D, D, z), OK),
        ("seq_device ncalls=0 null", "mk_session_compute_seq_device", (z, 0, z, z, z, z), OK),
        ("seq_device null in", "mk_session_compute_seq_device", (z, 1, D, D, D, z), EINVAL if n else OK),
        ("seq_device null status", "mk_session_compute_seq_device", (D, 1, D, z, D, z), EINVAL if n else OK),
        ("seq_device 2^32 calls", "mk_session_compute_seq_device", (D, 1 << 32, D, D, D, z), EINVAL),
        # ---- indexed: host
        ("indexed m=0", "mk_session_compute_indexed", (z, 0, z, 1, z, z, z), OK),
        ("indexed m=0, arrays", "mk_session_compute_indexed", (H, 0, H, 1, H, H, H), OK),
        ("indexed ncalls=0", "mk_session_compute_indexed", (good, m, z, 0, z, z, z), OK),
        ("indexed bad list, ncalls=0", "mk_session_compute_indexed", (bad, bad.size, H, 0, H, H, H), EINVAL),
        ("indexed null list, ncalls=0", "mk_session_compute_indexed", (z, 1, H, 0, H, H, H), EINVAL),
        ("indexed m>n, ncalls=0", "mk_session_compute_indexed", (_u32(0, 1, 2, 3), n + 1, H, 0, H, H, H), EINVAL),
        ("step_indexed m=0", "mk_session_step_indexed", (z, 0, z, z, z, z), OK),
        ("resume_indexed bad list", "mk_session_step_indexed", (bad, bad.size, z, H, H, H), EINVAL),
        # ---- indexed: device
        ("indexed_device m=0", "mk_session_compute_indexed_device", (z, 0, z, 1, z, z, z, z), OK),
        ("indexed_device ncalls=0", "mk_session_compute_indexed_device", (z, n, z, 0, z, z, z, z), OK),
        ("indexed_device m>n, ncalls=0", "mk_session_compute_indexed_device", (D, n + 1, D, 0, D, D, D, z), EINVAL),
        ("indexed_device null list", "mk_session_compute_indexed_device", (z, 1, D, 1, D, D, D, z), EINVAL),
        # ---- ragged: host (a null list stands for every session: m == n)
        ("ragged m=0, null list", "mk_session_compute_ragged", (z, 0, z, z, z, z, z), EINVAL if n else OK),
        ("ragged m=0, a list", "mk_session_compute_ragged", (H, 0, z, z, z, z, z), OK),
        ("ragged m=0, a list, off", "mk_session_compute_ragged", (H, 0, zeros, H, H, H, H), OK),
        ("ragged null off", "mk_session_compute_ragged", (z, dn, z, H, H, H, H), EINVAL),
        ("ragged m!=n, null list", "mk_session_compute_ragged", (z, n + 1, zeros, H, H, H, H), EINVAL),
        ("ragged bad list, zero off", "mk_session_compute_ragged", (bad, bad.size, zeros, H, H, H, H), EINVAL),
        ("ragged zero off, null arrays", "mk_session_compute_ragged", (z, n, zeros, z, z, z, z), OK),
        ("ragged zero off, a list", "mk_session_compute_ragged", (good, m, zeros, z, z, z, z), OK),
        # ---- ragged: device
        ("ragged_device m=0", "mk_session_compute_ragged_device", (z, 0, z, 0, z, z, z, z, z), OK),
        ("ragged_device m=0, total=1", "mk_session_compute_ragged_device", (z, 0, z, 1, z, z, z, z, z), OK),
        ("ragged_device total=0", "mk_session_compute_ragged_device", (z, n, z, 0, z, z, z, z, z), OK),
        ("ragged_device m>n", "mk_session_compute_ragged_device", (D, n + 1, D, 0, D, D, D, D, z), EINVAL),
        ("ragged_device 2^32 calls", "mk_session_compute_ragged_device", (D, dn, D, 1 << 32, D, D, D, D, z), EINVAL),
        # ---- queue
        ("queue total=0", "mk_session_compute_queue", (z, z, 0, z, z, z), OK),
        ("queue total=0, arrays", "mk_session_compute_queue", (H, H, 0, H, H, H), OK),
        ("queue null ids", "mk_session_compute_queue", (z, H, 1, H, H, H), EINVAL),
        ("queue null in", "mk_session_compute_queue", (H, z, 1, H, H, H), EINVAL),
        ("queue null status", "mk_session_compute_queue", (H, H, 1, H, z, H), EINVAL),
        ("queue id >= n", "mk_session_compute_queue", (_u32(0, n), H, 2, H, H, H), EINVAL),
        ("queue 2^32 requests", "mk_session_compute_queue", (H, H, 1 << 32, H, H, H), EINVAL),
        ("queue_device total=0", "mk_session_compute_queue_device", (z, z, 0, z, z, z, z), OK),
        ("queue_device null ids", "mk_session_compute_queue_device", (z, D, 1, D, D, D, z), EINVAL),
        ("queue_device null out", "mk_session_compute_queue_device", (D, D, 1, z, D, D, z), EINVAL),
        ("queue_device 2^32 requests", "mk_session_compute_queue_device", (D, D, 1 << 32, D, D, D, z), EINVAL),
    ]
    if n:
        rows += [
            ("indexed null in", "mk_session_compute_indexed", (good, m, z, 1, H, H, H), EINVAL),
            ("indexed null status", "mk_session_compute_indexed", (good, m, H, 1, H, z, H), EINVAL),
            ("step_indexed null out", "mk_session_step_indexed", (good, m, H, z, H, H), EINVAL),
            ("resume_indexed null status", "mk_session_step_indexed", (good, m, z, H, z, H), EINVAL),
            ("indexed_device null in", "mk_session_compute_indexed_device", (D, m, z, 1, D, D, D, z), EINVAL),
            ("ragged m!=n, null list, fewer", "mk_session_compute_ragged", (z, n - 1, zeros, H, H, H, H), EINVAL),
            ("ragged off[0]=1", "mk_session_compute_ragged", (z, n, ones, H, H, H, H), EINVAL),
            ("ragged off[0]=1, a list", "mk_session_compute_ragged", (good, m, ones, H, H, H, H), EINVAL),
            ("ragged decreasing off", "mk_session_compute_ragged", (z, n, down, H, H, H, H), EINVAL),
            ("ragged null in", "mk_session_compute_ragged", (z, n, work, z, H, H, H), EINVAL),
            ("ragged null out", "mk_session_compute_ragged", (z, n, work, H, z, H, H), EINVAL),
            ("ragged null status", "mk_session_compute_ragged", (z, n, work, H, H, z, H), EINVAL),
            ("ragged_device m!=n, null list", "mk_session_compute_ragged_device", (z, n - 1, D, 0, D, D, D, D, z),
             EINVAL),
            ("ragged_device null off", "mk_session_compute_ragged_device", (z, n, z, 2, D, D, D, D, z), EINVAL),
            ("ragged_device null in", "mk_session_compute_ragged_device", (z, n, D, 2, z, D, D, D, z), EINVAL),
        ]
    else:
        rows += [
            ("resume", "mk_session_step", (z, H, H, H), OK),
            ("step", "mk_session_step", (H, H, H, H), OK),
            ("seq 2^32 calls", "mk_session_compute_seq", (H, 1 << 32, H, H, H), OK),
            ("queue an id", "mk_session_compute_queue", (_u32(0), H, 1, H, H, H), EINVAL),
        ]
    return rows


def _arg(a):
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 0])
def test_degenerate_calls_return_codes_and_leave_the_set(gpu, tier, n):
    import torch

    g = mk.Network(mk.networks.example_network()).sessions(n)
    assert g.plan().startswith("tier=" + tier), g.plan()
    if n:
        g.compute(np.arange(n))
    before = g.snapshot().rec.copy()
    host = np.zeros(8, np.int64)
    dev = torch.zeros(8, dtype=torch.int64, device=gpu)
    lib = N.lib()
    for label, fn, args, want in _rows(n, host, C.c_void_p(dev.data_ptr())):
        got = getattr(lib, fn)(g._h, *[_arg(a) for a in args])
        assert got == want, f"{label}: {fn} returned {got}, expected {want} (n = {n}, {tier})"
        assert np.array_equal(g.snapshot().rec, before), f"{label}: the set's state changed (n = {n}, {tier})"
    assert not host.any(), "a degenerate call wrote to its host arrays"
    if n:  # the set still serves: the second call of every instance, as a set that made no degenerate call
        f = mk.Network(mk.networks.example_network()).sessions(n)
        f.compute(np.arange(n))
        a, b = g.compute(np.arange(n) + 7), f.compute(np.arange(n) + 7)
        assert np.array_equal(a.out, b.out) and np.array_equal(a.status, b.status) and np.array_equal(a.steps, b.steps)
        f.close()
    g.close()


@pytest.mark.gpu
def test_queue_device_on_an_empty_set_answers_zero(gpu, tier):
    """No id names an instance of a set of 0: every request reports 0 / 0 / 0."""
    import torch

    g = mk.Network(mk.networks.example_network()).sessions(0)
    ids = torch.tensor([0, 5], dtype=torch.int32, device=gpu)
    x = torch.tensor([1, 2], dtype=torch.int64, device=gpu)
    out = torch.full((2,), -1, dtype=torch.int32, device=gpu)
    st = torch.full((2,), 9, dtype=torch.uint8, device=gpu)
    sp = torch.full((2,), 9, dtype=torch.int32, device=gpu)
    g.compute_queue_device(ids.data_ptr(), x.data_ptr(), 2, out.data_ptr(), st.data_ptr(), sp.data_ptr())
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0] and st.tolist() == [0, 0] and sp.tolist() == [0, 0]
    g.close()
