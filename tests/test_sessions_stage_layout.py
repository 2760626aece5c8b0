"""The staging layout of the session host forms (sess_stage.h stage_layout,
through the check library's mkc_stage_layout): where in, out, steps, status
and the extras of a form -- the index list, a ragged burst's offsets, a
queue's ids and its busy flag -- lie in d_stage and its pinned mirror.  A bad
offset here is what would be an access out of bounds on the GPU."""
import ctypes as C
import itertools

import pytest

import schedcheck as sc

NAMES = ["in", "out", "steps", "status", "off", "sel", "ids", "flag"]
SEL, OFF, IDS, FLAG = 1, 2, 4, 8


def _al(b):
    return (b + 255) & ~255


def layout(c, m, extras):
    h = sc.lib()
    h.mkc_stage_layout.argtypes = [C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(C.c_size_t)]
    h.mkc_stage_layout.restype = None
    v = (C.c_size_t * 9)()
    h.mkc_stage_layout(c, m, extras, v)
    return dict(zip(NAMES, v[:8])), v[8]


@pytest.mark.parametrize("c", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257])
def test_regions_aligned_disjoint_long_enough_and_inside(c, m):
    for extras in range(16):
        at, total = layout(c, m, extras)
        need = {"in": c * 8, "out": c * 4, "steps": c * 4, "status": c}
        if extras & OFF:
            need["off"] = (m + 1) * 4
        if extras & SEL:
            need["sel"] = m * 4
        if extras & IDS:
            need["ids"] = c * 4
        if extras & FLAG:
            need["flag"] = 4
        ctx = f"c={c} m={m} extras={extras:04b}"
        spans = sorted((at[k], at[k] + need[k], k) for k in need)
        for lo, hi, k in spans:
            assert lo % 256 == 0, f"{k} at {lo} is not 256-aligned ({ctx})"
            assert hi <= total, f"{k} ends at {hi}, past the {total} bytes ({ctx})"
        for (_, hi, a), (lo, _, b) in zip(spans, spans[1:]):
            assert hi <= lo, f"{a} runs into {b} ({ctx})"
        # no room is taken for an extra that was not asked for
        assert total == sum(_al(b) for b in need.values()), ctx


@pytest.mark.parametrize("c", [1, 63, 64, 65, 1000])
def test_plain_layout_is_the_formula_it_replaced(c):
    for m in (0, 1, 255, 256, 257):
        at, total = layout(c, m, 0)
        assert total == _al(8 * c) + 2 * _al(4 * c) + _al(c)
        assert [at[k] for k in ("in", "out", "steps", "status")] == \
            [0, _al(8 * c), _al(8 * c) + _al(4 * c), _al(8 * c) + 2 * _al(4 * c)]


def test_a_list_alone_starts_the_staging():
    """The small indexed kernels (cancel, reset, call_open, snapshot, restore)
    stage the list with no I/O words: it lies at offset 0."""
    for m, extras in itertools.product((1, 255, 256, 257), (SEL,)):
        at, total = layout(0, m, extras)
        assert at["sel"] == 0 and total == _al(4 * m)
    assert layout(0, 7, 0)[1] == 0
