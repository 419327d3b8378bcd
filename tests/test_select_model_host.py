"""The selection model (tests/select_model.py) without a GPU: pinned to what the reference's own tests/selection.rs asserts, its one combine rule held to literal
restatements of the reference's two merges, the disc's span table held to integer squares, and the two-pass expand / contract formulation the device kernels
use held to the brute force over every case of tests/select_cases.py — the algorithm is proven here before any GPU run.  The last tests load the library
(no device needed) for the span table it builds and the entry points it must export."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import select_cases as SC
from . import select_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tests/selection.rs --------------------------------------------------------------------------------------------------------------------------------------
def test_rect_replace():                                         # :18-34
    m = M.select_rect(None, 100, 100, 10, 10, 50, 50, M.REPLACE)
    assert m[20, 20] == 255 and m[10, 10] == 255 and m[0, 0] == 0 and m[20, 51] == 0
    assert int((m == 255).sum()) == 41 * 41 and set(np.unique(m)) == {0, 255}


def test_ellipse_replace():                                      # :37-51
    m = M.select_ellipse(None, 100, 100, 50.0, 50.0, 20.0, 20.0, M.REPLACE)
    assert m[50, 50] == 255 and m[0, 0] == 0
    assert m[50, 30] == 255 and m[50, 70] == 255 and m[50, 29] == 0 and m[50, 71] == 0      # dx = -1 and 1 are inside


def test_add_subtract_intersect():                               # :58-136
    m = M.select_rect(M.select_rect(None, 100, 100, 0, 0, 30, 30, M.REPLACE), 100, 100, 70, 70, 99, 99, M.ADD)
    assert m[15, 15] == 255 and m[85, 85] == 255 and m[50, 50] == 0
    m = M.select_rect(M.select_rect(None, 100, 100, 0, 0, 99, 99, M.REPLACE), 100, 100, 30, 30, 70, 70, M.SUBTRACT)
    assert m[50, 50] == 0 and m[10, 10] == 255
    m = M.select_rect(M.select_rect(None, 100, 100, 0, 0, 60, 60, M.REPLACE), 100, 100, 40, 40, 99, 99, M.INTERSECT)
    assert m[50, 50] == 255 and m[10, 10] == 0 and m[90, 90] == 0


def test_translate():                                            # :163-200
    m = M.translate(M.select_rect(None, 100, 100, 10, 10, 30, 30, M.REPLACE), 20, 20)
    assert m[15, 15] == 0 and m[35, 35] == 255
    m = M.translate(M.select_rect(None, 100, 100, 80, 80, 99, 99, M.REPLACE), 10, 10)
    assert m[95, 95] == 255 and m[85, 85] == 0
    assert int((m == 255).sum()) == 10 * 10                      # the rest left the canvas


def test_fill_and_delete_of_a_rect():                            # :206-245
    sel = M.select_rect(None, 100, 100, 10, 10, 50, 50, M.REPLACE)
    white = np.full((100, 100, 4), 255, np.uint8)
    filled = M.fill_selected(white, sel, (255, 0, 0, 255))
    assert tuple(filled[20, 20]) == (255, 0, 0, 255) and tuple(filled[0, 0]) == (255, 255, 255, 255)
    deleted = M.delete_selected(white, sel)
    assert deleted[20, 20, 3] == 0 and deleted[0, 0, 3] == 255


def test_grey_fill_and_delete_round_half_away_from_zero():
    layer = np.array([[[10, 20, 30, 40], [255, 255, 255, 255], [1, 1, 1, 1]]], np.uint8)
    sel = np.array([[51, 128, 0]], np.uint8)                     # t = 0.2, 0.50196...
    got = M.fill_selected(layer, sel, (110, 0, 255, 40))
    assert tuple(got[0, 0]) == (30, 16, 75, 40) and tuple(got[0, 2]) == (1, 1, 1, 1)        # 10 * 0.8 + 110 * 0.2 = 30
    assert tuple(M.delete_selected(layer, sel)[0, 0]) == (10, 20, 30, 32)


# ---- one combine rule = the reference's two merges ------------------------------------------------------------------------------------------------------------
def shape_merge_literal(old, v, mode):
    """apply_selection_shape's match, canvas_state.rs:1743-1801, for one pixel inside the box whose contains() is v; outside the box it acts as v = 0"""
    if mode == M.REPLACE:
        new = 0                                  # "Zero the whole mask first"
        if v > 0:
            new = v
        return new
    if mode == M.ADD:
        return max(old, v) if v > 0 else old
    if mode == M.SUBTRACT:
        return max(old - v, 0) if v > 0 else old                 # saturating_sub
    new = 0                                      # intersect: "Zero entire mask first"
    if v > 0 and old > 0:
        new = min(v, old)
    return new


def lasso_merge_literal(old, v, mode):
    """the lasso's match over an existing mask, perspective_gradient.rs:41-86"""
    if mode == M.REPLACE:
        return v
    if mode == M.ADD:
        return 255 if v > 0 else old
    if mode == M.SUBTRACT:
        return 0 if v > 0 else old
    return min(v, old) if v > 0 and old > 0 else 0


@pytest.mark.parametrize("mode", M.MODES)
def test_the_combine_rule_is_both_merges_for_every_base_byte(mode):
    base = np.tile(np.arange(256, dtype=np.uint8), (2, 1))
    raw = np.zeros((2, 256), np.uint8)
    raw[1] = 255
    got = M.combine(base, raw, mode)
    for v_row in (0, 1):
        for old in range(256):
            v = int(raw[v_row, old])
            assert got[v_row, old] == shape_merge_literal(old, v, mode) == lasso_merge_literal(old, v, mode), (mode, old, v)
    # NULL base = all zero
    assert np.array_equal(M.combine(None, raw, mode), M.combine(np.zeros_like(raw), raw, mode))


# ---- casts, parameters ------------------------------------------------------------------------------------------------------------------------------------------
def test_casts_saturate_truncate_and_send_nan_to_zero():
    assert [M.cast_u32(v) for v in (-1.5, 0.99, 2.9, float("nan"), float("inf"), 5e9, -float("inf"))] == [0, 0, 2, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    assert [M.feather_params(r) for r in (-3.0, 0.4, 1.0, 2.9, 5.0, 9.0, 70.0, 512.0)] == [(1, 1), (1, 1), (1, 1), (1, 2), (2, 5), (4, 9), (35, 70), (256, 512)]
    assert M.ellipse_box(100, 100, 50.0, 50.0, 20.0, 20.0) == (30, 30, 70, 70)
    assert M.ellipse_box(100, 80, -5.5, 40.0, 20.7, float("nan")) == (0, 0, 16, 0)        # ceil(15.2) = 16; a NaN sum casts to 0


def test_lasso_rows():
    tri = [(1.0, 0.0), (9.0, 0.0), (1.0, 8.0)]                   # the hypotenuse x = 9 - y
    raw = M.lasso_raw(12, 10, tri)
    assert [int((raw[y] == 255).sum()) for y in range(10)] == [8, 7, 6, 5, 4, 3, 2, 1, 0, 0]   # row y: [1, trunc(9 - (y + 0.5) + 1))
    assert raw[0, 1] == 255 and raw[0, 0] == 0 and raw[0, 8] == 255 and raw[0, 9] == 0
    for n in (0, 1):
        assert not M.lasso_raw(12, 10, tri[:n]).any()
    counts = []
    M.lasso_raw(259, 131, SC.star(259, 131), counts)
    assert max(counts) >= 300                                    # hundreds of crossings in one row


def test_feather_windows_shrink_at_the_edge():
    m = np.zeros((1, 5), np.uint8)
    m[0, 0] = 255
    # r = 1: x = 0 averages 2 pixels (no clamp-replicate: that would give 170), x = 1 averages 3; the 1-row vertical pass changes nothing
    assert M.feather(m, 1.0).tolist() == [[127, 85, 0, 0, 0]]
    assert np.array_equal(M.feather(np.full((7, 9), 255, np.uint8), 70.0), np.full((7, 9), 255, np.uint8))


# ---- the disc as row spans ------------------------------------------------------------------------------------------------------------------------------------------
def check_span(r, k, s):
    assert s >= 0 and s * s <= r * r - k * k < (s + 1) * (s + 1), (r, k, s)


def test_span_table_against_integer_squares():
    for r in list(range(0, 130)) + [1000, M.MORPH_MAX_RADIUS]:
        span = M.span_table(r)
        assert len(span) == r + 1 and span[0] == r and span[r] == 0
        for k in (range(r + 1) if r <= 1000 else list(range(0, r + 1, 997)) + [r - 1, r]):
            check_span(r, k, span[k])


@pytest.mark.parametrize("size", SC.SIZES, ids=SC.size_id)
def test_two_pass_expand_and_contract_equal_the_brute_force(size):
    for name, mask in SC.morph_masks(*size).items():
        for radius in SC.morph_radii(size):
            assert np.array_equal(M.expand_two_pass(mask, radius), SC.morph_expected(size, name, "expand", radius)), (name, radius)
            assert np.array_equal(M.contract_two_pass(mask, radius), SC.morph_expected(size, name, "contract", radius)), (name, radius)


def test_expand_and_contract_rules():
    mask = SC.morph_masks(65, 66)
    assert np.array_equal(M.contract(mask["full"], 17), mask["full"])                    # the canvas edge does not erode
    assert not M.expand(mask["empty"], 17).any()
    ramp = mask["ramp"]
    grown, shrunk = M.expand(ramp, 2), M.contract(ramp, 2)
    assert np.array_equal(grown[ramp > 127], ramp[ramp > 127]) and set(np.unique(grown[ramp <= 127])) <= {0, 1, 127, 255}
    assert np.array_equal(shrunk[shrunk != 0], ramp[shrunk != 0])                        # survivors keep their grey value
    assert np.array_equal(M.expand(ramp, -4), ramp) and np.array_equal(M.contract(ramp, 0), ramp)
    assert M.expand(mask["corners"], SC.BIG_RADIUS)[33, 32] == 255 and M.expand(mask["corners"], 17)[33, 32] == 0


# ---- the library's side (no device needed) ----------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ["pfx_select_rect", "pfx_select_ellipse", "pfx_select_lasso", "pfx_selection_translate", "pfx_selection_feather", "pfx_selection_expand",
                "pfx_selection_contract"]
DEV_ONLY = ["pfx_selection_bounds_dev", "pfx_selection_fill_dev", "pfx_selection_delete_dev"]


@pytest.fixture(scope="module")
def lib():
    from paintfe_amd import _lib
    return _lib.load()


def test_the_abi_declares_and_exports_every_entry_point(lib):
    header = open(os.path.join(ROOT, "include", "pfx.h")).read()
    for name in ENTRY_POINTS + [n + "_dev" for n in ENTRY_POINTS] + DEV_ONLY:
        assert re.search(r"\bint\s+%s\s*\(\s*pfx_ctx\s*\*\s*ctx\b" % name, header), name
        fn = getattr(lib, name)                                  # AttributeError = not exported
        fn.restype = C.c_int
    zero, null = C.c_uint32(0), C.c_void_p(None)
    assert lib.pfx_selection_bounds_dev(null, null, zero, zero, null) != 0             # a NULL context is an error, not a fault
    assert lib.pfx_selection_expand(null, null, zero, zero, C.c_int32(0), null) != 0


def test_the_library_builds_the_same_span_table():
    from paintfe_amd import select_span
    for r in (0, 1, 2, 5, 17, 70, 1000, M.MORPH_MAX_RADIUS):
        span = M.span_table(r)
        for k in (range(r + 1) if r <= 1000 else list(range(0, r + 1, 997)) + [r - 1, r]):
            assert select_span(r, k) == span[k], (r, k)
    assert select_span(5, 6) == -1 and select_span(M.MORPH_MAX_RADIUS + 1, 0) == -1
