"""Host checks of tests/resize_model.py: the window restatement against hand-worked cases and against the oracle (an impulse image shows which source
columns carry weight), and the case tables of tests/test_gpu_resample_edges.py against what they were written for — tile-edge output sizes, tap counts
of every residue mod 4, spans of 511 / 512 / 513 source columns, and affine translations whose samples land exactly on every border."""
import ctypes as C

import numpy as np
import pytest

from . import oracle_lib as O
from . import resize_model as M

F = np.float32


def test_build_axis_by_hand():
    # 8 -> 4 bilinear: ratio 2, support 2; centres 1, 3, 5, 7: [floor(c - 2), ceil(c + 2)) clamped to [0, 8)
    left, count = M.build_axis(8, 4, "bilinear")
    assert left.tolist() == [0, 1, 3, 5] and count.tolist() == [3, 4, 4, 3]
    # 4 -> 8 bilinear: ratio 0.5, support 1; centres 0.25, 0.75, ..: [floor(c - 1), ceil(c + 1))
    left, count = M.build_axis(4, 8, "bilinear")
    assert left.tolist() == [0, 0, 0, 0, 1, 1, 2, 2] and count.tolist() == [2, 2, 3, 3, 3, 3, 2, 2]
    # nearest: support 0, one tap at floor(centre) (right = max(ceil(c), left + 1))
    left, count = M.build_axis(10, 4, "nearest")
    assert left.tolist() == [1, 3, 6, 8] and count.tolist() == [1, 1, 1, 1]
    # 6 -> 2 bicubic: ratio 3, support 6: both windows are the whole axis
    left, count = M.build_axis(6, 2, "bicubic")
    assert left.tolist() == [0, 0] and count.tolist() == [6, 6]
    # 1 -> 5: every window is the one sample
    for f in M.FILTERS:
        left, count = M.build_axis(1, 5, f)
        assert left.tolist() == [0] * 5 and count.tolist() == [1] * 5
    # span_max and the path rule: 8 tiles rows x span x 16 bytes within 64 KiB <=> span <= 512
    assert M.tile_spans(8, 4, "bilinear") == [8] and M.span_max(200, 130, "nearest") == max(M.tile_spans(200, 130, "nearest"))
    assert 512 * M.TILE_ROWS * 16 == M.LDS_BYTES
    assert M.path(8, 8, 8, 8, "bilinear") == M.COPY and M.path(8, 8, 4, 4, "bilinear") == M.FUSED and M.path(8, 8, 4, 4, "bilinear", two_pass=True) == M.TWO_PASS


@pytest.mark.parametrize("filter", M.FILTERS)
def test_windows_match_the_oracles_through_impulses(filter):
    """a mid-grey source with one white column: the output columns that leave the grey are those whose window holds the column with a weight that shows (a
    lobe may be negative, so the background is not 0).  No weight may show outside the model's window, every window shows in its output, and a window's
    taps are mostly visible (a tap at the open end of the support weighs exactly 0, small lobes round away)"""
    for (n_in, n_out) in ((37, 13), (50, 7), (9, 31), (23, 64), (64, 23), (5, 6)):
        left, count = M.build_axis(n_in, n_out, filter)
        flat = np.full((3, n_in, 4), 128, np.uint8)
        base = O.resize(flat, n_out, 3, filter)
        assert (base == 128).all()
        hit = np.zeros((n_in, n_out), bool)
        for col in range(n_in):
            img = flat.copy()
            img[:, col] = 255
            hit[col] = (O.resize(img, n_out, 3, filter)[1] != 128).any(-1)
        inside = (np.arange(n_in)[:, None] >= left[None, :]) & (np.arange(n_in)[:, None] < (left + count)[None, :])
        assert not (hit & ~inside).any(), f"{filter} {n_in}->{n_out}: weight outside the model's window"
        assert hit.any(0).all()
        visible = (inside & hit).sum(0) / count
        print(f"{filter} {n_in}->{n_out}: visible share of a window's taps {visible.min():.2f} .. {visible.max():.2f}")
        if filter in ("nearest", "bilinear"):   # kernels without lobes: only a window's end taps can weigh nothing (|x| = 1 exactly, or a byte's rounding)
            for o in range(n_out):
                cols = np.nonzero(hit[:, o])[0]
                assert cols[0] - left[o] <= 1 and (left[o] + count[o] - 1) - cols[-1] <= 1, f"{filter} {n_in}->{n_out} column {o}"
                assert filter == "bilinear" or (len(cols) == 1 and count[o] == 1)


def cases(prefix):
    return [c for c in M.resize_cases() if c[0].startswith(prefix)]


def test_resize_cases_reach_what_they_name():
    assert {c[2][0] for c in cases("width-")} == {1, 63, 64, 65, 127, 128, 129}
    assert {c[2][1] for c in cases("height-")} == {1, 7, 8, 9, 15, 16, 17}
    for f in M.FILTERS[1:]:   # nearest has one tap everywhere
        vert, horiz = set(), set()
        for (_, (w, h), (nw, nh), _) in cases("taps-"):
            horiz |= M.tap_residues(w, nw, f)
            vert |= M.tap_residues(h, nh, f)
        assert horiz == {0, 1, 2, 3} and vert == {0, 1, 2, 3}, (f, horiz, vert)
    assert {M.build_axis(37, 13, "nearest")[1].max(), M.build_axis(9, 129, "nearest")[1].max()} == {1}
    for f in M.FILTERS:
        want = {511: M.FUSED, 512: M.FUSED, 513: M.TWO_PASS}
        for span in (511, 512, 513):
            (name, (w, h), (nw, nh), fl), = cases(f"span-{span}-{f}")
            assert fl == [f] and nw == 64 and w < 1100 and h < 40
            assert M.span_max(w, nw, f) == span and M.path(w, h, nw, nh, f) == want[span]
        (name, (w, h), (nw, nh), fl), = cases(f"later-tile-{f}")
        spans = M.tile_spans(w, nw, f)
        assert spans[0] <= 512 < max(spans[1:]) and M.path(w, h, nw, nh, f) == M.TWO_PASS and w < 1100, (f, spans)
        (name, (w, h), (nw, nh), fl), = cases("last-tile-ties")
        spans = M.tile_spans(w, nw, f)
        assert len(spans) == 2 and spans[1] == max(spans) and nw % 64
    print({f: [M._span_width(s, f) for s in (511, 512, 513)] for f in M.FILTERS})
    for (name, (w, h), (nw, nh), fl) in M.resize_cases():
        assert w < 1100 and h <= 100 and nw <= 130 and nh <= 17, name


def test_no_last_partial_tile_is_strictly_the_widest():
    """why the table has no such case: searched over output widths of two and three tiles"""
    for f in M.FILTERS:
        for nw in (65, 100, 127, 129, 191):
            for w in list(range(2, 300)) + list(range(300, 1100, 37)):
                if w == nw:
                    continue
                spans = M.tile_spans(w, nw, f)
                assert spans[-1] <= max(spans[:-1]), (f, w, nw, spans)


# ---------------------------------------------------------------------------------------------------------------------------------- affine
def oracle_matrix(cw, ch, rz=0.0, rx=0.0, ry=0.0):
    hi = np.zeros(9, F)
    O.lib().pfxo_affine_matrix(C.c_uint32(cw), C.c_uint32(ch), C.c_float(rz), C.c_float(rx), C.c_float(ry), hi.ctypes.data_as(C.c_void_p))
    return hi


def test_identity_matrix_restatement_is_the_oracles():
    for (cw, ch) in M.AFFINE_CANVASES:
        assert np.array_equal(np.abs(oracle_matrix(cw, ch)), M.affine_identity_matrix(cw, ch)), (cw, ch)   # the oracle's zeros may be -0


def test_border_offsets_put_samples_exactly_on_every_border():
    """over a source's offsets and the canvases, the restated sample coordinate takes each border target exactly (bilinear: floor = -2, -1, 0, n - 2,
    n - 1, n with fractions 0, .25, .75; nearest: the .5 ties)"""
    for (sw, sh) in M.AFFINE_SOURCES:
        got_x, got_y = set(), set()
        for (cw, ch) in M.AFFINE_CANVASES:
            hi = M.affine_identity_matrix(cw, ch)
            for off in M.border_offsets(sw, sh):
                sx, sy, w = M.affine_coords(hi, cw, ch, offset=off)
                assert (np.abs(w) >= F(1e-8)).all()
                got_x |= set(np.unique(sx).tolist())
                got_y |= set(np.unique(sy).tolist())
        assert set(M.border_targets(sw)) <= got_x, (sw, sorted(set(M.border_targets(sw)) - got_x))
        assert set(M.border_targets(sh)) <= got_y, (sh, sorted(set(M.border_targets(sh)) - got_y))
        for n, got in ((sw, got_x), (sh, got_y)):
            floors = {int(np.floor(v)) for v in got if abs(v) < 1e6}
            assert {-2, -1, 0, n - 2, n - 1, n} <= floors
            assert {-0.5, n - 0.5} <= got   # round half away from zero: -0.5 -> -1 (outside), n - 0.5 -> n (outside)


def test_affine_scales_sit_on_both_sides_of_the_1e_6_test():
    took = {s: bool(abs(F(s)) > F(1e-6)) for s in (9e-7, 1e-6, 1.1e-6, -1e-6, 1e9, 1e-30)}
    print(took)
    assert took[9e-7] is False and took[1.1e-6] is True and took[1e9] is True and took[1e-30] is False
    assert took[1e-6] == took[-1e-6]   # 1e-6 as f32 against the f32 constant 1e-6: equal, so `>` is false


def test_right_angle_rotations_have_pixels_on_both_sides_of_the_w_test():
    """M.W_ZERO_CASES on their canvas: |w| < 1e-8 for one whole row (rotation_x) or column (rotation_y) and for no other pixel; the same rotations
    without the offset have no such pixel (the zero of w lies between pixel centres)"""
    cw, ch = M.W_ZERO_CANVAS
    for kw in M.W_ZERO_CASES:
        rx, ry = kw.get("rotation_x", 0.0), kw.get("rotation_y", 0.0)
        hi = oracle_matrix(cw, ch, rx=rx, ry=ry)
        sx, sy, w = M.affine_coords(hi, cw, ch, offset=kw["offset"])
        small = np.abs(w) < F(1e-8)
        assert small.sum() == (cw if rx else ch), (kw, int(small.sum()))
        assert small.all(1).sum() == 1 if rx else small.all(0).sum() == 1
        sx, sy, w = M.affine_coords(hi, cw, ch)
        assert not (np.abs(w) < F(1e-8)).any()
    assert all(k in M.affine_param_cases() for k in M.W_ZERO_CASES)


def test_the_singular_branch_of_invert_3x3_is_reachable_only_on_tiny_canvases():
    """|det| < 1e-12 -> identity: det = focal^3 cos(rx) cos(ry) with rotation_z = 0; two right angles give 1.9e-15 focal^3, below 1e-12 while
    focal = 1.5 max(w, h) < 8, i.e. canvases up to 5 x 5 — the 1 x 1 canvas of the table; from 63 x 3 up the matrix is inverted"""
    assert np.array_equal(oracle_matrix(1, 1, rx=90.0, ry=90.0), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F))
    assert not np.array_equal(oracle_matrix(63, 3, rx=90.0, ry=90.0), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F))
    assert not np.array_equal(oracle_matrix(1, 1, rx=90.0), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F))
