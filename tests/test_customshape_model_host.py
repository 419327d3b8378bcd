"""tests/customshape_model.py — the yardstick of the device custom-shape rasteriser, since the reference has no golden of these functions — held to two
things (CPU only): a scalar pixel-loop transcription of the reference that hoists and reorders nothing, on boxes of at most 24 x 24, and answers derived by
hand (an axis-aligned square at integer, quarter and half offsets, where the coverages are exactly 0, 1/4, 1/2, 3/4 and 1; a square with a square hole; the
same path listed backwards; the icon of the square at size 8)."""
import numpy as np
import pytest

from . import customshape_cases as CC
from . import customshape_model as CM
from . import shape_model as M

F = np.float32
F32_MAX = M.F32_MAX


# ---- the reference, statement by statement, on numpy float32 scalars (src/ops/shapes.rs) ----
def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def fmax(a, b):   # f32::max
    return b if a != a else (a if b != b else (a if a >= b else b))


def fmin(a, b):   # f32::min
    return b if a != a else (a if b != b else (a if a <= b else b))


def distance_to_segment(px, py, ax, ay, bx, by):                 # :1152
    dx = bx - ax
    dy = by - ay
    len2 = dx * dx + dy * dy
    if len2 <= F(1e-6):
        return np.sqrt((px - ax) * (px - ax) + (py - ay) * (py - ay))
    t = clamp(((px - ax) * dx + (py - ay) * dy) / len2, F(0), F(1))
    cx = ax + dx * t
    cy = ay + dy * t
    return np.sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy))


def distance_to_polylines(px, py, polylines):                    # :1140
    best = F32_MAX
    for poly in polylines:
        for i in range(len(poly) - 1):
            (ax, ay), (bx, by) = poly[i], poly[i + 1]
            best = fmin(best, distance_to_segment(px, py, ax, ay, bx, by))
    return best


def point_in_polylines(px, py, polylines):                       # :1122
    inside = False
    for poly in polylines:
        for i in range(len(poly) - 1):
            (x1, y1), (x2, y2) = poly[i], poly[i + 1]
            denom = y2 - y1
            if abs(denom) > F(1e-6) and ((y1 > py) != (y2 > py)) and (px < (x2 - x1) * (py - y1) / denom + x1):
                inside = not inside
    return inside


def coverage_sample(p, lx, ly, hx, hy, outline_width, fill):     # :1088
    min_x, min_y, max_x, max_y = p["bounds"]
    bw = fmax(max_x - min_x, F(1))
    bh = fmax(max_y - min_y, F(1))
    sx = bw / fmax(hx * F(2), F(1))
    sy = bh / fmax(hy * F(2), F(1))
    px = (lx + hx) * sx + min_x
    py = (ly + hy) * sy + min_y
    inside = point_in_polylines(px, py, p["polylines"])
    fill_cov = F(1) if inside else F(0)
    if fill == "filled":
        return fill_cov
    edge_dist = distance_to_polylines(px, py, p["polylines"]) / fmax(sx, sy)
    outline_cov = F(1) if edge_dist <= fmax(outline_width, F(1)) else F(0)
    return outline_cov if fill == "outline" else fmax(fill_cov, outline_cov)


def scalar_rasterize(s, p, canvas_w, canvas_h):                  # :1169-1305 with custom_shape_data
    x0, y0, bw, bh = box = M.bounds(s, canvas_w, canvas_h)
    buf = np.zeros((bh, bw, 4), np.uint8)
    cos_r, sin_r = M.cosf(s["rotation"]), M.sinf(s["rotation"])
    inv_cos, inv_sin = cos_r, -sin_r
    outline_width = fmax(s["outline_width"], F(0))
    for row in range(bh):
        py_canvas = F(y0 + row) + F(0.5)
        for col in range(bw):
            px_canvas = F(x0 + col) + F(0.5)
            dx = px_canvas - s["cx"]
            dy = py_canvas - s["cy"]
            lx = dx * inv_cos - dy * inv_sin
            ly = dx * inv_sin + dy * inv_cos
            total = F(0)
            for ox, oy in ((F(-0.25), F(-0.25)), (F(0.25), F(-0.25)), (F(-0.25), F(0.25)), (F(0.25), F(0.25))):
                total += coverage_sample(p, lx + ox, ly + oy, s["hw"], s["hh"], outline_width, s["fill"])
            coverage = total * F(0.25)
            if coverage > F(0.001):
                a = fmin(np.floor(F(s["primary"][3]) * coverage + F(0.5)), F(255))   # round(): the product is a non-negative multiple of 1/4, so + 0.5 is exact
                buf[row, col] = (*s["primary"][:3], int(a))
    return buf, box


def scalar_icon(p, size, dark):                                  # :122-155
    out = np.zeros((size, size, 4), np.uint8)
    fg = 235 if dark else 30
    for y in range(size):
        for x in range(size):
            cov = F(0)
            for sy in range(4):
                for sx in range(4):
                    lx = (F(x) + (F(sx) + F(0.5)) * F(0.25)) / F(size) * F(2) - F(1)
                    ly = (F(y) + (F(sy) + F(0.5)) * F(0.25)) / F(size) * F(2) - F(1)
                    cov += coverage_sample(p, lx, ly, F(0.82), F(0.82), F(0.04), "filled")
            cov = clamp(cov / F(16), F(0), F(1))
            if cov > 0:
                v = F(255) * cov
                out[y, x] = (fg, fg, fg, int(np.floor(v + F(0.5))))   # 255 * k / 16 is exact in f32 and never a tie below 255
    return out


SCALAR_CASES = {
    "square_filled_half": (CC.shape("filled", cx=12.5, cy=12.0, hw=4.0, hh=4.0), CC.square_path()),
    "hole_both_rot": (CC.shape("both", cx=12.0, cy=11.5, hw=7.0, hh=6.0, rotation=0.4, outline_width=1.5, primary=(9, 8, 7, 128)), CC.holed_path()),
    "edges_outline": (CC.on_grid_shape("outline", 12.25, 11.75, outline_width=0.5), CC.predicate_edge_path()),
    "edges_both_wide": (CC.on_grid_shape("both", 11.75, 12.25, outline_width=3.0, rotation=1.5707964), CC.predicate_edge_path()),
    "ring_outline_scaled": (CC.shape("outline", cx=11.0, cy=12.0, hw=9.0, hh=3.0, rotation=-0.7, outline_width=1.0, primary=(1, 2, 3, 1)), CC.counted_path(17)),
    "tiny_extent": (CC.shape("both", cx=6.0, cy=6.0, hw=0.3, hh=2.0, outline_width=2.0), CM.path([CC.square(0, 0, 0.5, 0.25)])),
    "open_two_segments": (CC.shape("both", cx=10.0, cy=10.0, hw=6.0, hh=6.0, outline_width=1.0), CC.counted_path(2)),
    "no_segment": (CC.shape("both", cx=10.0, cy=10.0, hw=6.0, hh=6.0, outline_width=40.0), CC.counted_path(0)),
}


@pytest.mark.parametrize("name", sorted(SCALAR_CASES))
def test_model_equals_the_scalar_transcription(name):
    s, p = SCALAR_CASES[name]
    with np.errstate(all="ignore"):
        want, box = scalar_rasterize(s, p, 24, 24)
    got, got_box = CM.rasterize(s, p, 24, 24)
    assert got_box == box and box[2] <= 24 and box[3] <= 24 and box[2] > 0
    assert np.array_equal(got, want)
    if name != "no_segment":
        assert want.any()


@pytest.mark.parametrize("dark", [False, True])
def test_icon_equals_the_scalar_transcription(dark):
    p = CC.holed_path()
    with np.errstate(all="ignore"):
        want = scalar_icon(p, 11, dark)
    assert np.array_equal(CM.icon(p, 11, dark), want) and want.any()


# ---- answers derived by hand ----
# The 8 x 8 square path under hw = hh = 4 has sx = sy = 1 and is inside for 0 <= px < 8 and 0 <= py < 8 (the ray towards +x toggles on the edge x = 8 where
# px < 8 and on the edge x = 0 where px < 0, both for py in [0, 8); the horizontal edges never toggle).  A pixel X of the canvas has its two sample abscissae at
# px = X + 0.5 - cx + 4 -+ 0.25.
def axis_counts(c, n, lo=0.0, hi=8.0, half=4.0):
    """how many of a pixel's two sample coordinates fall in [lo, hi), per canvas pixel 0 .. n - 1, in exact rational arithmetic (quarters)"""
    out = []
    for X in range(n):
        q = [4 * X + 2 - round(4 * c) + round(4 * half) + d for d in (-1, 1)]   # the coordinate in quarters
        out.append(sum(round(4 * lo) <= v < round(4 * hi) for v in q))
    return np.array(out)


def expect_from_counts(counts, box, primary):
    x0, y0, bw, bh = box
    a = primary[3]
    buf = np.zeros((bh, bw, 4), np.uint8)
    quarters = counts[y0:y0 + bh, x0:x0 + bw]
    hit = quarters > 0
    buf[hit, :3] = primary[:3]
    buf[hit, 3] = [int(a * q / 4 + 0.5) for q in quarters[hit]]   # round half away from zero, a * q / 4 >= 0
    return buf


@pytest.mark.parametrize("cx, cy, quarters", [(12.0, 12.0, {0, 4}), (12.5, 12.0, {0, 2, 4}), (12.5, 11.5, {0, 1, 2, 4}), (12.25, 12.75, {0, 2, 4})],
                         ids=["integer", "half_x", "half_both", "quarters"])
def test_axis_aligned_square_by_hand(cx, cy, quarters):
    s = CC.shape("filled", cx=cx, cy=cy, hw=4.0, hh=4.0, primary=(30, 200, 90, 255))
    got, box = CM.rasterize(s, CC.square_path(), 24, 24)
    nx, ny = axis_counts(cx, 24), axis_counts(cy, 24)
    counts = ny[:, None] * nx[None, :]
    assert np.array_equal(got, expect_from_counts(counts, box, s["primary"]))
    assert set(np.unique(counts)) == quarters


def test_one_row_of_the_half_offset_square_written_out():
    s = CC.shape("filled", cx=12.5, cy=12.0, hw=4.0, hh=4.0, primary=(30, 200, 90, 255))
    got, (x0, y0, bw, bh) = CM.rasterize(s, CC.square_path(), 24, 24)
    row = got[12 - y0, :, 3]          # canvas row 12: both sample rows are inside
    # canvas x:  8 is half covered (px = -0.25, 0.25), 9 .. 15 fully, 16 half (px = 7.75, 8.25); the box starts at x0 = floor(12.5 - 4 - 2) = 6
    assert x0 == 6 and list(row[:12]) == [0, 0, 128, 255, 255, 255, 255, 255, 255, 255, 128, 0]
    assert list(got[8 - y0, :12, 3]) == [0, 0, 128, 255, 255, 255, 255, 255, 255, 255, 128, 0] and not got[7 - y0].any()   # integer cy: rows 8 .. 15, all or nothing


def test_square_with_a_square_hole_by_hand():
    # 16 x 16 under hw = hh = 8 (sx = sy = 1): inside the outer [0, 16) x [0, 16) and not inside the hole [5, 11) x [5, 11).  At half offsets the hole's corners
    # give 3/4 and the outer corners 1/4.
    s = CC.shape("filled", cx=16.5, cy=15.5, hw=8.0, hh=8.0, primary=(1, 2, 3, 200))
    got, box = CM.rasterize(s, CC.holed_path(), 40, 40)
    ox, oy = axis_counts(16.5, 40, 0, 16, 8), axis_counts(15.5, 40, 0, 16, 8)
    hx, hy = axis_counts(16.5, 40, 5, 11, 8), axis_counts(15.5, 40, 5, 11, 8)
    counts = oy[:, None] * ox[None, :] - hy[:, None] * hx[None, :]
    assert set(np.unique(counts)) == {0, 1, 2, 3, 4}
    assert np.array_equal(got, expect_from_counts(counts, box, s["primary"]))
    assert set(np.unique(got[..., 3])) == {0, 50, 100, 150, 200}


@pytest.mark.parametrize("fill", ["filled", "outline", "both"])
def test_reverse_segment_order_changes_nothing(fill):
    s = CC.shape(fill, cx=20.0, cy=18.0, hw=15.0, hh=12.0, rotation=0.3, outline_width=2.0)
    p = CC.blob_path(24, 10)
    a, _ = CM.rasterize(s, p, 48, 40)
    b, _ = CM.rasterize(s, CC.reversed_path(p), 48, 40)
    assert np.array_equal(a, b) and a.any()
    assert np.array_equal(CM.segments(CC.reversed_path(p))[::-1][:, [2, 3, 0, 1]], CM.segments(p))


def test_icon_of_the_square_at_size_8_by_hand():
    # lx = (x + k) / 4 - 1 for k in {.125, .375, .625, .875}; inside for 0 <= lx + 0.82 < 1.64, that is 0.72 <= x + k < 7.28: column 0 keeps k = .875 only,
    # column 7 keeps k = .125 only, the rest all four.  No sample is within 0.1 of a bound, far beyond f32 rounding.
    per_axis = np.array([1, 4, 4, 4, 4, 4, 4, 1])
    sixteenths = per_axis[:, None] * per_axis[None, :]
    alpha = np.array([[int(255 * v / 16 + 0.5) for v in r] for r in sixteenths], np.uint8)
    assert alpha[0, 0] == 16 and alpha[0, 1] == 64 and alpha[1, 1] == 255
    for dark, fg in ((True, 235), (False, 30)):
        got = CM.icon(CC.square_path(), 8, dark)
        assert np.array_equal(got[..., 3], alpha) and (got[..., :3] == fg).all()


def test_segments_are_windows_of_every_polyline_in_order():
    p = CM.path([np.array([(0, 0), (1, 0), (1, 1)], F), np.zeros((0, 2), F), np.array([(5, 5)], F), np.array([(2, 2), (3, 3)], F)])
    assert CM.segments(p).tolist() == [[0, 0, 1, 0], [1, 0, 1, 1], [2, 2, 3, 3]]
    assert len(CM.segments(CC.counted_path(0))) == 0 and len(CM.segments(CC.counted_path(65))) == 65 and len(CM.segments(CC.far_and_near_path())) == 1004
