"""Host checks of tests/brush_cases.py: from the table and the CPU oracle alone, each family reaches the state it was written for — the no-op below the
radius skip and paint above it, both sides of the 0.01 gain cut-off, ties under `>=` and `>`, every branch of the tone modes' HSL round trip, NaN stamps
that paint column / row 0 wherever they stand.  The device runs the same rows in tests/test_gpu_brush_edges.py.  Wall time here: about 2 s in all."""
import numpy as np
import pytest

from . import brush_cases as BC

F = np.float32


@pytest.fixture(scope="module")
def oracle():
    from .backends import OracleBackend
    return OracleBackend()


def changed(row, out):
    return int((out != BC.target(row.target, *row.size)).any(-1).sum())


def test_table_is_complete_and_within_its_sizes():
    n = 0
    for fam in BC.FAMILIES:
        rows = BC.rows(fam)
        assert rows, fam
        names = [r.name for r in rows]
        assert len(set(names)) == len(names), fam
        for r in rows:
            n += 1
            w, h = r.size
            assert (w <= 200 and h <= 136) or (w, h) in ((64, 64), (65, 63), (1, 1))
            assert (r.points is None) != (r.line is None)
            assert r.points is None or (r.points.dtype == np.float32 and 1 <= len(r.points) <= 200)
            assert set(r.binning) <= {0, 1} and r.binning[0] == 1
            if r.points is not None and len(r.points) > 64:
                assert r.binning == (1, 0), f"{r}: more than 64 stamps run on both kernels"
    assert {r.brush["size"] for r in BC.rows("size") if r.size == (BC.W, BC.H)} == set(BC.SIZES)
    assert {len(r.points) for r in BC.rows("count")} == set(BC.COUNTS)
    print(f"{n} rows")


def test_the_skip_sits_between_0_0632_and_0_0633():
    """radius^2 < 0.001 in f32 (brush_render.rs:198): the exact pair"""
    def radius_sq(size):
        r = F(size) / F(2)
        return r * r
    assert radius_sq(0.06) < F(0.001) and radius_sq(0.0632) < F(0.001)
    assert not radius_sq(0.0633) < F(0.001) and not radius_sq(0.07) < F(0.001)
    print(f"radius^2: 0.0632 -> {radius_sq(0.0632)!r}, 0.0633 -> {radius_sq(0.0633)!r}, 0.001f = {F(0.001)!r}")
    # the first f32 size on the painting side, and its lower neighbour on the other
    s = F(0.0632)
    while radius_sq(s) < F(0.001):
        s = np.nextafter(s, F(1))
    assert F(0.0632) < s <= F(0.0633) and radius_sq(np.nextafter(s, F(0))) < F(0.001)


def test_size_rows_paint_above_the_skip_and_nothing_below(oracle):
    seen = set()
    for row in BC.rows("size"):
        if row.brush["is_eraser"] or row.brush["mode"]:
            continue
        n = changed(row, BC.run(oracle, row))
        seen.add(row.brush["size"])
        if row.expect.get("noop"):
            assert n == 0, f"{row}: {n} pixels changed below the skip"
        else:
            assert n >= row.expect["min_painted"], f"{row}: {n} pixels changed"
        if row.brush["size"] == 5000.0 and row.size != (1, 1):
            below = int((BC.target(row.target, *row.size)[..., 3] < 100).sum())   # the stroke's alpha is 173 at the centre line, less with hardness < 1
            assert below > 0.35 * row.size[0] * row.size[1] and n >= below, f"{row}: covers the canvas"
    assert seen == set(BC.SIZES)


def test_gain_rows_split_at_the_cut_off(oracle):
    for (a, flow, painted) in BC.GAINS:   # the label is the f32 product's side of 0.01f (geometry 1.0 at a stamp's centre)
        assert bool(F(1.0) * F(a) * F(flow) >= F(0.01)) == painted, (a, flow)
    assert any(p for *_, p in BC.GAINS) and any(not p for *_, p in BC.GAINS)
    for row in BC.rows("gain"):
        n = changed(row, BC.run(oracle, row))
        assert (n > 0) == row.expect["painted"], f"{row}: {n} pixels changed"


def test_count_rows_cover_the_switch_and_every_cull_group():
    for n in (63, 64, 65, 127, 128, 129, 193):
        assert n in BC.COUNTS
    p = BC.stroke(193)
    assert (p[:, 0] < 0).any() or (p[:, 0] >= BC.W).any() or (p[:, 1] < 0).any() or (p[:, 1] >= BC.H).any()
    assert len({(int(x) // 64, int(y) // 64) for x, y in p if 0 <= x < BC.W and 0 <= y < BC.H}) >= 6   # the stroke visits every chunk kind


def disc(row, cx, cy, shrink=0.0):
    w, h = row.size
    yy, xx = np.mgrid[0:h, 0:w]
    r = row.brush["size"] / 2.0 - shrink
    return (xx - float(cx)) ** 2 + (yy - float(cy)) ** 2 <= r * r


def test_order_rows_have_ties(oracle):
    for row in BC.rows("order"):
        tgt = BC.target(row.target, *row.size)
        cover = sum(disc(row, cx, cy).astype(int) for cx, cy in row.points[:7])
        assert (cover >= 2).sum() > 100, f"{row}: stamps overlap"
        gain = F(1.0) * F(row.brush["color"][3]) * F(row.brush["flow"])
        if row.expect["ties"] == "paint":
            a8 = int(gain * F(255.0))
            tied = (tgt[..., 3] == a8) & (cover >= 1)
            assert tied.sum() >= 4, f"{row}: lattice pixels at a8 = {a8} under a stamp"
            # every later stamp on a pixel ties with the one before it: the stroke backwards leaves other colours
            back = BC.Row(row.family, row.name, row.size, row.target, row.brush, row.points[::-1].copy(), dyn=row.dyn)
            assert not np.array_equal(BC.run(oracle, row), BC.run(oracle, back))
            out = BC.run(oracle, row)
            assert (out[tied][:, 3] == a8).all() and (out[tied][:, :3] != tgt[tied][:, :3]).any(), "a tie overwrites the colour"
        else:
            assert gain == F(128.0) / F(255.0)   # strength == old mask for lattice alpha 128: `>` leaves the pixel
            tied = (tgt[..., 3] == 128) & (cover >= 1)
            assert tied.sum() >= 4
            out = BC.run(oracle, row)
            assert np.array_equal(out[tied], tgt[tied]), "a tie leaves the pixel"
            below = (tgt[..., 3] == 127) & (cover >= 1)
            assert (out[below][:, :3] == 0).all() and below.sum() >= 4


def hsl_state(rgb):
    """adjustments.rs:944-974 on bytes, in f32: the branch conditions and h-less quantities"""
    c = rgb.astype(F) / F(255)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    d = mx - mn
    achro = np.abs(d) < F(1e-6)
    l = (mx + mn) / F(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(achro, F(0), np.where(l > F(0.5), d / (F(2) - mx - mn), d / (mx + mn))).astype(F)
        is_r = ~achro & (np.abs(mx - r) < F(1e-6))
        is_g = ~achro & ~is_r & (np.abs(mx - g) < F(1e-6))
        is_b = ~achro & ~is_r & ~is_g
        h_neg = is_r & ((g - b) / d < 0)
    return dict(achro=achro, is_r=is_r, is_g=is_g, is_b=is_b, h_neg=h_neg, l=l, s=s)


def test_tone_rows_take_every_hsl_branch(oracle):
    """stamp by stamp through the oracle; inside a stamp's disc (a pixel in from its edge) a hardness-1 brush has geometry 1.0 and the strength is exact"""
    checked = 0
    for row in BC.rows("tone"):
        if not row.expect["branches"]:
            continue
        checked += 1
        strength = (F(1.0) * F(row.brush["color"][3]) * F(row.brush["flow"])) * F(0.5)
        mode = row.brush["mode"]
        img = BC.target(row.target, *row.size)
        taken = dict.fromkeys(["achro", "is_r", "is_g", "is_b", "h_neg", "q_low", "q_high", "s_zero_out", "clamp"], 0)
        for cx, cy in row.points:
            inside = disc(row, cx, cy, shrink=1.0)
            st = hsl_state(img[..., :3])
            l2 = np.clip(st["l"] + strength, 0, 1) if mode == 1 else (np.clip(st["l"] - strength, 0, 1) if mode == 2 else st["l"])
            s2 = np.clip(st["s"] - strength, 0, 1) if mode == 3 else st["s"]
            chroma_out = np.abs(s2) >= F(1e-6)
            for k in ("achro", "is_r", "is_g", "is_b", "h_neg"):
                taken[k] += int((st[k] & inside).sum())
            taken["q_low"] += int((chroma_out & (l2 < F(0.5)) & inside).sum())
            taken["q_high"] += int((chroma_out & ~(l2 < F(0.5)) & inside).sum())
            taken["s_zero_out"] += int((~chroma_out & ~st["achro"] & inside).sum())
            raw = st["l"] + strength > 1 if mode == 1 else (st["l"] - strength < 0 if mode == 2 else st["s"] - strength < 0)
            taken["clamp"] += int((raw & inside).sum())
            step = BC.Row(row.family, row.name, row.size, row.target, row.brush, np.array([[cx, cy]], np.float32))
            nxt = BC.run(oracle, step, tgt=img)
            assert np.array_equal(nxt[~disc(row, cx, cy, shrink=-2.0)], img[~disc(row, cx, cy, shrink=-2.0)])
            img = nxt
        print(row, taken)
        need = ["achro", "is_r", "is_g", "is_b", "h_neg", "q_low", "q_high", "clamp"] + (["s_zero_out"] if mode == 3 else [])
        for k in need:
            assert taken[k] > 0, f"{row}: branch {k} never taken"
        assert np.array_equal(img, BC.run(oracle, row)), "stamp by stamp is the stroke"
    assert checked == 6
    c = BC.lattice_colors()
    assert len({tuple(x) for x in c if x[0] == x[1] == x[2]}) == 256
    for p in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)):
        assert (c == p).all(-1).any()
    spread = c.max(-1).astype(int) - c.min(-1)
    assert (spread == 1).sum() >= 30
    lum = (c.max(-1).astype(int) + c.min(-1)) / 510.0
    assert ((lum < 0.5) & (spread > 1)).any() and ((lum > 0.5) & (spread > 1)).any()


def test_tip_rows_cover_the_stated_masks_and_rotations():
    rows = BC.rows("tip")
    sizes = {r.dyn["tip_mask"].shape[0] for r in rows}
    assert set(BC.TIP_SIZES) <= sizes and max(sizes) > max(BC.W, BC.H)
    assert {r.dyn.get("tip_rotation") for r in rows} >= set(BC.TIP_ROTATIONS)
    # 0.0099 and 0.0101 straddle `abs(rotation) > 0.01` in f32
    assert not abs(F(0.0099)) > F(0.01) and abs(F(0.0101)) > F(0.01)
    lo, hi = next(r.dyn["tip_rotation_range"] for r in rows if r.name == "random-rotation-no-range")
    assert abs(F(hi) - F(lo)) < F(0.01) and F(hi) != F(lo)
    assert any(r.brush["is_eraser"] for r in rows) and any(not r.brush["is_eraser"] for r in rows)
    for kind in ("zeros", "full", "texel"):
        m = BC.tip_mask(kind, 33)
        assert {"zeros": (m == 0).all(), "full": (m == 255).all(), "texel": (m > 0).sum() == 1}[kind]


def test_tip_rows_paint_unless_the_mask_is_empty(oracle):
    for row in BC.rows("tip"):
        if row.dyn["tip_mask"].shape[0] == 300 and row.name.endswith("rotation-45.0"):
            continue
        n = changed(row, BC.run(oracle, row))
        assert (n > 0) == row.expect["painted"], f"{row}: {n} pixels changed"


def test_nonfinite_rows_nan_paints_column_or_row_zero_wherever_it_stands(oracle):
    """brush_render.rs:208-215: `floor().max(0.0) as u32` and `ceil() as u32` send a NaN centre to column (row) 0 and no distance test rejects NaN, so the
    stamp paints there.  The oracle must show that for every placement, or the device rows would hold the library to nothing"""
    rows = BC.rows("nonfinite")
    assert {r.expect["place"] for r in rows} == {"first", "middle", "last"} and {r.expect["n"] for r in rows} == {3, 70}
    assert {len(r.points) for r in rows} == {3, 70}
    n_checked = 0
    for row in rows:
        if not (row.expect["nan"] and row.name.endswith("-paint")):
            continue
        bad = row.expect["bad"]
        finite = BC.Row(row.family, row.name, row.size, row.target, row.brush, BC.NONFINITE_FINITE[row.expect["n"]])
        with_nan, without = BC.run(oracle, row), BC.run(oracle, finite)
        diff = (with_nan != without).any(-1)
        assert diff.any(), f"{row}: the NaN stamp paints"
        ys, xs = np.nonzero(diff)
        if np.isnan(bad[0]):
            assert (xs == 0).all(), f"{row}: only column 0"
        if np.isnan(bad[1]):
            assert (ys == 0).all(), f"{row}: only row 0"
        n_checked += 1
    assert n_checked == 2 * 3 * 3
    # +-inf and +-3e9 centres touch nothing (paint, round tip)
    for row in rows:
        if row.expect["nan"] or not row.name.endswith("-paint"):
            continue
        finite = BC.Row(row.family, row.name, row.size, row.target, row.brush, BC.NONFINITE_FINITE[row.expect["n"]])
        assert np.array_equal(BC.run(oracle, row), BC.run(oracle, finite)), f"{row}"


def test_selection_rows_mask_the_borders(oracle):
    for row in BC.rows("selection"):
        sel = BC.selection(row.selection, row)
        w, h = row.size
        assert (sel[:, 63] == 0).all() and (sel[:, 64] == 0).all() and (sel[63, :] == 0).all() and (sel[64, :] == 0).all()
        assert (sel[0] == 0).all() and (sel[:, w - 1] == 0).all()
        assert 0.5 < (sel > 0).mean() < 0.95
        if row.dyn is None:
            for cx, cy in row.points[:4]:
                x0, x1, y0, y1 = BC.stamp_box(row, cx, cy)
                if 0 <= x0 < w and 0 <= y0 < h:
                    assert sel[y0, x0] == 0
        out = BC.run(oracle, row)
        tgt = BC.target(row.target, w, h)
        assert np.array_equal(out[sel == 0], tgt[sel == 0])
        assert changed(row, out) > 0, f"{row}"


def test_line_rows_end_on_and_off_the_canvas(oracle):
    from . import oracle_lib as O
    for (p0, p1, on) in BC.LINES:
        assert (len(O.brush_line_points(p0, p1, 120, 80)) > 0) == on, (p0, p1)
    assert max(len(O.brush_line_points(p0, p1, 120, 80)) for p0, p1, _ in BC.LINES) > 128   # three cull groups
    for row in BC.rows("line"):
        if row.brush["is_eraser"] or row.brush["mode"]:
            continue
        n = changed(row, BC.run(oracle, row))
        if not row.expect["painted"]:
            assert n == 0, f"{row}: {n} pixels changed"
        elif row.brush["size"] >= 1.0:   # a thin soft line's alpha stays under most of the lattice's: shown on an empty preview
            assert BC.run(oracle, row, tgt=BC.target("zeros", *row.size)).any(), f"{row}"


def test_radius_rows_span_the_division_range_with_an_edge_band_on_the_canvas(oracle):
    radii = [r.expect["radius"] for r in BC.rows("radius")]
    assert len(radii) == 64 + 3 * 17
    assert min(radii) >= 0.0316 and max(radii) <= 4096.0 * (1 + 2 ** -23)
    logs = np.log2(np.array(radii[:64]))
    assert (np.histogram(logs, bins=8, range=(np.log2(0.0316), 12.0))[0] >= 2).all(), "the seeded radii spread over the range"
    for row in BC.rows("radius"):
        out = BC.run(oracle, row)
        a = out[..., 3]
        assert (a > 0).sum() >= 1, f"{row}"
        if row.expect["radius"] >= 4:   # partial coverage somewhere: the edge band is on the canvas
            assert ((a > 0) & (a < a.max())).sum() >= 8, f"{row}"
