"""tests/warp_cases.py reaches the kernel states it was written for: computed on the CPU from the tables, the kernels' compile-time shape
(pfx_int_warp_info) and the oracle alone.  No GPU."""
import numpy as np
import pytest

from . import oracle_lib as O
from . import warp_cases as WC

f32 = np.float32


def oracle_mesh(row):
    (w, h), (cols, rows) = row.size, row.grid
    orig, deformed = WC.mesh_points(row)
    field = O.mesh_displacement_fast(deformed, cols, rows, w, h) if orig is None else O.mesh_displacement(orig, deformed, cols, rows, w, h)
    return field, O.warp_displacement(WC.source(w, h), field)


def test_constants_are_the_ones_the_tables_were_checked_with():
    """the tables follow the constants; this only says which values the figures in the docstrings belong to"""
    c = WC.consts()
    assert c.walk <= 64 and c.wx in (1, 2, 4) and c.dab_cull == 64
    if (c.walk, c.wx, c.xcd_rows) == (48, 4, 16):
        assert WC.sizes() == [(70, 721), (130, 769), (257, 1105), (300, 1009), (1, 800), (2, 730), (65, 47)]
        assert WC.band_cases() == (130, 1500, [(0, 721), (37, 800), (699, 801), (1499, 1)])


def test_sizes_sit_on_the_launch_forms_they_name():
    c, t = WC.consts(), WC.tile_rows()
    s = WC.sizes()
    gy = [WC.tile_grid(w, h)[1] for (w, h) in s]
    assert gy[0] == c.xcd_rows and s[0][1] - (gy[0] - 1) * t == 1            # the threshold exactly, the last tile row 1 pixel row high
    assert gy[1] == c.xcd_rows + 1
    assert WC.tile_grid(*s[2]) == (2, c.xcd_rows + 8) and s[2][0] - WC.tile_cols() == 1   # the second tile column 1 pixel wide
    assert gy[3] == c.xcd_rows + 6
    assert s[4][0] == 1 and s[5][0] == 2 and gy[4] >= c.xcd_rows and gy[5] >= c.xcd_rows   # non-PAIR and the least PAIR width, both in XCD order
    assert gy[6] == 1 and s[6][0] < WC.tile_cols() and not WC.takes_xcd_order(s[6][1])
    assert all(WC.takes_xcd_order(h) for (w, h) in s[:6])
    assert any(h % c.walk for (w, h) in s) and any(w % 64 for (w, h) in s)


def test_xcd_partition_covers_every_tile_row_once_and_some_parts_return_early():
    ragged = 0
    for (w, h) in WC.sizes()[:6]:
        gx, gy = WC.tile_grid(w, h)
        parts = WC.xcd_parts(gy)
        assert parts[0][0] == 0 and parts[-1][1] == gy and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        lens = [r1 - r0 for r0, r1 in parts]
        assert min(lens) >= 1 and max(lens) <= -(-gy // 8)                 # every block of the launch 8 * ceil(gy / 8) * gx finds its part or returns
        launched, used = 8 * -(-gy // 8) * gx, sum(lens) * gx
        assert used == gx * gy and launched >= used
        if min(lens) < max(lens):
            ragged += 1
            assert launched > used                                            # blocks that return at once
    assert ragged >= 3
    assert any(WC.tile_grid(w, h)[1] % 8 == 0 for (w, h) in WC.sizes()[:6])  # and the even split


def test_walks_inside_one_cell_row_and_walks_across_two():
    rows = WC.mesh_rows()
    for size in WC.sizes():
        kinds = {row.grid: WC.walk_kinds(size[1], row.grid[1]) for row in rows if row.size == size}
        assert any(one and not two for one, two in kinds.values())            # (1, 1): every walk in one cell row
        if size[1] > WC.consts().walk:
            assert any(one and two for one, two in kinds.values()), size      # both forms in one launch
        assert kinds[(3, 200)][1] >= size[1] // WC.consts().walk > 0 or size[1] <= 200   # cell rows narrower than a walk: every full walk straddles
    w, h_full, bands = WC.band_cases()
    for first, n in bands[:3]:
        one, two = WC.walk_kinds(n, 6, first, h_full)
        assert one and two, (first, n)


def test_grids_sit_on_both_sides_of_the_lds_boundary_and_on_the_cap():
    p = WC.consts().lds_pts
    n = sorted(WC.n_points(g) for g in WC.grids())
    assert p in n and p + 1 in n and n[0] == 4
    assert {WC.n_points(g) for g in WC.CAP_GRIDS} == {2 * (WC.MAX_CELLS + 1)} and all(max(g) == WC.MAX_CELLS for g in WC.CAP_GRIDS)
    rows = WC.mesh_rows()
    for grid in WC.grids() + WC.CAP_GRIDS:
        assert {r.form for r in rows if r.grid == grid} == set(WC.FORMS), grid
    for size in WC.sizes():
        assert {r.form for r in rows if r.size == size} == set(WC.FORMS), size
        assert {r.deform for r in rows if r.size == size} == set(WC.DEFORMS), size
        assert {r.grid for r in rows if r.size == size} >= set(WC.grids())
    assert all(r.size == WC.small_size() for r in rows if r.grid in WC.CAP_GRIDS)
    for side in (0, WC.IN_LDS):                                              # fold, coincident and a NaN point on either side of the boundary
        assert {"fold", "coincident", "nan"} <= {r.deform for r in rows if WC.mesh_flags(r, 1, 1) & WC.IN_LDS == side}


def test_nonuniform_original_grids_are_not_the_identity_surface():
    for row in WC.mesh_rows():
        orig, deformed = WC.mesh_points(row)
        assert deformed.shape == (WC.n_points(row.grid), 2) and deformed.dtype == f32
        if row.form == "nonuniform":
            lat = WC.lattice(row.grid, *row.size).reshape(-1, 2)
            d = np.abs(orig - lat)
            assert (d > 0).mean() > 0.9 and d.max() <= 1.5 + 1e-3
        elif row.form == "uniform":
            assert np.array_equal(orig, WC.lattice(row.grid, *row.size).reshape(-1, 2))
        else:
            assert orig is None
        if row.deform in WC.NONFINITE:
            bad = ~np.isfinite(deformed) | (np.abs(deformed) >= 3e9)
            assert bad.sum() == 1


@pytest.mark.parametrize("size", WC.sizes(), ids=str)
def test_jitter_and_fold_rows_are_not_vacuous(size):
    """the oracle's result has 5 % to 60 % transparent pixels (samples leave the image, and most do not) and differs from the source on more than 90 %"""
    src = WC.source(*size)
    w, h = size
    seen, sides = 0, np.zeros(4, bool)
    for row in WC.mesh_rows():
        if row.size != size or row.deform not in ("jitter", "fold"):
            continue
        field, out = oracle_mesh(row)
        share, moved = WC.transparent_share(out), float((out != src).any(-1).mean())
        print(f"{row}: transparent {share:.3f}, differs {moved:.4f}")
        assert 0.05 <= share <= 0.60, (row, share)
        assert moved > 0.90, (row, moved)
        fx, fy = WC.sample_floor(field)
        sides |= [(fx < 0).any(), (fx >= w).any(), (fy < 0).any(), (fy >= h).any()]
        seen += 1
    assert seen >= len(WC.grids()) + 1
    assert sides.all() or (w <= 2 and sides[2:].all())      # samples leave on all four sides (0.3 of a width of 1 or 2 does not reach the next texel)


def test_nonfinite_control_points_reach_the_sampler():
    for row in WC.mesh_rows():
        if row.deform not in WC.NONFINITE:
            continue
        field, out = oracle_mesh(row)
        bad = ~np.isfinite(field).all(-1) | (np.abs(field) > 1e6).any(-1)
        assert 0.001 < bad.mean() < 0.9, (row, bad.mean())
        assert bad.mean() <= WC.transparent_share(out) <= 0.9 and (out[bad] == 0).all(), row      # what the point reaches is transparent, the rest mostly not
        field2, out2 = oracle_mesh(row)
        assert WC.same_field(field2, field) and np.array_equal(out, out2)


@pytest.mark.parametrize("size", WC.sizes(), ids=str)
def test_displacement_fields_put_whole_waves_on_every_border_texel(size):
    w, h = size
    for kind, axis in (("border_wave_x", 0), ("border_wave_y", 1)):
        img, disp = WC.field_case(kind, size)
        n = img.shape[1 - axis]
        fl = WC.sample_floor(disp)[axis]
        whole = set()
        for x0 in range(0, w, 64):
            seg = fl[:, x0:x0 + 64]
            whole |= {int(v) for v in seg[(seg == seg[:, :1]).all(1), 0]}
        assert {o for o in WC.BORDER_OFFSETS} | {n + o for o in WC.BORDER_OFFSETS} <= whole, (kind, size)
        other = WC.sample_floor(disp)[1 - axis]
        assert (other >= 0).all() and (other <= img.shape[axis] - 1).all()
    img, disp = WC.field_case("border_px", size)
    fx, fy = WC.sample_floor(disp)
    assert {-2, -1, 0, w - 2, w - 1, w} <= set(fx.ravel().astype(int)) and {-2, -1, 0, h - 2, h - 1, h} <= set(fy.ravel().astype(int))
    img, disp = WC.field_case("random", size)
    out = O.warp_displacement(img, disp)
    assert 0.05 < WC.transparent_share(out) < 0.9
    (a, _), (b, _) = WC.field_case("src_larger", size), WC.field_case("src_smaller", size)
    assert a.shape[0] > h and a.shape[1] > w and b.shape[0] < h and (b.shape[1] < w or w == 1)
    img, disp = WC.field_case("nonfinite", size)
    assert np.isnan(disp).any() and np.isposinf(disp).any() and np.isneginf(disp).any()
    if w >= 64:                                                              # the rest of such a wave samples strictly inside
        plain = (np.isfinite(disp) & (np.abs(disp) < 1e9)).all(-1)
        fx, fy = WC.sample_floor(np.where(plain[..., None], disp, f32(0.25)))
        assert ((fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1))[plain].all() and 8 <= (~plain).sum() <= 24


def reach_counts(dabs, w, h):
    """per pixel, the indices of the dabs that change the oracle's field there (from a start no sum returns to)"""
    hit = np.zeros((len(dabs), h, w), bool)
    for k, d in enumerate(dabs):
        a = np.full((h, w, 2), 1000.0, f32)
        hit[k] = (O.displacement_brush(a.copy(), *d) != a).any(-1)
    return hit


def test_stroke_reaches_pixels_from_every_group_of_the_cull_loop():
    n0 = WC.consts().dab_cull
    (w, h), dabs = WC.STROKE_SIZE, WC.stroke()
    assert len(dabs) == 200 and {d[0] for d in dabs} == {0, 1, 2, 3, 4}
    hit = reach_counts(dabs, w, h)
    assert hit.sum(0).max() > n0
    for edge in range(n0, len(dabs), n0):                                     # 64, 128, 192
        assert (hit[edge - n0:edge].any(0) & hit[edge:edge + n0].any(0)).any(), edge
    fwd, rev = WC.apply_dabs(WC.start_field(w, h), dabs), WC.apply_dabs(WC.start_field(w, h), dabs[::-1])
    assert not np.array_equal(fwd.view(np.uint32), rev.view(np.uint32))       # order matters for these inputs
    assert np.isfinite(fwd).all()


def test_dab_lists_have_the_lengths_and_launches_they_name():
    n0 = WC.consts().dab_cull
    lists = {L.name: L for L in WC.dab_lists()}
    assert len(lists["exactly one trip"].dabs) == n0 and len(lists["one dab into the second trip"].dabs) == n0 + 1
    late = lists["late"]
    assert len(late.dabs) == 300 and not WC.reaches_canvas(late.dabs[:n0], *late.size)
    hit = reach_counts(late.dabs, *late.size)
    assert not hit[:n0].any() and hit[n0:].any(0).sum() > 1000
    for L in WC.dab_lists():
        start = WC.start_field(*L.size)
        assert np.signbit(start).any() and (start == 3.25).any()
        got = WC.apply_dabs(start.copy(), L.dabs)
        same = got.view(np.uint32) == start.view(np.uint32)
        assert same.any() and not same.all() and np.signbit(got[same]).any(), L.name    # untouched -0.0 to keep
    # the spread list takes the chunk launch by pfx_displacement_brushes_dev's rule: at least 256 chunks in the common box, at most half of them touched
    sp = lists["spread"]
    boxes = [WC.dab_box(d, *sp.size) for d in sp.dabs]
    assert all(b[2] > b[0] and b[3] > b[1] for b in boxes)
    bx0, by0, bx1, by1 = min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes)
    assert bx0 % 64 and by0 % 64                                              # the common box does not start on a chunk boundary
    assert any(b[2] % 64 == 0 and b[3] % 64 == 0 and b[2] < sp.size[0] for b in boxes)   # one dab's box ends exactly on one
    touched = {(cx, cy) for b in boxes for cx in range(b[0] >> 6, ((b[2] - 1) >> 6) + 1) for cy in range(b[1] >> 6, ((b[3] - 1) >> 6) + 1)}
    n_all = (((bx1 + 63) >> 6) - (bx0 >> 6)) * (((by1 + 63) >> 6) - (by0 >> 6))
    assert n_all >= 256 and 2 * len(touched) <= n_all
    for L in WC.dab_lists():
        if L.launch == WC.DAB_PLAIN:
            b = [WC.dab_box(d, *L.size) for d in L.dabs]
            b = [x for x in b if x[2] > x[0] and x[3] > x[1]]
            n_box = (((max(x[2] for x in b) + 63) >> 6) - (min(x[0] for x in b) >> 6)) * (((max(x[3] for x in b) + 63) >> 6) - (min(x[1] for x in b) >> 6))
            assert n_box < 256, L.name


def test_oracle_takes_every_row_of_the_single_dab_table():
    """NaN only for a NaN strength, no inf anywhere; the rows that name a reach have it"""
    w, h = WC.EDGE_SIZE
    reached = {}
    for name in WC.EDGE_DABS:
        for mode in range(5):
            d = WC.edge_dab(name, mode)
            start = WC.start_field(w, h)
            got = WC.apply_dabs(start.copy(), [d])
            assert not np.isinf(got).any(), (name, mode)
            assert np.isnan(got).any() == (name == "strength NaN"), (name, mode)
            changed = (got.view(np.uint32) != start.view(np.uint32)).any(-1)
            reached[name, mode] = changed
            if not WC.reaches_canvas([d], w, h):
                assert not changed.any()
    for mode in range(5):
        assert reached["radius 1e9", mode].mean() > 0.9 and reached["radius +inf", mode].mean() > 0.9
        assert reached["centre 3e9", mode].mean() > 0.9 and reached["centre -3e9", mode].mean() > 0.9
        for name in ("centre NaN", "centre NaN y", "centre +inf"):
            assert not reached[name, mode].any()
        # radius 0, -5 and NaN all become 1 (f32::max)
        assert np.array_equal(reached["radius 0", mode], reached["radius -5", mode]) and np.array_equal(reached["radius 0", mode], reached["radius NaN", mode])
        assert 1 <= reached["radius 0", mode].sum() <= 4
    assert reached["dist_sq == r * r", 0][18, 23] and reached["dist_sq == r * r", 0][14, 15] and not reached["dist_sq == r * r", 0][18, 24]
    assert not reached["dist_sq == r * r", 0][14, 25]                       # dist_sq == r * r as well, but x1 = ceil(cx + r) is exclusive
    for name, (x0, y0, x1, y1) in {"box one past the left": (-1, 9, 9, 19), "box one past the top": (15, -1, 25, 9), "box one past the right": (w - 9, 9, w + 1, 19),
                                   "box one past the bottom": (15, h - 9, 25, h + 1)}.items():
        cx, cy, r, _ = WC.EDGE_DABS[name]
        assert (int(np.floor(cx - r)), int(np.floor(cy - r)), int(np.ceil(cx + r)), int(np.ceil(cy + r))) == (x0, y0, x1, y1)
    # the strengths that add a zero: +0 turns a -0.0 entry into +0.0, -0.0 leaves it (mode 0: delta * weight keeps the sign pattern apart)
    plus, minus = reached["strength 0", 0], reached["strength -0.0", 0]
    assert plus.any() and minus.any()

