"""tests/effect_cases.py reaches the kernel states it was written for (computed with numpy from the table alone), and the oracle alone stays inside
every cap on it: it finishes every ORACLE row, and on the LIBM rows its two libm flavours differ within the LIBM class."""
import numpy as np
import pytest

from . import effect_cases as EC
from . import libm_cases as LC

f32 = np.float32


def oil_bins(img, levels):
    """artistic.rs:160-166: the intensity level of every pixel"""
    s = img[..., 0].astype(np.uint32) + img[..., 1] + img[..., 2]
    return np.minimum(s // 3 * levels // 256, levels - 1)


def oil_rows():
    return [r for r in EC.rows("oil_painting") if r.expect == EC.ORACLE]


def eff_levels(r):
    return min(max(r.kw["levels"], 2), 64)     # artistic.rs:135-136


def eff_radius(r):
    return min(max(r.kw["radius"], 1), 10)


def test_oil_carry_case_fills_the_packed_word():
    """a 21 x 21 window of white: 441 pixels in one bin, each channel sum 441 * 255 = 112455 — the limits oil_kernel's u64 layout is built on"""
    hit = [r for r in oil_rows() if eff_radius(r) == 10 and "white" in r.kinds]
    assert hit
    for r in hit:
        size = next(s for s in r.sizes if s[0] >= 21 and s[1] >= 21)
        img = EC.content("white", *size)
        win = img[0:21, 0:21]
        bins = oil_bins(win, eff_levels(r))
        assert (bins == bins[0, 0]).all() and bins.size == 441
        assert int(win[..., 0].astype(np.uint32).sum()) == 112455 < (1 << 17)
    assert {eff_levels(r) for r in hit} >= {2, 32, 33, 64}


def test_oil_tie_case_has_two_bins_with_equal_maximal_count():
    hit = [r for r in oil_rows() if "levels2" in r.kinds and r.kw["levels"] == 3]
    assert {eff_radius(r) for r in hit} == {1, 10}
    for r in hit:
        rad = eff_radius(r)
        w, h = next(s for s in r.sizes if s[0] > 2 * rad + 1 and s[1] > 2 * rad + 1)
        bins = oil_bins(EC.content("levels2", w, h), 3)
        y, x = h // 2, w // 2                                        # an interior pixel: no clamped taps
        counts = np.bincount(bins[y - rad:y + rad + 1, x - rad:x + rad + 1].ravel(), minlength=3)
        top = counts.max()
        assert (counts == top).sum() >= 2, counts
        assert len(set(map(tuple, EC.content("levels2", w, h)[y, x - 1:x + 2, :3]))) == 3    # and the tied bins hold different colours


def test_zoom_rows_reach_both_odd_remainders_of_the_group_of_four():
    ns = {max(r.kw["samples"], 2) for r in EC.rows("zoom_blur") if r.expect == EC.ORACLE and not r.kw["strength"] < 0.001}
    assert {n % 4 for n in ns} == {0, 1, 2, 3} and 4096 in ns
    cx = [r.kw["center_x"] for r in EC.rows("zoom_blur")]
    cy = [r.kw["center_y"] for r in EC.rows("zoom_blur")]
    assert min(cx) < 0 and max(cx) > 1 and min(cy) < 0 and max(cy) > 1
    assert any(r.kw["center_x"] * w == int(r.kw["center_x"] * w) and r.kw["center_y"] * h == int(r.kw["center_y"] * h)
               for r in EC.rows("zoom_blur") for (w, h) in r.sizes if r.expect == EC.ORACLE)


def crystal_cells(w, h, cell_size, seed):
    """distort.rs:52-110: the index of the nearest seed point for every pixel (f32 as the reference)"""
    cs = f32(max(cell_size, 2.0))
    cells_x, cells_y = max(int(np.ceil(f32(w) / cs)), 1), max(int(np.ceil(f32(h) / cs)), 1)
    gy, gx = np.mgrid[0:cells_y, 0:cells_x]
    jx = LC.hash24(gx, gy, seed).astype(f32) / f32(16777216.0)
    jy = LC.hash24(gx, gy, (seed + 77) & 0xFFFFFFFF).astype(f32) / f32(16777216.0)
    sx, sy = gx.astype(f32) * cs + jx * cs, gy.astype(f32) * cs + jy * cs
    yy, xx = np.mgrid[0:h, 0:w]
    gcx, gcy = (xx.astype(f32) / cs).astype(np.int64), (yy.astype(f32) / cs).astype(np.int64)
    px, py = xx.astype(f32) + f32(0.5), yy.astype(f32) + f32(0.5)
    best = np.full((h, w), np.inf, f32)
    idx = np.zeros((h, w), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nx, ny = gcx + dx, gcy + dy
            ok = (nx >= 0) & (ny >= 0) & (nx < cells_x) & (ny < cells_y)
            nxc, nyc = np.clip(nx, 0, cells_x - 1), np.clip(ny, 0, cells_y - 1)
            d = (px - sx[nyc, nxc]) ** 2 + (py - sy[nyc, nxc]) ** 2
            take = ok & (d < best)
            best = np.where(take, d, best)
            idx = np.where(take, nyc * cells_x + nxc, idx)
    return idx


def test_crystallize_rows_reach_both_tile_heights_and_both_ends_of_the_block_table():
    rows = [r for r in EC.rows("crystallize") if r.expect == EC.ORACLE and abs(r.kw["cell_size"]) <= 1e4]
    sizes = {max(r.kw["cell_size"], 2.0) for r in rows}
    assert any(np.float32(c) < 8 for c in sizes) and any(np.float32(c) >= 8 for c in sizes) and 8.0 in sizes
    assert max(c for c in sizes if np.float32(c) < 8) >= 7.9 and min(c for c in sizes if c > 8.0) <= 8.1
    per_tile = []
    for r in rows:
        if np.float32(max(r.kw["cell_size"], 2.0)) < 8:
            continue                                                  # 64 x 64 tiles from 8.0 up (k_effects2.hip:pfxk_crystallize)
        for (w, h) in r.sizes:
            cells = crystal_cells(w, h, r.kw["cell_size"], r.kw["seed"])
            for y0 in range(0, h, 64):
                for x0 in range(0, w, 64):
                    per_tile.append(len(np.unique(cells[y0:y0 + 64, x0:x0 + 64])))
    assert max(per_tile) > 32 and min(per_tile) == 1, (max(per_tile), min(per_tile))
    assert max(per_tile) <= 256                                       # half the kernel's 512-slot table


def test_oil_rows_use_more_than_one_column_block_on_both_lane_counts():
    rows = oil_rows()
    assert any(eff_levels(r) <= 32 and w > 256 for r in rows for (w, h) in r.sizes)       # 256 lanes per block
    assert any(eff_levels(r) >= 33 and w > 128 for r in rows for (w, h) in r.sizes)       # 128 lanes per block
    assert {32, 33} <= {eff_levels(r) for r in rows}
    assert any(eff_radius(r) == 10 and h > 32 for r in rows for (w, h) in r.sizes)        # the histogram carried across a 32-row walk and into a second


def test_every_size_class_appears():
    ws, hs = {w for w, _ in EC.SIZES}, {h for _, h in EC.SIZES}
    assert {w % 64 for w in ws} >= {63, 0, 1}
    assert {h % 4 for h in hs} >= {3, 0, 1}
    for edge in (32, 64):                                             # oil painting's 32-row walk, crystallize's 64-row tiles
        assert any(h < edge for h in hs) and edge in hs and any(h > edge for h in hs)
    assert any(w > 256 for w in ws) and any(128 < w <= 256 for w in ws)
    full = [r for e in EC.EFFECTS for r in EC.rows(e) if r.sizes == EC.SIZES]
    # every effect has rows on the whole list, but outline (sizes of its own) and twist (LIBM rows stay off the two smallest images)
    assert {r.effect for r in full} >= set(EC.EFFECTS) - {"outline", "twist"}
    assert all(r.sizes == EC.LIBM_SIZES for r in EC.rows("twist") if r.sizes != [EC.NONFINITE_SIZE]) and len(EC.LIBM_SIZES) == len(EC.SIZES) - 2
    # alpha_bits_kernel's row stride 2 * ceil((w + 32) / 64) + 1: the outline sizes lie on both sides of two steps
    strides = {2 * ((w + 32 + 63) // 64) + 1 for (w, h) in EC.OUTLINE_SIZES}
    assert {3, 5, 7} <= strides
    assert {w + 32 for (w, h) in EC.OUTLINE_SIZES} >= {63, 64, 65, 128, 129}


def test_outline_rows_reach_both_sides_of_the_bit_plane_switch():
    rows = [r for r in EC.rows("outline") if r.expect == EC.ORACLE]
    radii = {max(r.kw["width"], 1) + 1 for r in rows}                  # render.rs:417-418: search radius = ceil(width) + 1
    assert {15, 16, 17, 65, 257} <= radii
    for width in (14, 15, 16):
        assert {(r.kw["mode"], r.kw["anti_alias"]) for r in rows if r.kw["width"] == width} == set(EC.ALL_MODES)
    assert {r.kw["width"] for r in rows if r.tune == ("outline_bits", 0)} == {14, 15}
    assert all(w <= 129 and h <= 65 for r in rows for (w, h) in r.sizes)


def test_every_status_row_names_its_bound_and_every_float_parameter_has_its_six_values():
    for r in EC.all_rows():
        assert (r.expect == EC.STATUS) == bool(r.bound), r
    for effect, params in EC.FLOAT_PARAMS.items():
        rows = [r for r in EC.rows(effect) if r.sizes == [EC.NONFINITE_SIZE]]
        for p in params:
            seen = []
            for r in rows:
                v = r.kw.get(p[0], (0.5, 0.5))[p[1]] if isinstance(p, tuple) else r.kw.get(p, 0.0)
                seen.append(v[0] if isinstance(v, tuple) else v)
            for want in EC.NONFINITE:
                assert any((v != v) if want != want else v == want for v in seen), (effect, p, want)


@pytest.mark.parametrize("effect", EC.EFFECTS)
def test_oracle_finishes_every_oracle_row(effect):
    """each row on its first size and content kind; STATUS rows are never handed to the oracle (it would not return on some)"""
    from .backends import OracleBackend
    oracle = OracleBackend()
    for r in EC.rows(effect):
        if r.expect != EC.ORACLE:
            continue
        (w, h), kind = r.cases()[0]
        out = oracle.effect(effect, EC.content(kind, w, h), mask=EC.selection(w, h), **r.kw)
        assert out.shape == (h, w, 4)


def test_libm_rows_stay_inside_the_libm_class_on_the_oracle_alone():
    """twist and monochrome gaussian noise: the oracle's glibc and device flavours differ by at most 1 on fewer than 0.1 % of channels on every case the
    device test holds to that bar"""
    from . import oracle_lib as O
    rows = [r for r in EC.all_rows() if r.cls == EC.LIBM and r.expect == EC.ORACLE]
    assert {r.effect for r in rows} == {"twist", "add_noise"}
    worst = 0.0
    for r in rows:
        for (w, h), kind in r.cases():
            img = EC.content(kind, w, h)
            ref = getattr(O, r.effect)(img, **r.kw)
            with O.libm_flavour("device"):
                dev = getattr(O, r.effect)(img, **r.kw)
            d = np.abs(ref.astype(np.int16) - dev.astype(np.int16))
            assert d.max() <= 1, (r.effect, r.kw, (w, h), kind)
            share = float((d > 0).mean())
            worst = max(worst, share)
            assert share < 1e-3, (r.effect, r.kw, (w, h), kind, share)
    print(f"LIBM rows: worst share of channels off by one {worst:.2e}")
