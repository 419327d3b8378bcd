"""Bucket fill and magic wand on the device (k_flood.hip) against the CPU model (tests/flood_model.py).  Everything is in the EXACT class: every comparison is
np.array_equal — device against model, host-buffer form against `_dev` form, the fused commit against preview + brush_commit.  The pass-count conditions
follow from the algorithm (a tile converges inside one visit, so a flood crosses one tile border per pass), not from a clock."""
import numpy as np
import pytest

from . import flood_cases as FC
from . import flood_model as M
from .dev_buffers import SENTINEL, DevBuffers

pytestmark = pytest.mark.gpu

NORMAL, MULTIPLY, OVERWRITE = 0, 1, 14


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def pass_cap(w, h):
    return w * h + 2


# ---- the distance map ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("global_scope", [False, True], ids=["contiguous", "global"])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("mode", [M.LEGACY, M.PERCEPTUAL], ids=["legacy", "perceptual"])
def test_distance_map_equals_the_model(gpu, mode, connectivity, global_scope):
    assert gpu.flood_last(2) == FC.TILE     # the sizes of the cases are chosen around this tile edge
    for case in FC.DISTANCE_CASES:
        img, seed, target = FC.case_image(case)
        want = FC.distance_expected(case[0], mode, connectivity, global_scope, False)   # Dijkstra; test_flood_model_host.py holds it to the relaxation
        got = gpu.flood_distance(img, seed, target, mode, connectivity, global_scope)
        assert np.array_equal(got, want), (case[0], int((got != want).sum()))
        if not global_scope:
            assert 1 <= gpu.flood_last(0) < pass_cap(case[1], case[2])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(FC.CORRIDORS))
def test_corridors_cross_tile_borders_dozens_of_times(gpu, name, connectivity):
    img, order = FC.CORRIDORS[name]()
    want = FC.corridor_expected(name, connectivity, False)
    got = gpu.flood_distance(img, order[0], FC.CORRIDOR_TARGET, M.LEGACY, connectivity)
    assert np.array_equal(got, want), int((got != want).sum())
    assert got[order[-1][1], order[-1][0]] == 40
    passes = gpu.flood_last(0)
    assert 2 <= passes < pass_cap(*img.shape[1::-1])
    assert passes <= len(order)      # far below the cap: a pass carries the flood at least to the corridor's next tile border


def test_forms_agree(gpu):
    case = next(c for c in FC.DISTANCE_CASES if c[0] == "130x70-noise-target")
    img, seed, target = FC.case_image(case)
    h, w = img.shape[:2]
    for mode, conn, glob in [(M.LEGACY, 4, False), (M.PERCEPTUAL, 8, False), (M.PERCEPTUAL, 4, True)]:
        want = FC.distance_expected(case[0], mode, conn, glob, False)
        with DevBuffers(gpu, img, np.full((h, w), SENTINEL, np.uint8)) as (d_img, d_dist):
            gpu.flood_distance_dev(d_img, w, h, seed, target, d_dist, mode, conn, glob)
            assert np.array_equal(gpu.dev_download(d_dist, (h, w)), want)
            assert np.array_equal(gpu.dev_download(d_img, img.shape), img)       # src is only read
        assert np.array_equal(gpu.flood_distance(img, seed, target, mode, conn, glob), want)


# ---- pass counts ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_uniform_image_takes_one_pass_per_tile_step(gpu, connectivity):
    tile = gpu.flood_last(2)
    img = FC.uniform(3, 2, tile)
    got = gpu.flood_distance(img, (0, 0), None, M.LEGACY, connectivity)
    assert not got.any()
    passes, visits = gpu.flood_last(0), gpu.flood_last(3)
    farthest = (3 - 1) + (2 - 1)      # Manhattan tile distance from the seed's tile to the farthest one
    assert passes <= farthest + 2, passes        # a per-pixel Jacobi sweep would need about w + h = 320
    assert visits < passes * 6


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("where", sorted(FC.MANY_SEEDS))
def test_uniform_image_of_80_tiles_keeps_many_tiles_in_flight(gpu, where, connectivity):
    assert gpu.flood_last(2) == FC.TILE
    tiles = FC.tile_count(FC.MANY_W, FC.MANY_H)
    got = gpu.flood_distance(FC.uniform_many(), FC.MANY_SEEDS[where], None, M.LEGACY, connectivity)
    assert np.array_equal(got, FC.uniform_many_expected(where, connectivity))      # 0 everywhere: test_flood_model_host.py
    passes, visits = gpu.flood_last(0), gpu.flood_last(3)
    print(where, connectivity, "passes", passes, "visits", visits, "tiles", tiles)
    assert passes <= tiles + 2, passes
    assert visits <= passes * tiles, (visits, passes)
    assert visits > passes, (visits, passes)                          # more than one tile in at least one pass
    assert visits >= tiles                                            # every tile is reached


@pytest.mark.parametrize("global_scope", [False, True], ids=["contiguous", "global"])
@pytest.mark.parametrize("run", FC.MANY_TILE_RUNS, ids=["legacy-4", "perceptual-8"])
@pytest.mark.parametrize("case", FC.MANY_TILE_CASES, ids=[c[0] for c in FC.MANY_TILE_CASES])
def test_many_tiles_equal_the_model(gpu, case, run, global_scope):
    mode, connectivity = run
    img, seed, target = FC.case_image(case)
    want = FC.many_tile_expected(case[0], mode, connectivity, global_scope)
    got = gpu.flood_distance(img, seed, target, mode, connectivity, global_scope)
    assert np.array_equal(got, want), (case[0], int((got != want).sum()))
    if not global_scope:
        print(case[0], run, "passes", gpu.flood_last(0), "visits", gpu.flood_last(3))
        assert 1 <= gpu.flood_last(0) < pass_cap(case[1], case[2])
        assert gpu.flood_last(3) <= gpu.flood_last(0) * FC.tile_count(case[1], case[2])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_walled_in_seed_visits_its_own_tile_only(gpu, connectivity):
    tile = gpu.flood_last(2)
    img = FC.walled(3, 2, tile)
    got = gpu.flood_distance(img, (5, 5), None, M.LEGACY, connectivity)
    want = np.full(img.shape[:2], 255, np.uint8)
    want[:40, :40] = 0
    assert np.array_equal(got, want)
    assert np.array_equal(got, M.distance_map(img, (5, 5), img[5, 5], M.LEGACY, connectivity, False, check=False))
    passes, visits = gpu.flood_last(0), gpu.flood_last(3)
    assert 1 <= passes <= 2 and visits < passes * 6 and visits <= 2     # the active-tile list: the other five tiles are never visited


# ---- masks, boxes, preview --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti_aliased", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("combine", [M.REPLACE, M.ADD, M.SUBTRACT, M.INTERSECT], ids=["replace", "add", "subtract", "intersect"])
def test_wand_mask(gpu, combine, anti_aliased):
    d, base = FC.ramp_distance(), FC.base_mask()
    h, w = d.shape
    for t in FC.THRESHOLDS:
        for b in (None, base):
            want = M.wand_mask(d, t, anti_aliased, combine, b)
            assert np.array_equal(gpu.wand_mask(d, t, anti_aliased, combine, b), want), (t, b is None)
        inplace = base.copy()
        assert gpu.wand_mask(d, t, anti_aliased, combine, inplace, out=inplace) is inplace
        assert np.array_equal(inplace, M.wand_mask(d, t, anti_aliased, combine, base)), t
    if anti_aliased:
        assert (gpu.wand_mask(d, 255, True, M.REPLACE) == 255).all()
    # the device forms: separate output, in place, no base; at an odd offset the kernel's byte path runs
    t = 37
    with DevBuffers(gpu, d, base, np.full((h, w), SENTINEL, np.uint8), d.ravel()[1:], base.ravel()[1:]) as (d_d, d_b, d_o, d_d1, d_b1):
        gpu.wand_mask_dev(d_d, w, h, t, d_o, anti_aliased, combine, d_b)
        assert np.array_equal(gpu.dev_download(d_o, (h, w)), M.wand_mask(d, t, anti_aliased, combine, base))
        gpu.wand_mask_dev(d_d, w, h, t, d_o, anti_aliased, combine)
        assert np.array_equal(gpu.dev_download(d_o, (h, w)), M.wand_mask(d, t, anti_aliased, combine, None))
        gpu.wand_mask_dev(d_d, w, h, t, d_b, anti_aliased, combine, d_b)
        assert np.array_equal(gpu.dev_download(d_b, (h, w)), M.wand_mask(d, t, anti_aliased, combine, base))
        n = w * h - 3
        gpu.wand_mask_dev(d_d1 + 1, n, 1, t, d_b1 + 1, anti_aliased, combine, d_b1 + 1)
        assert np.array_equal(gpu.dev_download(d_b1 + 1, (n,)), M.wand_mask(d.ravel()[2:2 + n], t, anti_aliased, combine, base.ravel()[2:2 + n]))


def test_bboxes(gpu):
    d = FC.ramp_distance()
    late = d.copy()
    late[late < 3] = 3                       # nothing at 0, 1, 2: three "none" boxes
    col = d[:, :1].copy()                    # 1 pixel wide
    for dist in (d, late, col, np.full((3, 300), 9, np.uint8)):
        h, w = dist.shape
        with DevBuffers(gpu, dist) as (d_dist,):
            got = gpu.flood_bboxes_dev(d_dist, w, h)
        assert np.array_equal(got, M.bboxes(dist))
    assert (M.bboxes(late)[:3] == -1).all()


@pytest.mark.parametrize("fill", [(200, 30, 60, 255), (10, 220, 90, 128)], ids=["opaque", "half"])
def test_fill_preview(gpu, fill):
    d, sel = FC.ramp_distance(), FC.selection()
    h, w = d.shape
    for t in (0, 37, 254):
        for s in (None, sel):
            want = M.fill_preview(d, t, fill, s)
            assert 0 < (want[..., 3] > 0).sum() < w * h
            assert np.array_equal(gpu.fill_preview(d, t, fill, s), want), (t, s is None)
    want = M.fill_preview(d, 37, fill, sel)
    with DevBuffers(gpu, d, sel, np.full((h, w, 4), SENTINEL, np.uint8)) as (d_d, d_s, d_o):
        gpu.fill_preview_dev(d_d, w, h, 37, fill, d_o, d_s)
        assert np.array_equal(gpu.dev_download(d_o, (h, w, 4)), want)
    # the preview is what composite_preview takes
    layer = FC.layer()
    gpu.ensure_layer_texture(0, layer, generation=1)
    try:
        shown = gpu.composite_preview(w, h, [(0, 1.0, True, NORMAL)], want, 0, NORMAL)
        plain = gpu.composite(w, h, [(0, 1.0, True, NORMAL)])
    finally:
        gpu.clear_layers()
    assert shown.shape == (h, w, 4) and not np.array_equal(shown, plain)


# ---- commit ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [NORMAL, MULTIPLY, OVERWRITE], ids=["normal", "multiply", "overwrite"])
def test_fused_commit_equals_preview_then_brush_commit(gpu, mode):
    layer, sel = FC.layer(), FC.selection()
    h, w = layer.shape[:2]
    d = M.distance_map(layer, (5, 5), layer[5, 5], M.LEGACY, 4, True, check=False)
    t = M.tolerance_threshold(5.0)
    for fill in [(10, 20, 30, 128), (250, 240, 10, 255), (1, 2, 3, 0)]:
        for s in (None, sel):
            want = gpu.brush_commit(layer, gpu.fill_preview(d, t, fill, s), mode, selection=s)
            assert np.array_equal(want, M.fill_commit(layer, d, t, fill, mode, s))
            with DevBuffers(gpu, layer, d, sel) as (d_l, d_d, d_s):
                gpu.fill_commit_dev(d_l, d_d, w, h, t, fill, mode, d_s if s is not None else 0)
                got = gpu.dev_download(d_l, layer.shape)
            assert np.array_equal(got, want), (fill, s is None)
            if fill[3]:
                assert not np.array_equal(got, layer)
            else:
                assert np.array_equal(got, layer)          # a preview without alpha commits nothing


@pytest.mark.parametrize("global_fill", [False, True], ids=["contiguous", "global"])
def test_bucket_fill_end_to_end(gpu, global_fill):
    layer, sel = FC.layer(), FC.selection()
    for seed, tol, fill, mode, s in [((5, 5), 5.0, (10, 20, 30, 128), NORMAL, None), ((100, 40), 12.0, (250, 240, 10, 255), MULTIPLY, sel),
                                     ((129, 69), 0.0, (0, 0, 255, 255), OVERWRITE, None)]:
        want = M.bucket_fill(layer, seed, tol, fill, mode, global_fill, s, check=False)
        got = gpu.bucket_fill(layer, seed, tol, fill, mode, global_fill, s)
        assert np.array_equal(got, want), (seed, tol)
        d = M.distance_map(layer, seed, layer[seed[1], seed[0]], M.LEGACY, 4, global_fill, check=False)
        filled = d <= M.tolerance_threshold(tol)
        if s is not None:
            filled &= s > 0
        assert 0 < filled.sum() < filled.size
        assert np.array_equal(got[~filled], layer[~filled])      # nothing outside the filled set moves


def test_bucket_fill_of_a_line_through_a_border_seed(gpu):
    """the seed on a tile border, every other pixel of its tile's border at distance 255: the fill must cross the border"""
    for kind, seed in [("hline", (64, 20)), ("hline", (63, 20)), ("cross", (64, 64))]:
        layer = FC.IMAGES[kind](130, 70)
        want = M.bucket_fill(layer, seed, 10.0, (255, 0, 0, 255), NORMAL, False, check=False)
        got = gpu.bucket_fill(layer, seed, 10.0, (255, 0, 0, 255), NORMAL, False)
        assert np.array_equal(got, want), (kind, seed)
        line = (layer[..., 0] == 0)
        assert (got[line] == (255, 0, 0, 255)).all() and np.array_equal(got[~line], layer[~line])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(gpu):
    from paintfe_amd import PfxError
    import ctypes as C
    from paintfe_amd import _lib
    img = FC.noise(70, 40)
    h, w = img.shape[:2]
    d = FC.ramp_distance(w, h)

    def refused(fn, *a, **k):
        with pytest.raises(PfxError) as e:
            fn(*a, **k)
        assert e.value.status == _lib.ERR_INVALID

    with DevBuffers(gpu, img, np.full((h, w), SENTINEL, np.uint8), d, np.full((h, w, 4), SENTINEL, np.uint8)) as (d_img, d_out, d_dist, d_canvas):
        for seed in [(w, 0), (0, h), (2 ** 32 - 1, 0)]:
            refused(gpu.flood_distance_dev, d_img, w, h, seed, (0, 0, 0, 255), d_out)
        refused(gpu.flood_distance_dev, d_img, w, h, (1, 1), (0, 0, 0, 255), d_out, connectivity=5)
        refused(gpu.flood_distance_dev, d_img, w, h, (1, 1), (0, 0, 0, 255), d_out, distance_mode=2)
        refused(gpu.flood_distance_dev, d_img, w, h, (1, 1), (0, 0, 0, 255), d_img + 16)                  # dist inside src
        refused(gpu.flood_distance_dev, d_img, 0, h, (0, 0), (0, 0, 0, 255), d_out)
        refused(gpu.flood_distance_dev, d_img + 2, w, h - 1, (1, 1), (0, 0, 0, 255), d_out)                 # RGBA8 pixels are read as dwords
        refused(gpu.fill_preview_dev, d_dist, w, h - 1, 37, (1, 2, 3, 4), d_canvas + 1)
        refused(gpu.fill_commit_dev, d_canvas + 2, d_dist, w, h - 1, 37, (1, 2, 3, 4), 0)
        refused(gpu.flood_distance_dev, d_img, 20000, 20000, (0, 0), (0, 0, 0, 255), d_out)
        refused(gpu.wand_mask_dev, d_dist, w, h, 37, d_out, combine=4)
        refused(gpu.wand_mask_dev, d_dist, w, h, 37, d_dist)                                              # the mask over its distance map
        refused(gpu.wand_mask_dev, d_dist, w, h - 1, 37, d_out, base_ptr=d_out + w)                       # a base that overlaps the output without being it
        refused(gpu.fill_preview_dev, d_dist, w, h, 37, (1, 2, 3, 4), d_dist)
        refused(gpu.fill_preview_dev, d_dist, w, h, 37, (1, 2, 3, 4), d_canvas, selection_ptr=d_canvas + 8)
        refused(gpu.fill_commit_dev, d_canvas, d_dist, w, h, 37, (1, 2, 3, 4), 25)                        # an unknown blend mode
        refused(gpu.fill_commit_dev, d_canvas, d_canvas + 4, w, h, 37, (1, 2, 3, 4), 0)
        assert (gpu.dev_download(d_out, (h, w)) == SENTINEL).all() and (gpu.dev_download(d_canvas, (h, w, 4)) == SENTINEL).all()
        assert np.array_equal(gpu.dev_download(d_dist, (h, w)), d) and np.array_equal(gpu.dev_download(d_img, img.shape), img)
    out = np.full((h, w), SENTINEL, np.uint8)
    f = _lib.Flood(w, 0, (C.c_uint8 * 4)(0, 0, 0, 255), 0, 4, 0, 0)
    assert gpu._lib.pfx_flood_distance(gpu.handle, img.ctypes.data_as(C.c_void_p), C.c_uint32(w), C.c_uint32(h), C.byref(f), out.ctypes.data_as(C.c_void_p)) == _lib.ERR_INVALID
    assert (out == SENTINEL).all()
    layer = img.copy()
    refused(gpu.bucket_fill, layer, (w, 3), 10.0, (1, 2, 3, 255))
    refused(gpu.bucket_fill, layer, (3, 3), 10.0, (1, 2, 3, 255), blend_mode=99)
    # the context still floods
    assert np.array_equal(gpu.flood_distance(img, (3, 3), None, M.LEGACY, 4), M.distance_map(img, (3, 3), img[3, 3], M.LEGACY, 4, False, check=False))
