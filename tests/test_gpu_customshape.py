"""The device custom-shape rasteriser and the picker icon (k_customshape.hip) against tests/customshape_model.py (GPU).  Everything at tolerance 0, no pixel
left out.  The reference has no golden of these functions: the model is the yardstick, and tests/test_customshape_model_host.py holds the model.

The cases are the smallest at which the kernel can go wrong: segment counts around a wave, a batch (B) and a full LDS list (L) — both read from the library —,
boxes around the 64 x 4 tile, rotations (a tile's samples are then not axis-aligned in path space, which the y-cull must survive), samples exactly on vertices
and intercepts, degenerate segments, a path with a thousand segments far from the box, every fill mode and outline widths up to wider than a tile."""
import ctypes as C
import math

import numpy as np
import pytest

from . import customshape_cases as CC
from . import customshape_model as CM
from . import shape_cases as SC
from . import shape_model as M

pytestmark = pytest.mark.gpu
F = np.float32
NORMAL, MULTIPLY, XOR, OVERWRITE = 0, 1, 13, 14   # BlendMode::to_u8
W, H = CC.CANVAS_W, CC.CANVAS_H


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def cpath(p):
    from paintfe_amd import CustomPath
    return CustomPath(p["polylines"], p["bounds"])


def check(gpu, s, p, w=W, h=H, what=""):
    """box buffer and preview against the model; returns the buffer"""
    want, box = CM.rasterize(s, p, w, h)
    got, got_box = gpu.rasterize_custom_shape(SC.to_api(s), cpath(p), w, h)
    assert got_box == box and got.shape == want.shape, what
    bad = int((got != want).any(-1).sum())
    assert bad == 0, f"{what}: {bad} of {want.shape[0] * want.shape[1]} box pixels differ from the model"
    assert np.array_equal(gpu.custom_shape_preview(SC.to_api(s), cpath(p), w, h), M.to_canvas(want, box, w, h)), f"{what}: preview"
    return got


def test_segments_are_the_models(gpu):
    for p in (CC.counted_path(0), CC.counted_path(2), CC.holed_path(), CC.predicate_edge_path(), CC.far_and_near_path()):
        assert np.array_equal(gpu.custom_shape_segments(cpath(p)), CM.segments(p))


def segment_counts(gpu):
    b, l = gpu.customshape_info(0), gpu.customshape_info(1)
    assert b >= 64 and l >= b and 2 * b + 1 <= 1100 and l + 1 <= 1100
    return sorted({0, 1, 2, 63, 64, 65, b - 1, b, b + 1, 2 * b + 1, l - 1, l, l + 1})


@pytest.mark.parametrize("fill, rotation", [("filled", 0.0), ("both", 0.3), ("outline", -1.2)])
def test_segment_counts_around_a_wave_a_batch_and_a_list(gpu, fill, rotation):
    s = CC.shape(fill, cx=40.0, cy=16.0, hw=33.0, hh=7.0, rotation=rotation, outline_width=2.0)
    drew = 0
    for n in segment_counts(gpu):
        p = CC.counted_path(n, seed=n)
        assert len(CM.segments(p)) == n
        drew += bool(check(gpu, s, p, 96, 64, f"{n} segments").any())
    assert drew >= 10


@pytest.mark.parametrize("bh", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("bw", [1, 63, 64, 65, 129])
def test_box_sizes_around_the_tile(gpu, bw, bh):
    # the shape covers the whole canvas, so the box is the canvas
    s = CC.shape("both", cx=bw * 0.5 + 0.25, cy=bh * 0.5, hw=90.0, hh=12.0, rotation=0.1, outline_width=1.5)
    p = CC.blob_path(48, 16)
    assert M.bounds(s, bw, bh) == (0, 0, bw, bh)
    check(gpu, s, p, bw, bh, f"{bw}x{bh}")


@pytest.mark.parametrize("bw", [63, 64, 65, 129])
def test_unclipped_box_widths(gpu, bw):
    s = CC.shape("both", cx=100.5 if bw % 2 else 100.0, cy=60.5, hw=(bw - 4) / 2, hh=10.5, outline_width=1.0)
    assert M.bounds(s, W, H)[2:] == (bw, 25)
    assert check(gpu, s, CC.blob_path(48, 16), what=f"width {bw}").any()


@pytest.mark.parametrize("cx, cy", [(5.0, 100.0), (236.0, 100.0), (120.0, 4.0), (120.0, 197.5), (3.0, 2.0)], ids=["left", "right", "top", "bottom", "corner"])
def test_box_clipped_by_each_canvas_edge(gpu, cx, cy):
    s = CC.shape("both", cx=cx, cy=cy, hw=30.0, hh=22.0, rotation=0.5, outline_width=2.0)
    x0, y0, bw, bh = M.bounds(s, W, H)
    assert x0 == 0 or y0 == 0 or x0 + bw == W or y0 + bh == H
    assert check(gpu, s, CC.blob_path(), what="clipped").any()


def test_box_off_the_canvas_is_ok_and_touches_nothing(gpu):
    s = SC.to_api(CC.shape("both", cx=400.0, cy=40.0, hw=20.0, hh=10.0))
    p = cpath(CC.blob_path())
    assert gpu.shape_bounds(s, W, H) == (0, 0, 0, 0)
    buf = np.full((H, W, 4), 0xA5, np.uint8)
    assert gpu._lib.pfx_custom_shape_rasterize(gpu._h, C.byref(s.to_c()), C.byref(p.c), W, H, buf.ctypes.data_as(C.c_void_p)) == 0 and (buf == 0xA5).all()
    assert not gpu.custom_shape_preview(s, p, W, H).any()
    layer = np.random.default_rng(5).integers(0, 256, (H, W, 4), dtype=np.uint8)
    assert np.array_equal(gpu.draw_custom_shape(layer, s, p, NORMAL), layer)


@pytest.mark.parametrize("fill", M.FILLS)
@pytest.mark.parametrize("rotation", [0.0, math.pi / 2, 0.4, -2.1])
def test_rotations(gpu, rotation, fill):
    s = CC.shape(fill, cx=118.5, cy=97.0, hw=70.0, hh=48.0, rotation=rotation, outline_width=3.0)
    assert check(gpu, s, CC.blob_path(), what=f"rotation {rotation}").any()


@pytest.mark.parametrize("fill", M.FILLS)
@pytest.mark.parametrize("rotation", [0.0, math.pi / 2])
@pytest.mark.parametrize("cx, cy", [(20.25, 30.25), (20.75, 30.25), (20.25, 30.75), (20.5, 30.0)])
def test_samples_on_vertices_intercepts_and_degenerate_segments(gpu, cx, cy, rotation, fill):
    # sx = sy = 1 and quarter offsets: py equals vertex ordinates (the `>` against `<=` asymmetry), px equals intercepts of the vertical and 45-degree edges
    s = CC.on_grid_shape(fill, cx, cy, rotation=rotation, outline_width=1.0)
    p = CC.predicate_edge_path()
    if rotation == 0.0 and (cx, cy) != (20.5, 30.0):
        lx, ly = CM.local_frame(s, M.bounds(s, 64, 64))
        ox, oy = (F(-0.25) if cx % 1 == 0.25 else F(0.25)), (F(-0.25) if cy % 1 == 0.25 else F(0.25))   # the sample that lands on the lattice
        px, py = (lx + ox) + F(8), (ly + oy) + F(8)
        assert (py == F(14)).any() and (py == F(2)).any() and (px == F(14)).any() and ((px == py) & (px > 8) & (px < 14)).any()
    assert check(gpu, s, p, 64, 64, "predicate edges").any()


@pytest.mark.parametrize("sy_log2", [-2, 3])
def test_power_of_two_scales_put_samples_on_vertex_rows(gpu, sy_log2):
    half = 8.0 / 2.0 ** sy_log2                                   # sy = 16 / (2 * half) = 2^sy_log2
    s = CC.shape("both", cx=40.25, cy=40.25, hw=8.0, hh=half, outline_width=1.0)
    assert CM.scales(CC.predicate_edge_path(), s["hw"], s["hh"]) == (F(1), F(2.0 ** sy_log2))
    assert check(gpu, s, CC.predicate_edge_path(), 96, 96, "power-of-two sy").any()


@pytest.mark.parametrize("fill, rotation, outline_width", [("both", 0.0, 3.0), ("filled", 0.4, 1.0), ("outline", 0.4, 40.0)])
def test_many_segments_far_from_the_box_and_a_few_near(gpu, fill, rotation, outline_width):
    # hw = hh = 2000 under bounds 4000: sx = sy = 1, and the 96 x 64 canvas looks at the path around (2000, 2000) where only the small square is
    s = CC.shape(fill, cx=48.0, cy=32.0, hw=2000.0, hh=2000.0, rotation=rotation, outline_width=outline_width)
    p = CC.far_and_near_path()
    got = check(gpu, s, p, 96, 64, "far and near")
    assert got.any() and not got.all()


def test_whole_path_in_view_with_a_thousand_segments(gpu):
    s = CC.shape("filled", cx=60.0, cy=40.0, hw=50.0, hh=34.0, rotation=0.2)
    got = check(gpu, s, CC.far_and_near_path(), 120, 80, "whole path")
    assert got.any()


@pytest.mark.parametrize("outline_width", [0.0, 0.5, 1.0, 3.0, 40.0])
@pytest.mark.parametrize("fill", ["outline", "both"])
def test_outline_widths(gpu, fill, outline_width):
    s = CC.shape(fill, cx=100.0, cy=90.5, hw=60.0, hh=50.0, rotation=0.4, outline_width=outline_width)
    got = check(gpu, s, CC.holed_path(), what=f"outline {outline_width}")
    assert got.any()
    if outline_width <= 1.0:   # clamped to 1: the same picture
        assert np.array_equal(got, CM.rasterize(dict(s, outline_width=F(1)), CC.holed_path(), W, H)[0])


@pytest.mark.parametrize("alpha", [255, 128, 1])
@pytest.mark.parametrize("fill", M.FILLS)
def test_primary_alpha_and_ignored_fields(gpu, fill, alpha):
    # sx = sy = 1 at half-pixel offsets: the path's corners cover one, two and three samples of a pixel (tests/test_customshape_model_host.py derives it)
    s = CC.shape(fill, cx=60.5, cy=50.5, hw=8.0, hh=8.0, outline_width=2.0, primary=(200, 100, 50, alpha))
    p = CC.holed_path()
    got = check(gpu, s, p, what=f"alpha {alpha}")
    assert len(np.unique(got[..., 3])) == (2 if alpha == 1 else 5)
    partial = (got[..., 0] == 200) & (got[..., 3] < alpha)
    assert partial.any()
    if alpha == 1:   # round(1 * 0.25) = 0: the colour stays in the box buffer with alpha 0, and the preview drops the pixel
        assert ((got[..., 3] == 0) & (got[..., 0] == 200)).any()
    other = dict(s, secondary=(1, 2, 3, 4), anti_alias=not s["anti_alias"], corner_radius=F(9))
    assert np.array_equal(gpu.rasterize_custom_shape(SC.to_api(other), cpath(p), W, H)[0], got)
    skewed = dict(s, kind="parallelogram")   # the kind shapes the box, nothing else
    want, box = CM.rasterize(skewed, p, W, H)
    got2, box2 = gpu.rasterize_custom_shape(SC.to_api(skewed), cpath(p), W, H)
    assert box2 == box and box != M.bounds(s, W, H) and np.array_equal(got2, want)


SCALE_CASES = {
    "narrow_half_width": (CC.shape("both", cx=30.0, cy=30.0, hw=0.3, hh=20.0, outline_width=1.0), CC.holed_path()),
    "narrow_both": (CC.shape("both", cx=30.0, cy=30.0, hw=0.2, hh=0.4, outline_width=2.0), CC.holed_path()),
    "bounds_below_one": (CC.shape("both", cx=40.0, cy=30.0, hw=30.0, hh=20.0, rotation=0.3, outline_width=1.0), CM.path([CC.square(0, 0, 0.5, 0.25)])),
    "sx_8_sy": (CC.shape("both", cx=60.0, cy=50.0, hw=5.0, hh=40.0, rotation=0.2, outline_width=2.0), CC.holed_path()),
    "sy_8_sx": (CC.shape("outline", cx=60.0, cy=50.0, hw=40.0, hh=5.0, rotation=0.2, outline_width=2.0), CC.holed_path()),
}


@pytest.mark.parametrize("name", sorted(SCALE_CASES))
def test_scale_edges(gpu, name):
    s, p = SCALE_CASES[name]
    sx, sy = CM.scales(p, s["hw"], s["hh"])
    if name == "sx_8_sy":
        assert sx == 8 * sy
    if name == "sy_8_sx":
        assert sy == 8 * sx
    assert check(gpu, s, p, 128, 100, name).any()


def test_culling_changes_nothing(gpu):
    s = CC.shape("both", cx=48.0, cy=32.0, hw=2000.0, hh=2000.0, rotation=0.4, outline_width=3.0)
    p = cpath(CC.far_and_near_path())
    on = gpu.rasterize_custom_shape(SC.to_api(s), p, 96, 64)[0]
    was = gpu.customshape_cull(False)
    try:
        assert gpu.customshape_info(2) == 0
        off = gpu.rasterize_custom_shape(SC.to_api(s), p, 96, 64)[0]
    finally:
        gpu.customshape_cull(was)
    assert was and gpu.customshape_info(2) == 1 and np.array_equal(on, off) and on.any()


@pytest.fixture(scope="module")
def draw_inputs():
    rng = np.random.default_rng(77)
    layer = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    layer[:, :60, 3] = 0
    layer[:, 60:100, 3] = 255
    selection = (rng.integers(0, 3, (H, W)) * 127).astype(np.uint8)
    return layer, selection


DRAW_SHAPE = CC.shape("both", cx=90.25, cy=70.5, hw=58.0, hh=37.0, rotation=0.4, outline_width=4.0, primary=(250, 70, 30, 140))


@pytest.mark.parametrize("masked", [False, True], ids=["all", "selection"])
@pytest.mark.parametrize("mode", [NORMAL, MULTIPLY, OVERWRITE, XOR])
def test_draw_equals_preview_then_commit(gpu, draw_inputs, mode, masked):
    layer, selection = draw_inputs
    sel = selection if masked else None
    s, p = SC.to_api(DRAW_SHAPE), cpath(CC.blob_path())
    x0, y0, bw, bh = gpu.shape_bounds(s, W, H)
    want = gpu.brush_commit(layer, gpu.custom_shape_preview(s, p, W, H), mode, selection=sel)
    got = gpu.draw_custom_shape(layer, s, p, mode, selection=sel)
    assert np.array_equal(got, want) and not np.array_equal(got, layer)
    outside = np.ones(layer.shape[:2], bool)
    outside[y0:y0 + bh, x0:x0 + bw] = False
    assert np.array_equal(got[outside], layer[outside])


def test_draw_on_a_layer_at_a_pointer_offset_with_guards(gpu, draw_inputs):
    layer, selection = draw_inputs
    s, p = SC.to_api(DRAW_SHAPE), cpath(CC.blob_path())
    lead, tail = 4 * 37, 4 * 29                                    # dword-aligned, not 16-byte aligned
    guarded = np.concatenate([np.full(lead, 0x5A, np.uint8), layer.ravel(), np.full(tail, 0xC3, np.uint8)])
    d, d_sel = gpu.dev_alloc(guarded.nbytes), gpu.dev_alloc(selection.nbytes)
    try:
        gpu.dev_upload(d, guarded)
        gpu.dev_upload(d_sel, selection)
        gpu.draw_custom_shape_dev(d + lead, W, H, s, p, MULTIPLY, d_sel)
        got = gpu.dev_download(d, guarded.shape)
    finally:
        gpu.dev_free(d)
        gpu.dev_free(d_sel)
    assert (got[:lead] == 0x5A).all() and (got[-tail:] == 0xC3).all()
    want = gpu.brush_commit(layer, gpu.custom_shape_preview(s, p, W, H), MULTIPLY, selection=selection)
    assert np.array_equal(got[lead:-tail].reshape(layer.shape), want)


def test_device_tiers_equal_the_host_tiers(gpu):
    s, p = SC.to_api(DRAW_SHAPE), cpath(CC.blob_path())
    buf, (x0, y0, bw, bh) = gpu.rasterize_custom_shape(s, p, W, H)
    d = gpu.dev_alloc(W * H * 4)
    try:
        gpu.dev_upload(d, np.full(W * H * 4, 0x77, np.uint8))
        gpu.rasterize_custom_shape_dev(s, p, W, H, d)
        flat = gpu.dev_download(d, (W * H * 4,))
        assert np.array_equal(flat[:bw * bh * 4].reshape(bh, bw, 4), buf) and (flat[bw * bh * 4:] == 0x77).all()
        gpu.custom_shape_preview_dev(s, p, W, H, d)
        assert np.array_equal(gpu.dev_download(d, (H, W, 4)), gpu.custom_shape_preview(s, p, W, H))
        gpu.dev_upload(d, np.full(W * H * 4, 0x77, np.uint8))
        gpu.custom_shape_icon_dev(p, 48, True, d)
        flat = gpu.dev_download(d, (W * H * 4,))
        assert np.array_equal(flat[:48 * 48 * 4].reshape(48, 48, 4), gpu.custom_shape_icon(p, 48, True)) and (flat[48 * 48 * 4:] == 0x77).all()
    finally:
        gpu.dev_free(d)


@pytest.mark.parametrize("dark", [False, True], ids=["light", "dark"])
@pytest.mark.parametrize("size", [1, 7, 48, 65])
def test_icon(gpu, size, dark):
    p = CC.blob_path()
    want = CM.icon(p, size, dark)
    got = gpu.custom_shape_icon(cpath(p), size, dark)
    assert np.array_equal(got, want) and want.any()
    if size >= 48:
        assert (want[..., 3] == 0).any() and (want[..., 3] == 255).any() and ((want[..., 3] > 0) & (want[..., 3] < 255)).any()


def test_icon_of_a_path_without_segments_is_empty(gpu):
    assert not gpu.custom_shape_icon(cpath(CC.counted_path(0)), 16, True).any()


def test_every_refusal_leaves_the_output_alone(gpu):
    from paintfe_amd import CustomPath
    lib, h = gpu._lib, gpu._h
    good_s, good_p = SC.to_api(DRAW_SHAPE), cpath(CC.holed_path())
    buf = np.full((H, W, 4), 0xA5, np.uint8)
    out = buf.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")
    many = np.zeros((65538, 2), np.float32)
    many[:, 0] = np.arange(65538) % 7
    many[:, 1] = np.arange(65538) % 5
    bad_paths = {"nan point": CustomPath([np.array([(0, 0), (nan, 1), (2, 2)], F)], (0, 0, 4, 4)),
                 "inf point": CustomPath([CC.square(0, 0, 4, 4), np.array([(0, 0), (1, -inf)], F)], (0, 0, 4, 4)),
                 "nan bound": CustomPath([CC.square(0, 0, 4, 4)], (0, 0, nan, 4)),
                 "inf bound": CustomPath([CC.square(0, 0, 4, 4)], (-inf, 0, 4, 4)),
                 "65537 segments": CustomPath([many], (0, 0, 8, 8))}
    at_the_limit = CustomPath([many[:65537]], (0, 0, 8, 8))
    n = C.c_uint32(0)
    assert lib.pfx_custom_shape_segments(C.byref(at_the_limit.c), None, 0, C.byref(n)) == 0 and n.value == 65536
    d_layer = gpu.dev_alloc(buf.nbytes)
    try:
        gpu.dev_upload(d_layer, buf)

        def refused(s_ref, p_ref, what):
            assert lib.pfx_custom_shape_rasterize(h, s_ref, p_ref, W, H, out) == -1, what
            assert lib.pfx_custom_shape_preview(h, s_ref, p_ref, W, H, out) == -1, what
            assert lib.pfx_custom_shape_rasterize_dev(h, s_ref, p_ref, W, H, C.c_void_p(d_layer)) == -1, what
            assert lib.pfx_custom_shape_preview_dev(h, s_ref, p_ref, W, H, C.c_void_p(d_layer)) == -1, what
            assert lib.pfx_custom_shape_draw_dev(h, C.c_void_p(d_layer), W, H, s_ref, p_ref, 0, None) == -1, what

        for what, p in bad_paths.items():
            refused(C.byref(good_s.to_c()), C.byref(p.c), what)
            assert lib.pfx_custom_shape_icon(h, C.byref(p.c), 16, 1, out) == -1, what
            assert lib.pfx_custom_shape_icon_dev(h, C.byref(p.c), 16, 1, C.c_void_p(d_layer)) == -1, what
            assert lib.pfx_custom_shape_segments(C.byref(p.c), None, 0, C.byref(n)) == -1, what
        for field, value in (("fill_mode", 3), ("cx", nan), ("cy", inf), ("hw", nan), ("hh", -inf), ("rotation", inf), ("outline_width", nan),
                             ("outline_width", inf)):
            c = good_s.to_c()
            setattr(c, field, value)
            refused(C.byref(c), C.byref(good_p.c), field)
        refused(None, C.byref(good_p.c), "null shape")
        refused(C.byref(good_s.to_c()), None, "null path")
        for size in (0, 1025):
            assert lib.pfx_custom_shape_icon(h, C.byref(good_p.c), size, 1, out) == -1
            assert lib.pfx_custom_shape_icon_dev(h, C.byref(good_p.c), size, 1, C.c_void_p(d_layer)) == -1
        assert lib.pfx_custom_shape_icon(h, None, 16, 1, out) == -1 and lib.pfx_custom_shape_icon(h, C.byref(good_p.c), 16, 1, None) == -1
        assert lib.pfx_custom_shape_rasterize(h, C.byref(good_s.to_c()), C.byref(good_p.c), W, H, None) == -1
        assert lib.pfx_custom_shape_draw_dev(h, None, W, H, C.byref(good_s.to_c()), C.byref(good_p.c), 0, None) == -1
        null_points = CustomPath([CC.square(0, 0, 4, 4)], (0, 0, 4, 4))
        null_points.c.points_xy = None
        refused(C.byref(good_s.to_c()), C.byref(null_points.c), "null points")
        assert (buf == 0xA5).all() and (gpu.dev_download(d_layer, buf.shape) == 0xA5).all()
        # and the context still draws
        assert gpu.rasterize_custom_shape(good_s, good_p, W, H)[0].any()
    finally:
        gpu.dev_free(d_layer)


@pytest.mark.parametrize("kind", ["rectangle", "heart", "arrow"])
def test_built_in_shapes_still_equal_their_model(gpu, kind):
    # guards k_shape_pixel.h, which k_shapes.hip now shares with k_customshape.hip
    for fill in M.FILLS:
        s = M.shape(kind, fill, cx=70.25, cy=53.5, hw=48.0, hh=31.0, rotation=0.4, outline_width=4.0, primary=(250, 70, 30, 140), secondary=(20, 160, 240, 90))
        want, box, _ = M.rasterize(s, W, H, "device")
        got, got_box = gpu.rasterize_shape(SC.to_api(s), W, H)
        assert got_box == box and np.array_equal(got, want) and want.any()
        assert np.array_equal(gpu.shape_preview(SC.to_api(s), W, H), M.to_canvas(want, box, W, H))
