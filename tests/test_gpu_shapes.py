"""The device shape rasteriser (k_shapes.hip) against the reference's goldens and the CPU model (GPU).

Exact kinds (no per-pixel libm) match the goldens and the model at tolerance 0.  The libm kinds (pentagon, hexagon, octagon, star5, star6) are in the LIBM
class against the goldens and match the model's device flavour at tolerance 0 — unless the model counted `amb` ambiguous libm calls (an f64 result
within 4 f64 ulps of an f32 rounding boundary), in which case at most `amb` pixels may differ, by at most 1."""
import ctypes as C

import numpy as np
import pytest

from . import shape_cases as SC
from . import shape_model as M
from .test_gpu_libm_model import EXACT, LIBM, check_glibc

pytestmark = pytest.mark.gpu
NORMAL, MULTIPLY, XOR, OVERWRITE = 0, 1, 13, 14   # BlendMode::to_u8


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


@pytest.fixture(scope="module")
def goldens():
    return SC.load_goldens()


def check_model(got, s, model, amb, what):
    d = np.abs(got.astype(np.int16) - model.astype(np.int16))
    px = int((d.max(-1) > 0).sum()) if d.size else 0
    worst = int(d.max()) if d.size else 0
    if s["kind"] not in M.LIBM_KINDS or amb == 0:
        assert worst == 0, f"{what} vs model: max diff {worst}, {px} px differ, no ambiguous call"
    else:
        assert worst <= 1 and px <= amb, f"{what} vs model: max diff {worst}, {px} px differ, {amb} ambiguous calls"


@pytest.mark.parametrize("name", sorted(SC.GOLDEN))
def test_goldens_through_shape_preview(gpu, goldens, name):
    s = SC.GOLDEN[name]
    got = gpu.shape_preview(SC.to_api(s), SC.GOLDEN_W, SC.GOLDEN_H)
    check_glibc(got, goldens[f"shapes/{name}"], LIBM if s["kind"] in M.LIBM_KINDS else EXACT, name)
    model, amb = M.preview(s, SC.GOLDEN_W, SC.GOLDEN_H, "device")
    check_model(got, s, model, amb, name)


@pytest.mark.parametrize("kind", M.KINDS)
def test_rasterize_matches_the_model_on_the_sweep(gpu, kind):
    n = 0
    for cid, s in SC.sweep_cases():
        if s["kind"] != kind:
            continue
        model, box, amb = M.rasterize(s, SC.SWEEP_W, SC.SWEEP_H, "device")
        got, got_box = gpu.rasterize_shape(SC.to_api(s), SC.SWEEP_W, SC.SWEEP_H)
        assert got_box == box and got.shape == model.shape, cid
        check_model(got, s, model, amb, cid)
        if s["fill"] == "both":   # the box form pasted where a > 0 is the canvas form
            assert np.array_equal(gpu.shape_preview(SC.to_api(s), SC.SWEEP_W, SC.SWEEP_H), M.to_canvas(got, box, SC.SWEEP_W, SC.SWEEP_H)), cid
        n += 1
    assert n == 36


@pytest.mark.parametrize("case", SC.width_cases(), ids=lambda c: c[0])
def test_box_widths_around_the_tile_width(gpu, case):
    cid, s, bw = case
    model, box, amb = M.rasterize(s, SC.SWEEP_W, SC.SWEEP_H, "device")
    got, got_box = gpu.rasterize_shape(SC.to_api(s), SC.SWEEP_W, SC.SWEEP_H)
    assert got_box == box and box[2] == bw
    check_model(got, s, model, amb, cid)
    assert np.array_equal(gpu.shape_preview(SC.to_api(s), SC.SWEEP_W, SC.SWEEP_H), M.to_canvas(model, box, SC.SWEEP_W, SC.SWEEP_H))


def test_empty_box_is_ok_and_touches_nothing(gpu):
    s = SC.to_api(M.shape("heart", "both", cx=400.0, cy=40.0, hw=20.0, hh=10.0))
    assert gpu.shape_bounds(s, SC.SWEEP_W, SC.SWEEP_H) == (0, 0, 0, 0)
    buf = np.full((SC.SWEEP_H, SC.SWEEP_W, 4), 0xA5, np.uint8)
    st = gpu._lib.pfx_shape_rasterize(gpu._h, C.byref(s.to_c()), C.c_uint32(SC.SWEEP_W), C.c_uint32(SC.SWEEP_H), buf.ctypes.data_as(C.c_void_p))
    assert st == 0 and (buf == 0xA5).all()
    assert not gpu.shape_preview(s, SC.SWEEP_W, SC.SWEEP_H).any()
    layer = np.random.default_rng(5).integers(0, 256, (SC.SWEEP_H, SC.SWEEP_W, 4), dtype=np.uint8)
    assert np.array_equal(gpu.draw_shape(layer, s, NORMAL), layer)


def test_bad_shapes_are_refused_and_leave_the_output_alone(gpu):
    from paintfe_amd import PfxError
    buf = np.full((SC.GOLDEN_H, SC.GOLDEN_W, 4), 0xA5, np.uint8)
    for field, value in (("kind", 17), ("fill_mode", 3), ("hw", float("nan")), ("rotation", float("inf"))):
        c = SC.to_api(SC.GOLDEN["heart_filled"]).to_c()
        setattr(c, field, value)
        for fn in (gpu._lib.pfx_shape_rasterize, gpu._lib.pfx_shape_preview):
            assert fn(gpu._h, C.byref(c), C.c_uint32(SC.GOLDEN_W), C.c_uint32(SC.GOLDEN_H), buf.ctypes.data_as(C.c_void_p)) == -1, field
    assert (buf == 0xA5).all()
    with pytest.raises(PfxError):
        gpu.shape_preview(SC.to_api(M.shape(17, 0)), 64, 64)


DRAW_SHAPES = {"heart": M.shape("heart", "both", cx=70.25, cy=33.5, hw=38.0, hh=27.0, rotation=0.4, outline_width=4.0, primary=(250, 70, 30, 140),
                                secondary=(20, 160, 240, 90)),
               "star_clipped": M.shape("star5", "both", cx=118.0, cy=8.0, hw=30.0, hh=30.0, outline_width=2.0, secondary=(20, 160, 240, 200))}


@pytest.fixture(scope="module")
def draw_inputs():
    rng = np.random.default_rng(77)
    layer = rng.integers(0, 256, (SC.SWEEP_H, SC.SWEEP_W, 4), dtype=np.uint8)
    layer[:, :20, 3] = 0
    layer[:, 20:40, 3] = 255
    selection = (rng.integers(0, 3, (SC.SWEEP_H, SC.SWEEP_W)) * 127).astype(np.uint8)
    return layer, selection


@pytest.mark.parametrize("masked", [False, True], ids=["all", "selection"])
@pytest.mark.parametrize("mode", [NORMAL, MULTIPLY, OVERWRITE, XOR])
@pytest.mark.parametrize("which", sorted(DRAW_SHAPES))
def test_draw_equals_preview_then_commit(gpu, draw_inputs, which, mode, masked):
    layer, selection = draw_inputs
    sel = selection if masked else None
    s = SC.to_api(DRAW_SHAPES[which])
    x0, y0, bw, bh = gpu.shape_bounds(s, SC.SWEEP_W, SC.SWEEP_H)
    want = gpu.brush_commit(layer, gpu.shape_preview(s, SC.SWEEP_W, SC.SWEEP_H), mode, selection=sel)
    got = gpu.draw_shape(layer, s, mode, selection=sel)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, layer)
    outside = np.ones(layer.shape[:2], bool)
    outside[y0:y0 + bh, x0:x0 + bw] = False
    assert np.array_equal(got[outside], layer[outside])
    # in place: a second draw on the result is a second commit
    assert np.array_equal(gpu.draw_shape(got, s, mode, selection=sel), gpu.brush_commit(want, gpu.shape_preview(s, SC.SWEEP_W, SC.SWEEP_H), mode, selection=sel))


def test_draw_dev_twice_on_one_device_layer(gpu, draw_inputs):
    layer, _ = draw_inputs
    s = SC.to_api(DRAW_SHAPES["heart"])
    d = gpu.dev_alloc(layer.nbytes)
    try:
        gpu.dev_upload(d, layer)
        gpu.draw_shape_dev(d, SC.SWEEP_W, SC.SWEEP_H, s, MULTIPLY)
        gpu.draw_shape_dev(d, SC.SWEEP_W, SC.SWEEP_H, s, MULTIPLY)
        got = gpu.dev_download(d, layer.shape)
    finally:
        gpu.dev_free(d)
    pv = gpu.shape_preview(s, SC.SWEEP_W, SC.SWEEP_H)
    assert np.array_equal(got, gpu.brush_commit(gpu.brush_commit(layer, pv, MULTIPLY), pv, MULTIPLY))
