"""The text layer's styles on the device (k_textfx.hip, pfx_textfx.cpp) against the CPU model (tests/textfx_model.py).  Everything is in the EXACT class — u8 disc
maxima, integer source-over, single-rounded f32 with the host's cosf / sinf, on top of the bit-exact Gaussian — so every comparison is np.array_equal.
tests/test_textfx_model_host.py asserts that each case draws what it is named after, so nothing here passes vacuously.  The argument contract of the four new
calls is pinned here (the table of tests/test_gpu_arg_contract.py keys on width / height parameters, which these calls carry in their descriptor)."""
import ctypes as C

import numpy as np
import pytest

from . import textfx_cases as TC
from . import textfx_model as M
from .dev_buffers import SENTINEL, DevBuffers, differing, sentinel_like

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -5
FLOATS = ["outline_width", "shadow_offset_x", "shadow_offset_y", "shadow_blur_radius", "shadow_spread", "inner_offset_x", "inner_offset_y", "inner_blur_radius",
          "gradient_angle_degrees", "gradient_scale", "texture_scale"]
FLOAT_PAIRS = ["gradient_offset", "texture_offset"]


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


@pytest.fixture(autouse=True)
def stop_after_a_device_error(gpu):
    """a HIP error behind a test ends the session: nothing more is launched on a device that has reported one"""
    yield
    from paintfe_amd import PfxError
    try:
        gpu.synchronize()
    except PfxError as e:
        pytest.exit(f"the device reported an error after this test: {e}", returncode=3)


def describe(size, effects):
    from paintfe_amd import text_effects
    return text_effects(size, **effects)


def run_dev(gpu, fx, text, texture, call="effects"):
    """one of the two device calls on fresh buffers with sentinels around them; the inputs must come back untouched"""
    arrays = [text, sentinel_like(text)] + ([texture] if texture is not None else [])
    bufs = DevBuffers(gpu, *arrays)
    with bufs as ptrs:
        d_tex = ptrs[2] if texture is not None else 0
        region = None
        if call == "effects":
            gpu.text_effects_dev(fx, ptrs[0], ptrs[1], texture_ptr=d_tex)
        else:
            region = gpu.text_layer_effects_dev(fx, ptrs[0], ptrs[1], texture_ptr=d_tex)
        got = gpu.dev_download(ptrs[1], text.shape)
        assert np.array_equal(gpu.dev_download(ptrs[0], text.shape), text)
        assert texture is None or np.array_equal(gpu.dev_download(d_tex, texture.shape), texture)
        assert bufs.surroundings_intact()
    return got, region


# ---- apply_text_effects ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", TC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", TC.NAMES)
def test_effects_equal_the_model(gpu, name, size):
    want, _ = TC.expected(name, size)
    got, _ = run_dev(gpu, describe(size, TC.effects_of(name)), TC.text_of(size), TC.texture_of(name))
    n = differing(got, want)
    print(f"{name} {size}: {n} differing pixels")
    assert np.array_equal(got, want), n


@pytest.mark.parametrize("width,position", TC.TILE_SHAPE_OUTLINES)
def test_the_largest_radius_and_the_two_tile_shapes(gpu, width, position):
    """PFX_TEXT_FX_MAX_RADIUS: the disc kernel's largest halo, wider than the 131 x 70 image is tall; and both sides of the halo (8) at which the disc
    kernel changes its tile from 64 x 32 to 64 x 64"""
    size = TC.MEASURED
    effects = dict(outline=dict(width=width, position=position, color=(9, 99, 199, 230)))
    want, counts = M.apply(TC.text_of(size), effects)
    assert sum(counts["outline"]) > 500
    got, _ = run_dev(gpu, describe(size, effects), TC.text_of(size), None)
    assert np.array_equal(got, want), differing(got, want)
    # the same on the image that sees each tap of this disc: the slab for the minimum, whose eroded plane is not zero, the dots for the maximum, whose
    # dilated plane is the disc itself (the rings saturate under a large maximum and vanish under a large minimum; the slab saturates under any maximum:
    # tests/test_textfx_disc_host.py)
    image = TC.tile_shape_image(position)
    shape = (image.shape[1], image.shape[0])
    want, counts = M.apply(image, effects)
    assert sum(counts["outline"]) > 500
    got, _ = run_dev(gpu, describe(shape, effects), image, None)
    assert np.array_equal(got, want), (shape, differing(got, want))


@pytest.mark.parametrize("name,size", TC.DISC_RUNS, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_disc_cases_equal_the_model(gpu, name, size):
    """inside outlines on the slab, outside outlines and spread shadows on the dots: inputs on which a tap missing from the disc changes the picture"""
    want, _ = TC.expected_disc_case(name, size)
    got, _ = run_dev(gpu, describe(size, TC.DISC_CASES[name][1]), TC.disc_text(name, size), None)
    assert np.array_equal(got, want), differing(got, want)


@pytest.mark.parametrize("name", ["defaults", "everything"])
def test_host_tier(gpu, name):
    size = TC.MEASURED
    want, _ = TC.expected(name, size)
    got = gpu.text_effects(describe(size, TC.effects_of(name)), TC.text_of(size), TC.texture_of(name))
    assert np.array_equal(got, want), differing(got, want)


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.DOCUMENTS)
def test_layer_equals_the_model(gpu, name):
    text, effects = TC.document(name)
    want, want_region = TC.expected_layer(name)
    got, r = run_dev(gpu, describe(TC.CANVAS, effects), text, None, call="layer")
    assert dict(x=r.x, y=r.y, w=r.w, h=r.h, pad_px=r.pad_px, full_canvas=r.full_canvas) == want_region
    assert np.array_equal(got, want), differing(got, want)


@pytest.mark.parametrize("name", list(TC.BOUNDS_DOCUMENTS))
def test_tight_bounds_at_the_canvas_edges(gpu, name):
    """the bounds kernel's extremes: each corner, the column behind a workgroup's first 256, the rows behind its first 2048 workgroups"""
    text = TC.bounds_document(name)
    canvas = TC.BOUNDS_DOCUMENTS[name][0]
    want, want_region = TC.expected_bounds_layer(name)
    assert want_region["w"] > 0 and want.any()
    got, r = run_dev(gpu, describe(canvas, TC.BOUNDS_EFFECTS), text, None, call="layer")
    assert dict(x=r.x, y=r.y, w=r.w, h=r.h, pad_px=r.pad_px, full_canvas=r.full_canvas) == want_region
    assert np.array_equal(got, want), differing(got, want)


def test_layer_region_with_a_texture(gpu):
    """the region path hands the texture through, sampled from the region's origin"""
    text, _ = TC.document("corner")
    effects = dict(shadow={}, texture_fill=dict(texture_width=7, texture_height=3, scale=2.5, offset=(-10.5, -7.0)))
    want, want_region = M.layer(text, effects, TC.TEXTURE)
    got, r = run_dev(gpu, describe(TC.CANVAS, effects), text, TC.TEXTURE, call="layer")
    assert (r.x, r.y, r.w, r.h, r.full_canvas) == (want_region["x"], want_region["y"], want_region["w"], want_region["h"], 0)
    assert np.array_equal(got, want), differing(got, want)


# ---- the argument contract ---------------------------------------------------------------------------------------------------------------------------------------------------
SIZE = (40, 12)
EVERYTHING = dict(outline={}, shadow={}, inner_shadow={}, gradient_fill={}, texture_fill=dict(texture_width=7, texture_height=3))


class Call:
    """the three calls that take a context, on raw pointers: status only"""
    def __init__(self, gpu, which):
        from paintfe_amd import _lib
        self.lib, self.ctx, self.which, self.region = _lib.load(), gpu.handle, which, _lib.TextRegion(7, 7, 7, 7, 7, 7)

    def __call__(self, fx, text, texture, out):
        p = [C.c_void_p(v or None) for v in (text, texture, out)]
        fxp = C.byref(fx) if fx is not None else None
        if self.which == "effects_dev":
            return self.lib.pfx_text_effects_dev(self.ctx, fxp, *p)
        if self.which == "effects":
            return self.lib.pfx_text_effects(self.ctx, fxp, *p)
        return self.lib.pfx_text_layer_effects_dev(self.ctx, fxp, *p, C.byref(self.region))

    def region_untouched(self):
        return bytes(self.region) == np.full(6, 7, np.uint32).tobytes()


def refusals(fx_of, text, texture, out):
    """(what, descriptor, text, texture, out, status) for pointers text / texture / out that are fine as they are"""
    yield "null descriptor", None, text, texture, out, ERR_INVALID
    yield "null text", fx_of(), 0, texture, out, ERR_INVALID
    yield "null out", fx_of(), text, texture, 0, ERR_INVALID
    yield "texture flag, a texture size, no texture", fx_of(), text, 0, out, ERR_INVALID
    for field in FLOATS:
        for bad in (float("nan"), float("inf"), float("-inf")):
            fx = fx_of()
            setattr(fx, field, bad)
            yield f"{field} = {bad}", fx, text, texture, out, ERR_INVALID
    for field in FLOAT_PAIRS:
        for k in (0, 1):
            fx = fx_of()
            getattr(fx, field)[k] = float("nan")
            yield f"{field}[{k}] = nan", fx, text, texture, out, ERR_INVALID
    fx = fx_of(); fx.flags = 0; fx.shadow_spread = float("nan")
    yield "a float that is not finite behind a cleared flag", fx, text, texture, out, ERR_INVALID
    for pos in (3, -1, 1 << 20):
        fx = fx_of(); fx.outline_position = pos
        yield f"outline position {pos}", fx, text, texture, out, ERR_INVALID
    for w, h in ((0, 12), (40, 0), (20000, 20000), (0xFFFFFFFF, 0xFFFFFFFF)):
        fx = fx_of(); fx.width, fx.height = w, h
        yield f"size {w} x {h}", fx, text, texture, out, ERR_INVALID
    fx = fx_of(); fx.tex_w, fx.tex_h = 20000, 20000
    yield "a texture outside the document limit", fx, text, texture, out, ERR_INVALID
    yield "out is text", fx_of(), text, texture, text, ERR_INVALID
    yield "out starts inside text", fx_of(), text, texture, text + 4 * SIZE[0], ERR_INVALID
    yield "out ends inside text", fx_of(), text + 4 * SIZE[0], texture, text, ERR_INVALID
    yield "out overlaps the texture", fx_of(), text, out + 8, out, ERR_INVALID
    for what, fx in (("outline 64.5", dict(outline=dict(width=64.5))), ("centre outline 129.5", dict(outline=dict(width=129.5, position="center"))),
                     ("inside outline 1000", dict(outline=dict(width=1000.0, position="inside"))), ("spread 64.01", dict(shadow=dict(spread=64.01))),
                     ("shadow blur beyond the Gaussian", dict(shadow=dict(blur_radius=1.0e6))), ("inner blur beyond the Gaussian", dict(inner_shadow=dict(blur_radius=284.0)))):
        yield what, describe(SIZE, fx), text, texture, out, ERR_UNSUPPORTED


@pytest.mark.parametrize("which", ["effects_dev", "layer_dev"])
def test_device_calls_refuse_before_they_touch_anything(gpu, which):
    text = TC.text_image(SIZE[0], 3 * SIZE[1], seed=3)     # three images' worth, so that shifted pointers stay inside the allocation
    prior_out = sentinel_like(text)
    bufs = DevBuffers(gpu, text, prior_out, TC.TEXTURE)
    call = Call(gpu, which)
    with bufs as (d_text, d_out, d_tex):
        assert call(describe(SIZE, EVERYTHING), d_text, d_tex, d_out) == OK        # the same arguments, nothing wrong: accepted
        gpu.dev_upload(d_out, prior_out)
        call.region = type(call.region)(7, 7, 7, 7, 7, 7)
        cases = list(refusals(lambda: describe(SIZE, EVERYTHING), d_text, d_tex, d_out))
        for ptr in ("text", "texture", "out"):
            for off in (1, 2, 3):
                p = dict(text=d_text, texture=d_tex, out=d_out)
                p[ptr] += off
                cases.append((f"{ptr} {off} bytes off a dword", describe(SIZE, EVERYTHING), p["text"], p["texture"], p["out"], ERR_INVALID))
        for what, fx, t, x, o, status in cases:
            assert call(fx, t, x, o) == status, what
        gpu.synchronize()
        assert np.array_equal(gpu.dev_download(d_out, prior_out.shape), prior_out)
        assert np.array_equal(gpu.dev_download(d_text, text.shape), text) and np.array_equal(gpu.dev_download(d_tex, TC.TEXTURE.shape), TC.TEXTURE)
        assert bufs.surroundings_intact() and call.region_untouched()
        # an unused texture pointer is not looked at: NULL with tex_w = 0, and without the flag
        fx = describe(SIZE, EVERYTHING); fx.tex_w = 0
        assert call(fx, d_text, 0, d_out) == OK
        assert call(describe(SIZE, dict(outline={})), d_text, 0, d_out) == OK


def test_host_call_refuses_before_it_touches_anything(gpu):
    text = TC.text_image(SIZE[0], 3 * SIZE[1], seed=3)
    out = sentinel_like(text)
    tex = TC.TEXTURE.copy()
    call = Call(gpu, "effects")
    for what, fx, t, x, o, status in refusals(lambda: describe(SIZE, EVERYTHING), text.ctypes.data, tex.ctypes.data, out.ctypes.data):
        assert call(fx, t, x, o) == status, what
    assert (out == SENTINEL).all()
    assert call(describe(SIZE, EVERYTHING), text.ctypes.data + 1, tex.ctypes.data, out.ctypes.data) == OK   # host buffers need no alignment
    want, _ = M.apply(np.frombuffer(text.tobytes()[1:1 + SIZE[0] * SIZE[1] * 4], np.uint8).reshape(SIZE[1], SIZE[0], 4), EVERYTHING, tex)
    assert np.array_equal(out[:SIZE[1]], want) and (out[SIZE[1]:] == SENTINEL).all()
