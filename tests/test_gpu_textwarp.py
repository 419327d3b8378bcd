"""The text block's warps, rotation and placement on the device (k_textwarp.hip, pfx_textwarp.cpp) against the CPU model (tests/textwarp_model.py).
Path, envelope, rotate and blit are in the EXACT class: np.array_equal.  Arc and circular call atan2 per pixel: against the device-flavour model at
tolerance 0 unless the model counted ambiguous calls (then at most that many pixels off by one), against the glibc flavour within the LIBM class.
tests/test_textwarp_model_host.py holds the model and asserts that each case draws what it is named after, so nothing here passes vacuously.
Every buffer sits between sentinels and the inputs must come back untouched."""
import ctypes as C

import numpy as np
import pytest

from . import textfx_cases as FX
from . import textfx_model as FXM
from . import textwarp_cases as TC
from . import textwarp_model as M
from .libm_checks import LIBM, check_glibc
from .dev_buffers import SENTINEL, DevBuffers, differing, sentinel_like

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -5


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


def hold_to_the_libm_models(got, device, ambiguous, glibc, what):
    """the device image against the device-flavour model (tolerance 0 but for its ambiguous calls) and against the glibc flavour (the LIBM class)"""
    assert got.shape == device.shape, what
    d = np.abs(got.astype(np.int16) - device.astype(np.int16))
    px = int((d.max(-1) > 0).sum()) if d.size else 0
    print(f"{what}: {px} px differ from the device model, {ambiguous} ambiguous calls, {differing(got, glibc)} px differ from glibc")
    if ambiguous == 0:
        assert px == 0, f"{what} vs device model: max diff {int(d.max())}, {px} px differ, no ambiguous call"
    else:
        assert d.max() <= 1 and px <= ambiguous, f"{what} vs device model: max diff {int(d.max())}, {px} px differ, {ambiguous} ambiguous calls"
    check_glibc(got, glibc, LIBM, what)


def describe(size, warp):
    from paintfe_amd import text_warp
    return text_warp(size, **warp)


def run_warp(gpu, name):
    """pfx_text_warp_dev of a case between sentinels: the image and the library's plan"""
    from paintfe_amd import text_warp_plan
    size, warp, _ = TC.WARPS[name]
    desc, src = describe(size, warp), TC.source(size)
    g = text_warp_plan(desc)
    bufs = DevBuffers(gpu, src, np.full((g.out_h, g.out_w, 4), SENTINEL, np.uint8))
    with bufs as (d_src, d_out):
        gpu.text_warp_dev(desc, d_src, d_out)
        got = gpu.dev_download(d_out, (g.out_h, g.out_w, 4))
        assert np.array_equal(gpu.dev_download(d_src, src.shape), src)
        assert bufs.surroundings_intact()
    return got, g


def plan_matches(g, plan):
    return (g.out_w, g.out_h, g.off_x, g.off_y, bool(g.identity)) == (plan["out_w"], plan["out_h"], plan["off_x"], plan["off_y"], plan["identity"])


# ---- the warps -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.EXACT_WARPS)
def test_exact_warps_equal_the_model(gpu, name):
    want, plan, _, _ = TC.expected_warp(name)
    got, g = run_warp(gpu, name)
    assert plan_matches(g, plan)
    n = differing(got, want)
    print(f"{name}: {n} differing pixels")
    assert np.array_equal(got, want), n


@pytest.mark.parametrize("name", TC.LIBM_WARPS)
def test_libm_warps_hold_to_both_flavours(gpu, name):
    device, plan, _, ambiguous = TC.expected_warp(name, "device")
    glibc = TC.expected_warp(name, "glibc")[0]
    got, g = run_warp(gpu, name)
    assert plan_matches(g, plan)
    hold_to_the_libm_models(got, device, ambiguous, glibc, name)


# ---- the rotation ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.ROTATIONS))
def test_rotations_equal_the_model(gpu, name):
    from paintfe_amd import text_rotate_plan
    size, angle, pivot = TC.ROTATIONS[name]
    want, plan = TC.expected_rotation(name)
    src = TC.source(size)
    g = text_rotate_plan(size[0], size[1], angle, pivot)
    assert plan_matches(g, plan)
    bufs = DevBuffers(gpu, src, np.full((g.out_h, g.out_w, 4), SENTINEL, np.uint8))
    with bufs as (d_src, d_out):
        gpu.text_rotate_dev(size[0], size[1], angle, d_src, d_out, pivot=pivot)
        got = gpu.dev_download(d_out, want.shape)
        assert np.array_equal(gpu.dev_download(d_src, src.shape), src) and bufs.surroundings_intact()
    assert np.array_equal(got, want), differing(got, want)


# ---- the placement ------------------------------------------------------------------------------------------------------------------------------------------------------------
def place_on_device(gpu, name):
    from paintfe_amd import text_block
    blocks = TC.PLACEMENTS[name][1]
    sources = [TC.source(size) for size, *_ in blocks]
    bufs = DevBuffers(gpu, TC.start_canvas(name), *sources)
    with bufs as (d_canvas, *d_sources):
        for (size, warp, offset, rotation, pivot), d_src in zip(blocks, d_sources):
            gpu.text_block_place_dev(text_block(describe(size, warp), offset, TC.CANVAS, rotation, pivot), d_src, d_canvas)
        got = gpu.dev_download(d_canvas, (TC.CANVAS[1], TC.CANVAS[0], 4))
        for src, d_src in zip(sources, d_sources):
            assert np.array_equal(gpu.dev_download(d_src, src.shape), src)
        assert bufs.surroundings_intact()
    return got


@pytest.mark.parametrize("name", list(TC.PLACEMENTS))
def test_placements_equal_the_model(gpu, name):
    got = place_on_device(gpu, name)
    device, ambiguous = TC.expected_placement(name, "device")
    glibc, _ = TC.expected_placement(name, "glibc")
    if any(warp["kind"] in ("arc", "circular") for _, warp, *_ in TC.PLACEMENTS[name][1]):
        hold_to_the_libm_models(got, device, ambiguous, glibc, name)
    else:
        assert np.array_equal(got, glibc), differing(got, glibc)


def test_a_placed_block_through_the_styles_equals_the_two_models_composed(gpu):
    """the device pipeline from the block raster on: warp, rotate, blit into a zero canvas, then the layer's default styles"""
    from paintfe_amd import text_block, text_effects
    (size, warp, offset, rotation, pivot), = TC.PLACEMENTS["warped_and_rotated"][1]
    effects = FX.effects_of("defaults")
    layer_text, _ = TC.expected_placement("warped_and_rotated")
    want, want_region = FXM.layer(layer_text, effects)
    assert want_region["w"] > 0 and want.any()
    src = TC.source(size)
    zero = np.zeros((TC.CANVAS[1], TC.CANVAS[0], 4), np.uint8)
    bufs = DevBuffers(gpu, src, zero, sentinel_like(zero))
    with bufs as (d_src, d_canvas, d_out):
        gpu.text_block_place_dev(text_block(describe(size, warp), offset, TC.CANVAS, rotation, pivot), d_src, d_canvas)
        r = gpu.text_layer_effects_dev(text_effects(TC.CANVAS, **effects), d_canvas, d_out)
        got = gpu.dev_download(d_out, zero.shape)
        assert np.array_equal(gpu.dev_download(d_canvas, zero.shape), layer_text) and bufs.surroundings_intact()
    assert (r.x, r.y, r.w, r.h) == (want_region["x"], want_region["y"], want_region["w"], want_region["h"])
    assert np.array_equal(got, want), differing(got, want)


# ---- the host tier ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arc_distorted", "circle_ccw", "path_default", "envelope_default", "none"])
def test_host_tier(gpu, name):
    size, warp, _ = TC.WARPS[name]
    got, g = gpu.text_warp(describe(size, warp), TC.source(size))
    device, plan, _, ambiguous = TC.expected_warp(name, "device")
    assert plan_matches(g, plan)
    hold_to_the_libm_models(got, device, ambiguous, TC.expected_warp(name, "glibc")[0], name)


# ---- the argument contract ----------------------------------------------------------------------------------------------------------------------------------------------------
SIZE = (40, 12)
FLOATS = ["arc_bend", "arc_hdist", "arc_vdist", "circ_radius", "circ_start_angle"]
POINTS = ["path", "top", "bottom"]


def warp_refusals(make, src, out):
    """(what, descriptor, src, out, status) for pointers that are fine as they are; out holds at least four source images"""
    yield "null descriptor", None, src, out, ERR_INVALID
    yield "null src", make(), 0, out, ERR_INVALID
    yield "null out", make(), src, 0, ERR_INVALID
    for kind in (-1, 5, 1 << 20):
        w = make(); w.kind = kind
        yield f"kind {kind}", w, src, out, ERR_INVALID
    for sw, sh in ((0, 12), (40, 0)):
        w = make(); w.src_w, w.src_h = sw, sh
        yield f"source {sw} x {sh}", w, src, out, ERR_INVALID
    for field in FLOATS:
        for bad in (float("nan"), float("inf"), float("-inf")):
            w = make(); w.kind = 0
            setattr(w, field, bad)
            yield f"{field} = {bad} behind kind none", w, src, out, ERR_INVALID
    for field in POINTS:
        for i in (0, 3):
            for k in (0, 1):
                w = make()
                getattr(w, field)[i][k] = float("nan")
                yield f"{field}[{i}][{k}] = nan", w, src, out, ERR_INVALID
    yield "out is src", make(), src, src, ERR_INVALID
    yield "out starts inside src", make(), src, src + 4 * SIZE[0], ERR_INVALID
    yield "out ends inside src", make(), out + 4 * SIZE[0], out, ERR_INVALID
    for sign in (1.0, -1.0):
        w = make(); w.circ_start_angle = sign * TC.BEYOND_EIGHT_PI
        yield f"start angle {sign} * (8 pi + an ulp)", w, src, out, ERR_UNSUPPORTED
    w = make(); w.src_w, w.src_h = 20000, 20000
    yield "a source over the document limit", w, src, out, ERR_UNSUPPORTED
    w = make(); w.kind, w.circ_radius = 2, 9000.0
    yield "a circle whose square is over the document limit", w, src, out, ERR_UNSUPPORTED


def test_device_calls_refuse_before_they_touch_anything(gpu):
    from paintfe_amd import _lib, text_block, text_warp_plan
    lib, ctx = _lib.load(), gpu.handle
    make = lambda: describe(SIZE, dict(kind="arc", bend=0.5))   # noqa: E731
    g = text_warp_plan(make())
    src = TC.source((SIZE[0], 3 * SIZE[1]))                     # three sources' worth, so that shifted pointers stay inside the allocation
    prior = np.full((4 * g.out_h, g.out_w, 4), SENTINEL, np.uint8)
    canvas = TC.prior_canvas()
    bufs = DevBuffers(gpu, src, prior, canvas)
    ptr = lambda v: C.c_void_p(v or None)   # noqa: E731
    with bufs as (d_src, d_out, d_canvas):
        def warp_dev(w, s, o):
            return lib.pfx_text_warp_dev(ctx, C.byref(w) if w is not None else None, ptr(s), ptr(o))

        def rotate_dev(w, h, angle, pivot, s, o):
            return lib.pfx_text_rotate_dev(ctx, C.c_uint32(w), C.c_uint32(h), C.c_float(angle), pivot, ptr(s), ptr(o))

        def place_dev(b, s, c):
            return lib.pfx_text_block_place_dev(ctx, C.byref(b) if b is not None else None, ptr(s), ptr(c))
        assert warp_dev(make(), d_src, d_out) == OK      # the same arguments, nothing wrong: accepted
        gpu.dev_upload(d_out, prior)
        cases = list(warp_refusals(make, d_src, d_out))
        for off in (1, 2, 3):
            cases.append((f"src {off} bytes off a dword", make(), d_src + off, d_out, ERR_INVALID))
            cases.append((f"out {off} bytes off a dword", make(), d_src, d_out + off, ERR_INVALID))
        for what, w, s, o, status in cases:
            assert warp_dev(w, s, o) == status, what
        # the rotation
        nan2, piv = (C.c_float * 2)(float("nan"), 0.0), (C.c_float * 2)(3.0, 4.0)
        for what, args, status in (("zero width", (0, 12, 0.3, None, d_src, d_out), ERR_INVALID), ("zero height", (40, 0, 0.3, None, d_src, d_out), ERR_INVALID),
                                   ("nan angle", (40, 12, float("nan"), None, d_src, d_out), ERR_INVALID), ("inf angle", (40, 12, float("inf"), None, d_src, d_out), ERR_INVALID),
                                   ("nan pivot", (40, 12, 0.3, nan2, d_src, d_out), ERR_INVALID), ("null src", (40, 12, 0.3, piv, 0, d_out), ERR_INVALID),
                                   ("null out", (40, 12, 0.3, piv, d_src, 0), ERR_INVALID), ("out is src", (40, 12, 0.3, piv, d_src, d_src), ERR_INVALID),
                                   ("misaligned src", (40, 12, 0.3, piv, d_src + 2, d_out), ERR_INVALID), ("misaligned out", (40, 12, 0.3, piv, d_src, d_out + 1), ERR_INVALID),
                                   ("over the limit", (20000, 20000, 0.3, None, d_src, d_out), ERR_UNSUPPORTED)):
            assert rotate_dev(*args) == status, what
        # the placement
        block = lambda **kw: text_block(make(), (5, 5), TC.CANVAS, **kw)   # noqa: E731
        assert place_dev(None, d_src, d_canvas) == ERR_INVALID and place_dev(block(), 0, d_canvas) == ERR_INVALID and place_dev(block(), d_src, 0) == ERR_INVALID
        for field, bad, status in (("canvas_w", 0, ERR_INVALID), ("canvas_h", 0, ERR_INVALID), ("rotation", float("nan"), ERR_INVALID), ("rotation", float("inf"), ERR_INVALID)):
            b = block(); setattr(b, field, bad)
            assert place_dev(b, d_src, d_canvas) == status, field
        b = block(); b.pivot[1] = float("nan")
        assert place_dev(b, d_src, d_canvas) == ERR_INVALID
        b = block(); b.warp.kind = 9
        assert place_dev(b, d_src, d_canvas) == ERR_INVALID
        b = block(); b.warp.arc_vdist = float("inf")
        assert place_dev(b, d_src, d_canvas) == ERR_INVALID
        b = block(); b.warp.circ_start_angle = TC.BEYOND_EIGHT_PI
        assert place_dev(b, d_src, d_canvas) == ERR_UNSUPPORTED
        b = block(); b.canvas_w, b.canvas_h = 20000, 20000
        assert place_dev(b, d_src, d_canvas) == ERR_UNSUPPORTED
        assert place_dev(block(), d_src + 1, d_canvas) == ERR_INVALID and place_dev(block(), d_src, d_canvas + 2) == ERR_INVALID
        assert place_dev(block(), d_canvas + 400, d_canvas) == ERR_INVALID      # the raster inside the canvas
        gpu.synchronize()
        assert np.array_equal(gpu.dev_download(d_out, prior.shape), prior) and np.array_equal(gpu.dev_download(d_src, src.shape), src)
        assert np.array_equal(gpu.dev_download(d_canvas, canvas.shape), canvas) and bufs.surroundings_intact()


def test_host_call_refuses_before_it_touches_anything(gpu):
    from paintfe_amd import _lib, text_warp_plan
    lib, ctx = _lib.load(), gpu.handle
    make = lambda: describe(SIZE, dict(kind="arc", bend=0.5))   # noqa: E731
    g = text_warp_plan(make())
    need = g.out_w * g.out_h * 4
    src = TC.source((SIZE[0], 3 * SIZE[1])).copy()
    out = np.full((4 * g.out_h, g.out_w, 4), SENTINEL, np.uint8)
    plan = _lib.TextWarpGeom(7, 7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
    untouched = bytes(plan)

    def call(w, s, o, out_bytes=out.nbytes):
        return lib.pfx_text_warp(ctx, C.byref(w) if w is not None else None, C.c_void_p(s or None), C.c_void_p(o or None), C.c_size_t(out_bytes), C.byref(plan))
    for what, w, s, o, status in warp_refusals(make, src.ctypes.data, out.ctypes.data):
        assert call(w, s, o) == status, what
    assert call(make(), src.ctypes.data, out.ctypes.data, need - 1) == ERR_INVALID and call(make(), src.ctypes.data, out.ctypes.data, 0) == ERR_INVALID
    assert (out == SENTINEL).all() and bytes(plan) == untouched
    assert call(make(), src.ctypes.data + 1, out.ctypes.data, need) == OK   # host buffers need no alignment; out_bytes may be exact
    shifted = np.frombuffer(src.tobytes()[1:1 + SIZE[0] * SIZE[1] * 4], np.uint8).reshape(SIZE[1], SIZE[0], 4)
    want, _, painted = M.apply_warp(shifted, dict(kind="arc", bend=0.5))[:3]
    got = out.reshape(-1)[:need].reshape(g.out_h, g.out_w, 4)
    assert painted > 100 and (plan.out_w, plan.out_h) == (g.out_w, g.out_h) and (out.reshape(-1)[need:] == SENTINEL).all()
    check_glibc(got, want, LIBM, "host tier on an unaligned source")
