"""The gradient tool and the perspective crop without a device.  There is no golden and no reference test for these tools, so the model
(tests/gradient_model.py) is held here to a scalar pixel-loop transcription written independently of its array code, to answers derived by hand, and the
library's host functions are held to the model through ctypes.  The last part asserts that tests/gradient_cases.py reaches every branch, so that no comparison
of tests/test_gpu_gradient.py passes vacuously."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from . import gradient_cases as GC
from . import gradient_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OK, ERR_INVALID = 0, -1


# ---- the scalar transcription -----------------------------------------------------------------------------------------------------------------------------------------
def rnd(v):
    """f32::round of one value as an int, half away from zero"""
    v = float(v)
    if math.isnan(v):
        return 0
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def as_u8(v):
    return min(max(v, 0), 255)


def rem_euclid_scalar(x, m):
    if math.isinf(float(x)) or math.isnan(float(x)):
        return F(np.nan)
    r = F(math.fmod(float(x), m))          # exact: both are f32 values, the result is representable
    return F(r + F(m)) if r < 0 else r


def clamp01(x):
    if x < 0:
        return F(0.0)
    if x > 1:
        return F(1.0)
    return x


def scalar_render(g, lut, w, h, sel):
    """the loops of :386-523, pixel by pixel in f32 scalars"""
    scale = g["preview_scale"]
    rw, rh = (w + scale - 1) // scale, (h + scale - 1) // scale
    table = lut
    if g["mode"] == M.TRANSPARENCY:
        table = np.zeros((256, 4), np.uint8)
        for i in range(256):
            lum = int(F(F(F(0.299) * F(lut[i][0])) + F(F(0.587) * F(lut[i][1]))) + F(F(0.114) * F(lut[i][2])))
            table[i] = (255, 255, 255, as_u8(lum) * int(lut[i][3]) // 255)
    ax, ay, bx, by = (F(v) for v in (*g["start"], *g["end"]))
    dx, dy = F(bx - ax), F(by - ay)
    len_sq = F(F(dx * dx) + F(dy * dy))
    length = F(np.sqrt(len_sq))
    inv_len = F(F(1.0) / length) if length > F(1e-6) else F(0.0)
    inv_len_sq = F(F(1.0) / len_sq) if len_sq > F(1e-6) else F(0.0)
    ux, uy = F(dx * inv_len), F(dy * inv_len)
    sf = F(scale)
    out = np.zeros((rh, rw, 4), np.uint8)
    for y in range(rh):
        py = F(F(F(y) * sf) + F(sf * F(0.5)))
        ry = F(py - ay)
        dot_y, dist_y_sq, proj_y, perp_y = F(ry * dy), F(ry * ry), F(ry * uy), F(ry * ux)
        gy = y * scale
        for x in range(rw):
            px = F(F(F(x) * sf) + F(sf * F(0.5)))
            gx = x * scale
            if sel is not None and sel[gy, gx] == 0:
                continue
            rx = F(px - ax)
            if g["shape"] == M.LINEAR:
                raw = F(F(F(rx * dx) + dot_y) * inv_len_sq)
                t = rem_euclid_scalar(raw, 1.0) if g["repeat"] else clamp01(raw)
            elif g["shape"] == M.REFLECTED:
                raw = F(F(F(rx * dx) + dot_y) * inv_len_sq)
                if g["repeat"]:
                    t_mod = rem_euclid_scalar(raw, 2.0)
                    t = F(F(2.0) - t_mod) if t_mod > 1 else t_mod
                else:
                    t = F(F(1.0) - abs(F(F(F(2.0) * clamp01(raw)) - F(1.0))))
            elif g["shape"] == M.RADIAL:
                dist = F(F(np.sqrt(F(F(rx * rx) + dist_y_sq))) * inv_len)
                t = rem_euclid_scalar(dist, 1.0) if g["repeat"] else clamp01(dist)
            else:
                proj = F(abs(F(F(rx * ux) + proj_y)) * inv_len)
                perp = F(abs(F(F(rx * F(-uy)) + perp_y)) * inv_len)
                dist = F(proj + perp)
                t = rem_euclid_scalar(dist, 1.0) if g["repeat"] else clamp01(dist)
            scaled = F(t * F(255.0))
            idx = 0 if math.isnan(float(scaled)) else int(scaled)
            a = int(table[idx][3])
            if sel is not None and sel[gy, gx] < 255:
                a = a * int(sel[gy, gx]) // 255
            if a > 0:
                out[y, x] = (table[idx][0], table[idx][1], table[idx][2], a)
    return out


def scalar_commit(layer, preview, is_eraser):
    out = layer.copy()
    h, w = layer.shape[:2]
    for y in range(h):
        for x in range(w):
            src, dst = preview[y, x], layer[y, x]
            if src[3] == 0:
                continue
            if is_eraser:
                strength, cur = F(F(src[3]) / F(255.0)), F(F(dst[3]) / F(255.0))
                new_a = max(F(cur * F(F(1.0) - strength)), F(0.0))
                out[y, x, 3] = as_u8(rnd(F(new_a * F(255.0))))
                continue
            sa, da = F(F(src[3]) / F(255.0)), F(F(dst[3]) / F(255.0))
            rest = F(F(1.0) - sa)
            out_a = F(sa + F(da * rest))
            if out_a > 0:
                rgb = [as_u8(rnd(F(F(F(F(src[k]) * sa) + F(F(F(dst[k]) * da) * rest)) / out_a))) for k in range(3)]
                out[y, x] = (*rgb, as_u8(rnd(F(out_a * F(255.0)))))
    return out


def scalar_crop(corners, layer):
    h, w = layer.shape[:2]
    plan = M.crop_plan(corners, w, h)
    out_w, out_h = plan
    c = [(F(p[0]), F(p[1])) for p in corners]
    out = np.zeros((out_h, out_w, 4), np.uint8)

    def lerp(a, b, t):
        return as_u8(rnd(F(F(F(a) * F(F(1.0) - t)) + F(F(b) * t))))
    for oy in range(out_h):
        v = F(F(F(oy) + F(0.5)) / F(out_h))
        for ox in range(out_w):
            u = F(F(F(ox) + F(0.5)) / F(out_w))
            iu, iv = F(F(1.0) - u), F(F(1.0) - v)
            s = []
            for k in (0, 1):
                s.append(F(F(F(F(F(iu * iv) * c[0][k]) + F(F(u * iv) * c[1][k])) + F(F(u * v) * c[2][k])) + F(F(iu * v) * c[3][k])))
            fx0, fy0 = math.floor(float(s[0])), math.floor(float(s[1]))
            x0, y0 = min(max(int(fx0), 0), w - 1), min(max(int(fy0), 0), h - 1)
            x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
            fx, fy = F(s[0] - F(fx0)), F(s[1] - F(fy0))
            for k in range(4):
                top = lerp(layer[y0, x0, k], layer[y0, x1, k], fx)
                bottom = lerp(layer[y1, x0, k], layer[y1, x1, k], fx)
                out[oy, ox, k] = lerp(top, bottom, fy)
    return out


SMALL = [n for n in GC.NAMES if not n.startswith("130x70-") or n == "130x70-scale3"]


@pytest.mark.parametrize("name", SMALL)
def test_render_equals_the_scalar_transcription(name):
    c = GC.CASES[name]
    want = scalar_render(c["g"], GC.lut(), c["w"], c["h"], GC.selection_of(name))
    assert np.array_equal(GC.rendered(name)[0], want)


@pytest.mark.parametrize("name,is_eraser", [c for c in GC.COMMITS if not c[0].startswith("130x70")])
def test_commit_equals_the_scalar_transcription(name, is_eraser):
    c = GC.CASES[name]
    want = scalar_commit(GC.layer(c["w"], c["h"]), GC.rendered(name)[0], is_eraser)
    assert np.array_equal(GC.committed(name, is_eraser), want)


@pytest.mark.parametrize("quad", GC.CROP_NAMES)
def test_crop_equals_the_scalar_transcription(quad):
    w, h = 67, 5
    assert np.array_equal(GC.cropped(w, h, quad)[0], scalar_crop(GC.quads(w, h)[quad], GC.layer(w, h)))


# ---- answers derived by hand -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_horizontal_linear_gradient_over_256_columns():
    """start (0, y), end (256, y) on a 256-wide canvas: px = x + 0.5, raw = (x + 0.5) * 256 / 65536 and t * 255 = (2x + 1) * 255 / 512, every step exact"""
    table = np.zeros((256, 4), np.uint8)
    table[:, 0] = np.arange(256)
    table[:, 3] = 255
    out = M.render(M.gradient((0.0, 1.0), (256.0, 1.0)), table, 256, 3)
    want = np.array([(2 * x + 1) * 255 // 512 for x in range(256)], np.uint8)
    assert np.array_equal(out[..., 0], np.broadcast_to(want, (3, 256))) and (out[..., 3] == 255).all() and not out[..., 1:3].any()


@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("repeat", [False, True])
def test_a_degenerate_drag_paints_the_first_entry(shape, repeat):
    out = M.render(M.gradient((12.5, 2.0), (12.5, 2.0), shape, repeat), GC.lut(), 67, 5)
    assert (out == GC.lut()[0]).all() and GC.lut()[0][3] == 255


def test_the_rainbow_preset_s_table():
    """entry 128: t = 128 / 255 = 0.50196 lies between the stops at 0.5 (0, 200, 0) and 0.67 (0, 100, 255): local_t = 0.00196 / 0.17 = 0.011534, so
    g = 200 - 100 * 0.011534 = 198.85 -> 199 and b = 255 * 0.011534 = 2.94 -> 3; the ends are the first and the last stop"""
    table = M.build_lut(M.preset_stops("rainbow", (1, 2, 3, 4), (5, 6, 7, 8)))
    assert tuple(table[0]) == (255, 0, 0, 255) and tuple(table[128]) == (0, 199, 3, 255) and tuple(table[255]) == (148, 0, 211, 255)


def test_the_identity_quad_is_a_two_stage_mean_of_four_neighbours():
    """64 x 64: u = (ox + 0.5) / 64 and the four corner products are exact, so the sample sits at exactly ox + 0.5: both fractions are 0.5 and each lerp is the
    mean of two bytes rounded half up; the last column and row read the edge pixel twice"""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    sx, sy = M.crop_coordinates([(0, 0), (64, 0), (64, 64), (0, 64)], 64, 64)
    assert np.array_equal(sx, np.broadcast_to(np.arange(64, dtype=np.float32) + 0.5, (64, 64))) and np.array_equal(sy, sx.T)
    p = img.astype(np.int32)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    row = (p + right + 1) // 2
    below = np.concatenate([row[1:], row[-1:]], axis=0)
    assert np.array_equal(M.crop([(0, 0), (64, 0), (64, 64), (0, 64)], img), ((row + below + 1) // 2).astype(np.uint8))


def test_premultiply_and_commit_known_answers():
    px = lambda *v: np.array(v, np.uint8).reshape(1, 1, 4)
    assert tuple(M.premultiply(px(255, 128, 1, 128))[0, 0]) == (128, 64, 1, 128)          # (255 * 128 + 128) / 255 = 128, (128 * 128 + 128) / 255 = 64, 256 / 255 = 1
    assert tuple(M.commit(px(0, 0, 0, 255), px(255, 255, 255, 128), False)[0, 0]) == (128, 128, 128, 255)
    assert tuple(M.commit(px(9, 8, 7, 200), px(1, 2, 3, 0), False)[0, 0]) == (9, 8, 7, 200)      # preview alpha 0: untouched
    assert tuple(M.commit(px(9, 8, 7, 200), px(1, 2, 3, 255), False)[0, 0]) == (1, 2, 3, 255)
    assert tuple(M.commit(px(9, 8, 7, 0), px(1, 2, 3, 77), False)[0, 0]) == (1, 2, 3, 77)
    assert tuple(M.commit(px(9, 8, 7, 200), px(255, 255, 255, 255), True)[0, 0]) == (9, 8, 7, 0)   # full strength erases
    assert tuple(M.commit(px(9, 8, 7, 200), px(255, 255, 255, 51), True)[0, 0]) == (9, 8, 7, 160)  # 200 * (1 - 0.2)


# ---- the library's host functions against the model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from paintfe_amd import _lib
    return _lib.load()


CTX_ENTRY_POINTS = ["pfx_gradient_render_dev", "pfx_gradient_render", "pfx_gradient_commit_dev", "pfx_gradient_commit", "pfx_gradient_apply_dev",
                    "pfx_perspective_crop_dev", "pfx_perspective_crop"]
HOST_ENTRY_POINTS = ["pfx_gradient_build_lut", "pfx_gradient_preset_stops", "pfx_gradient_bake_eraser_lut", "pfx_gradient_drag_scale", "pfx_perspective_crop_plan"]


def test_the_abi_declares_and_exports_every_entry_point(lib):
    header = open(os.path.join(ROOT, "include", "pfx.h")).read()
    for name in CTX_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*pfx_ctx\s*\*\s*ctx\b" % name, header), name
        getattr(lib, name).restype = C.c_int
    for name in HOST_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(lib, name), name
    assert lib.pfx_abi_version() == 1
    null, zero = C.c_void_p(None), C.c_uint32(0)
    assert lib.pfx_gradient_render_dev(null, None, null, null, zero, zero, null, null) != OK       # a NULL context is an error, not a fault
    assert lib.pfx_gradient_render(null, None, null, null, zero, zero, null, null) != OK
    assert lib.pfx_gradient_commit_dev(null, null, null, zero, zero, 0) != OK and lib.pfx_gradient_commit(null, null, null, zero, zero, 0) != OK
    assert lib.pfx_gradient_apply_dev(null, None, null, null, null, zero, zero) != OK
    assert lib.pfx_perspective_crop_dev(null, None, None, None, zero, zero, zero) != OK and lib.pfx_perspective_crop(null, None, null, null, 0, zero, zero) != OK


def test_the_binding_lays_the_structs_out_as_the_header_does():
    from paintfe_amd import _lib
    assert C.sizeof(_lib.GradientStop) == 8 and _lib.GradientStop.color.offset == 4
    assert C.sizeof(_lib.Gradient) == 32 and _lib.Gradient.shape.offset == 16 and _lib.Gradient.preview_scale.offset == 28


LUT_CASES = {
    "none": [],
    "one": [(0.4, (9, 8, 7, 6))],
    "unsorted": GC.STOPS,
    "duplicates": [(0.5, (255, 0, 0, 255)), (0.2, (0, 0, 0, 0)), (0.5, (0, 255, 0, 128)), (0.5, (0, 0, 255, 64)), (0.9, (10, 20, 30, 40))],
    "outside": [(-0.5, (0, 0, 0, 255)), (1.5, (255, 255, 255, 0)), (0.25, (200, 100, 50, 128))],
    "all-equal": [(0.5, (1, 2, 3, 4)), (0.5, (5, 6, 7, 8))],
    "rainbow": M.preset_stops("rainbow", (0, 0, 0, 0), (0, 0, 0, 0)),
    "tie-at-an-entry": [(0.0, (0, 0, 0, 0)), (51 / 255, (255, 255, 255, 255)), (102 / 255, (0, 0, 0, 0)), (1.0, (255, 1, 2, 3))],
}


@pytest.mark.parametrize("name", sorted(LUT_CASES))
def test_the_lut_builder_equals_the_model(lib, name):
    from paintfe_amd import gradient_lut
    assert np.array_equal(gradient_lut(LUT_CASES[name]), M.build_lut(LUT_CASES[name]))


def test_the_duplicate_stops_keep_their_order():
    """a stable sort: of three stops at 0.5 the FIRST one ends the pair that brackets t below 0.5, the first pair with left <= t <= right wins above it"""
    table = M.build_lut(LUT_CASES["duplicates"])
    assert tuple(table[127]) != tuple(table[128]) and table[127][0] > 200 and table[127][1] == 0     # towards (255, 0, 0, 255), the first of the three
    assert table[128][2] > 200                                                                      # from (0, 0, 255, 64), the last of the three


def test_the_lut_builder_refusals(lib):
    from paintfe_amd import _lib
    lut = np.full((256, 4), 7, np.uint8)
    stops = (_lib.GradientStop * 2)(_lib.GradientStop(0.0, (C.c_uint8 * 4)(1, 2, 3, 4)), _lib.GradientStop(float("nan"), (C.c_uint8 * 4)(1, 2, 3, 4)))
    assert lib.pfx_gradient_build_lut(stops, 2, lut.ctypes.data_as(C.c_void_p)) == ERR_INVALID and (lut == 7).all()
    stops[1].position = float("inf")
    assert lib.pfx_gradient_build_lut(stops, 2, lut.ctypes.data_as(C.c_void_p)) == ERR_INVALID and (lut == 7).all()
    assert lib.pfx_gradient_build_lut(None, 2, lut.ctypes.data_as(C.c_void_p)) == ERR_INVALID and lib.pfx_gradient_build_lut(stops, 1, None) == ERR_INVALID
    assert lib.pfx_gradient_build_lut(None, 0, lut.ctypes.data_as(C.c_void_p)) == OK and not lut.any()
    assert lib.pfx_gradient_bake_eraser_lut(None, lut.ctypes.data_as(C.c_void_p)) == ERR_INVALID and lib.pfx_gradient_bake_eraser_lut(lut.ctypes.data_as(C.c_void_p), None) == ERR_INVALID
    assert lib.pfx_gradient_preset_stops(4, None, None, None, None) == ERR_INVALID


def test_the_eraser_bake_equals_the_model(lib):
    from paintfe_amd import gradient_bake_eraser_lut
    rng = np.random.default_rng(4)
    for table in (GC.lut(), rng.integers(0, 256, (256, 4), dtype=np.uint8), np.full((256, 4), 255, np.uint8)):
        assert np.array_equal(gradient_bake_eraser_lut(table), M.bake_eraser_lut(table))
    white = int(F(F(F(0.299) * F(255.0)) + F(F(0.587) * F(255.0))) + F(F(0.114) * F(255.0)))
    assert tuple(M.bake_eraser_lut(np.full((256, 4), 255, np.uint8))[0]) == (255, 255, 255, white) and white in (254, 255)
    grey = np.tile(np.array([100, 100, 100, 200], np.uint8), (256, 1))
    assert tuple(M.bake_eraser_lut(grey)[0]) == (255, 255, 255, 100 * 200 // 255)


@pytest.mark.parametrize("preset", M.PRESETS)
def test_the_presets_equal_the_model(lib, preset):
    from paintfe_amd import gradient_preset_stops
    got = gradient_preset_stops(preset, (10, 20, 30, 40), (50, 60, 70, 80))
    want = M.preset_stops(preset, (10, 20, 30, 40), (50, 60, 70, 80))
    assert [(F(p), c) for p, c in got] == [(F(p), c) for p, c in want]


def test_the_drag_scale(lib):
    from paintfe_amd import gradient_drag_scale
    assert gradient_drag_scale(1500, 1000) == 1 and gradient_drag_scale(1500001, 1) == 2      # 1 500 000 and 1 500 001 pixels
    for w, h in ((1500, 1000), (1500001, 1), (1920, 1080), (2000, 2000), (2001, 2000), (3840, 2160), (7680, 4320), (16000, 16000), (65535, 65535), (0, 0)):
        assert gradient_drag_scale(w, h) == M.drag_scale(w, h), (w, h)
    assert M.drag_scale(1920, 1080) == 2 and M.drag_scale(2000, 2000) == 2 and M.drag_scale(2001, 2000) == 3 and M.drag_scale(7680, 4320) == 6


PLAN_EXTRA = {
    "clamped-by-the-canvas": (130, 70, [(-40.0, -9.5), (300.0, -2.0), (280.0, 90.0), (-6.0, 75.0)]),     # 130 x 70 after the clamps
    "none": (130, 70, GC.none_quad(130, 70)),
    "wholly-left": (130, 70, [(-50.0, 10.0), (-5.0, 10.0), (-5.0, 60.0), (-50.0, 60.0)]),                  # max_x < min_x = 0: a negative width -> 0 -> None
    "half-rounds-up": (130, 70, [(10.0, 10.0), (12.5, 10.0), (12.5, 11.5), (10.0, 11.5)]),                  # 2.5 x 1.5 -> 3 x 2
    "huge": (130, 70, [(-3.0e38, -3.0e38), (3.0e38, -3.0e38), (3.0e38, 3.0e38), (-3.0e38, 3.0e38)]),
}


def test_the_crop_plan_equals_the_model(lib):
    from paintfe_amd import perspective_crop_plan
    cases = dict(PLAN_EXTRA)
    for w, h in GC.CROP_SIZES:
        for quad, corners in GC.quads(w, h).items():
            cases[f"{w}x{h}-{quad}"] = (w, h, corners)
    for name, (w, h, corners) in cases.items():
        assert perspective_crop_plan(corners, w, h) == M.crop_plan(corners, w, h), name
    assert M.crop_plan(PLAN_EXTRA["clamped-by-the-canvas"][2], 130, 70) == (130, 70) and M.crop_plan(PLAN_EXTRA["none"][2], 130, 70) is None
    assert M.crop_plan(PLAN_EXTRA["wholly-left"][2], 130, 70) is None and M.crop_plan(PLAN_EXTRA["half-rounds-up"][2], 130, 70) == (3, 2)
    ow, oh = C.c_uint32(7), C.c_uint32(7)
    good = (C.c_float * 8)(0, 0, 9, 0, 9, 9, 0, 9)
    assert lib.pfx_perspective_crop_plan(None, 130, 70, C.byref(ow), C.byref(oh)) == ERR_INVALID and lib.pfx_perspective_crop_plan(good, 130, 70, None, None) == ERR_INVALID
    assert lib.pfx_perspective_crop_plan(good, 20000, 20000, C.byref(ow), C.byref(oh)) == ERR_INVALID and lib.pfx_perspective_crop_plan(good, 0, 70, C.byref(ow), C.byref(oh)) == ERR_INVALID
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(8):
            corners = (C.c_float * 8)(0, 0, 9, 0, 9, 9, 0, 9)
            corners[k] = bad
            assert lib.pfx_perspective_crop_plan(corners, 130, 70, C.byref(ow), C.byref(oh)) == ERR_INVALID
    assert (ow.value, oh.value) == (7, 7)


# ---- branch reach of the GPU cases -------------------------------------------------------------------------------------------------------------------------------------
def test_every_shape_and_repeat_takes_both_sides():
    for w, h in GC.SIZES:
        for shape in GC.SHAPE_NAMES:
            for rep in ("clamp", "repeat"):
                for mode in ("colour", "erase"):
                    s = GC.rendered(f"{w}x{h}-{shape}-{rep}-{mode}")[2]
                    assert s["outside"] >= 5 and s["inside"] >= 5, (w, h, shape, rep, mode, s)     # clamped / wrapped, and not
    for w, h in GC.SIZES:
        assert GC.rendered(f"{w}x{h}-linear-repeat-colour")[2]["negative_remainder"] >= 5            # rem_euclid's `r < 0` arm
        assert GC.rendered(f"{w}x{h}-reflected-repeat-colour")[2]["negative_remainder"] >= 5
        assert GC.rendered(f"{w}x{h}-reflected-repeat-colour")[2]["folded"] >= 5                     # t_mod > 1
    assert GC.rendered("130x70-off-canvas")[2]["inside"] == 0 and GC.rendered("130x70-off-canvas")[2]["drawn"] > 1000


def test_selection_and_alpha_branches_are_reached():
    total = {}
    for name in GC.NAMES:
        c, s = GC.CASES[name], GC.rendered(name)[2]
        if c["sel"] is None:
            assert s["dropped"] == 0 and s["grey"] == 0
        else:
            assert s["dropped"] >= 1 or c["w"] == 1, (name, s)
        if c["sel"] == "grey" and c["w"] > 1:
            assert s["grey"] >= 20, (name, s)
        for k, v in s.items():
            total[k] = total.get(k, 0) + v
    assert total["lut_alpha_zero"] >= 100 and total["grey_to_zero"] >= 5 and total["dropped"] >= 1000 and total["drawn"] >= 10000, total
    used = [(GC.CASES[n]["sel"], GC.CASES[n]["premul"]) for n in GC.NAMES]
    assert {s for s, _ in used} == {None, "binary", "grey"} and {p for _, p in used} == {True, False}
    grey = GC.selection(67, 5, "grey")
    assert (grey == 0).any() and (grey == 255).any() and ((grey > 0) & (grey < 255)).any()
    assert (GC.lut()[:, 3] == 0).any() and (GC.lut()[:, 3] == 255).any() and ((GC.lut()[:, 3] > 0) & (GC.lut()[:, 3] < 255)).any()


def test_the_scaled_cases_reach_the_last_column():
    assert M.gen_size(67, 5, 2) == (34, 3) and M.gen_size(67, 5, 3) == (23, 2) and M.gen_size(130, 70, 3) == (44, 24) and M.gen_size(64, 8, 2) == (32, 4)
    assert 33 * 2 == 66 and 22 * 3 == 66 and 43 * 3 == 129           # the last generated column reads the selection's last column
    assert 44 % 4 == 0 and 130 % 4 != 0 and 32 % 4 == 0 and 34 % 4 != 0
    assert GC.BIG[0] * GC.BIG[1] > 8192 * 256 * 4 and GC.BIG[0] % 4 == 0


@pytest.mark.parametrize("name,is_eraser", GC.COMMITS)
def test_commit_sees_every_pair_of_alphas(name, is_eraser):
    c = GC.CASES[name]
    pa, la = GC.rendered(name)[0][..., 3], GC.layer(c["w"], c["h"])[..., 3]
    kind = lambda a: np.where(a == 0, 0, np.where(a == 255, 2, 1))
    pairs = set(zip(kind(pa).ravel().tolist(), kind(la).ravel().tolist()))
    assert pairs == {(p, l) for p in range(3) for l in range(3)}, pairs
    assert not np.array_equal(GC.committed(name, is_eraser), GC.layer(c["w"], c["h"]))


def test_the_crop_cases_hit_every_clamp():
    for w, h in GC.CROP_SIZES:
        s = GC.cropped(w, h, "beyond")[1]
        assert min(s["left"], s["right"], s["above"], s["below"], s["x1_clamped"], s["y1_clamped"], s["inside"]) >= 3, (w, h, s)
        s = GC.cropped(w, h, "inside")[1]
        assert s["left"] == s["right"] == s["above"] == s["below"] == 0 and s["inside"] >= 100
        assert GC.cropped(w, h, "identity")[0].shape == (h, w, 4)
        assert M.crop_plan(GC.none_quad(w, h), w, h) is None and M.crop(GC.none_quad(w, h), GC.layer(w, h)) is None
        flipped = GC.cropped(w, h, "flipped")[0]
        assert flipped.shape[0] >= 2 and not np.array_equal(flipped, GC.cropped(w, h, "inside")[0][:flipped.shape[0], :flipped.shape[1]])
