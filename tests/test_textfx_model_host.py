"""The text-style model (tests/textfx_model.py) and cases (tests/textfx_cases.py) on the host: known answers worked out by hand from effects.rs, the u8 disc
form against the tap-by-tap f32 dilate_mask, the region rule, the conditions that keep a case from passing empty, and the C ABI's host-only part.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from . import textfx_cases as TC
from . import textfx_model as M

F = np.float32
OK, ERR_INVALID = 0, -1


# ---- known answers: one pixel (200, 100, 50, 128) in the middle of 3 x 3 -----------------------------------------------------------------------------------------------
def one_pixel():
    t = np.zeros((3, 3, 4), np.uint8)
    t[1, 1] = (200, 100, 50, 128)
    return t


def lit(out):
    """{(x, y): rgba} of the pixels that are not zero"""
    return {(int(x), int(y)): tuple(int(v) for v in out[y, x]) for y, x in zip(*np.nonzero(out.any(axis=-1)))}


def test_no_effect_is_the_text_over_zero():
    # out_a = 128 + 0; colour = sc * 128 / 128
    assert lit(M.apply(one_pixel(), {})[0]) == {(1, 1): (200, 100, 50, 128)}


def test_outline_outside_one_pixel():
    # the disc of radius 1 is a plus: the four neighbours see coverage 128 / 255, clamp(c - 0) * (255 / 255) * 255 rounds to 128; the centre's ring alpha is 0
    got = lit(M.apply(one_pixel(), dict(outline=dict(width=1.0, color=(10, 20, 30, 255))))[0])
    ring = (10, 20, 30, 128)
    assert got == {(1, 0): ring, (0, 1): ring, (2, 1): ring, (1, 2): ring, (1, 1): (200, 100, 50, 128)}


def test_outline_center_draws_the_outside_half_only():
    # width 2 at Center is radius 1 outside and nothing inside: the same picture as Outside at width 1
    a = M.apply(one_pixel(), dict(outline=dict(width=2.0, position="center", color=(10, 20, 30, 255))))[0]
    b = M.apply(one_pixel(), dict(outline=dict(width=1.0, position="outside", color=(10, 20, 30, 255))))[0]
    assert np.array_equal(a, b)


def test_outline_inside_one_pixel():
    # eroded = 0 (a transparent neighbour is in the plus), so sa = round(128 / 255 * 255) = 128 over the text's (200, 100, 50, 128):
    # inv = 127, out_a = 128 + 128 * 127 / 255 = 128 + 63 = 191; r = (10 * 128 + 200 * 128 * 127 / 255) / 191 = (1280 + 12749) / 191 = 73;
    # g = (2560 + 6374) / 191 = 46; b = (3840 + 3187) / 191 = 36
    assert lit(M.apply(one_pixel(), dict(outline=dict(width=1.0, position="inside", color=(10, 20, 30, 255))))[0]) == {(1, 1): (73, 46, 36, 191)}


def test_shadow_unblurred_one_pixel():
    # shifted right by round(0.5) = 1 (half away from zero): alpha = round(128 / 255 * 180) = round(90.35) = 90 at (2, 1); round(-0.5) = -1 moves it left
    s = dict(color=(1, 2, 3, 180), offset_x=0.5, offset_y=0.0, blur_radius=0.0, spread=0.0)
    assert lit(M.apply(one_pixel(), dict(shadow=s))[0]) == {(1, 1): (200, 100, 50, 128), (2, 1): (1, 2, 3, 90)}
    assert lit(M.apply(one_pixel(), dict(shadow={**s, "offset_x": -0.5}))[0]) == {(1, 1): (200, 100, 50, 128), (0, 1): (1, 2, 3, 90)}


def test_shadow_spread_one_pixel():
    # spread 1 grows the shifted pixel into a plus around (2, 1); its left arm lies under the text: 90 under (200, 100, 50, 128) is
    # out_a = 128 + 90 * 127 / 255 = 128 + 44 = 172, r = (200 * 128 + 1 * 90 * 127 / 255) / 172 = (25600 + 44) / 172 = 149, g = (12800 + 89) / 172 = 74,
    # b = (6400 + 134) / 172 = 37; the arm at (3, 1) is outside the image
    s = dict(color=(1, 2, 3, 180), offset_x=1.0, offset_y=0.0, blur_radius=0.0, spread=1.0)
    sh = (1, 2, 3, 90)
    assert lit(M.apply(one_pixel(), dict(shadow=s))[0]) == {(2, 0): sh, (2, 1): sh, (2, 2): sh, (1, 1): (149, 74, 37, 172)}


def test_inner_shadow_unblurred_one_pixel():
    # shifted by (1, 0) the inverted mask at the centre reads the transparent (0, 1): 1.0; sa = round(1.0 * 128 * (128 / 255)) = round(64.25) = 64 over the text:
    # inv = 191, out_a = 64 + 128 * 191 / 255 = 64 + 95 = 159; r = (200 * 128 * 191 / 255) / 159 = 19174 / 159 = 120; g = 9587 / 159 = 60; b = 4793 / 159 = 30
    i = dict(color=(0, 0, 0, 128), offset_x=1.0, offset_y=0.0, blur_radius=0.0)
    assert lit(M.apply(one_pixel(), dict(inner_shadow=i))[0]) == {(1, 1): (120, 60, 30, 159)}
    # read from outside the image the inverted mask is 1.0 as well: a shift by 2 gives the same pixel
    assert lit(M.apply(one_pixel(), dict(inner_shadow={**i, "offset_x": 2.0}))[0]) == {(1, 1): (120, 60, 30, 159)}
    # unshifted it reads its own coverage: sa = round((1 - 128 / 255) * 128 * (128 / 255)) = round(31.999) = 32;
    # inv = 223, out_a = 32 + 128 * 223 / 255 = 32 + 111 = 143; r = (200 * 128 * 223 / 255) / 143 = 22387 / 143 = 156; g = 11193 / 143 = 78; b = 5596 / 143 = 39
    assert lit(M.apply(one_pixel(), dict(inner_shadow={**i, "offset_x": 0.0}))[0]) == {(1, 1): (156, 78, 39, 143)}


def test_gradient_one_pixel():
    # x = 1, scale 2: t = 0.5; r = round(127.5) = 128, b = round(127.5) = 128, alpha = round(255 * 128 / 255) = 128
    g = dict(start_color=(255, 0, 0, 255), end_color=(0, 0, 255, 255), angle_degrees=0.0, scale=2.0, offset=(0.0, 0.0), repeat=False)
    assert lit(M.apply(one_pixel(), dict(gradient_fill=g))[0]) == {(1, 1): (128, 0, 128, 128)}
    # an offset of 3 makes the projection -1: clamped to 0 without repeat; with repeat rem_euclid(-1, 1) = 0 as well; -0.75 wraps to 0.25
    assert lit(M.apply(one_pixel(), dict(gradient_fill={**g, "offset": (3.0, 0.0)}))[0]) == {(1, 1): (255, 0, 0, 128)}
    assert lit(M.apply(one_pixel(), dict(gradient_fill={**g, "offset": (3.0, 0.0), "repeat": True}))[0]) == {(1, 1): (255, 0, 0, 128)}
    # r = round(255 * 0.75) = round(191.25) = 191, b = round(63.75) = 64
    assert lit(M.apply(one_pixel(), dict(gradient_fill={**g, "offset": (2.5, 0.0), "repeat": True}))[0]) == {(1, 1): (191, 0, 64, 128)}
    # the gradient wins over a texture
    tex = np.array([[[9, 8, 7, 100]]], np.uint8)
    assert lit(M.apply(one_pixel(), dict(gradient_fill=g, texture_fill=dict(texture_width=1, texture_height=1)), tex)[0]) == {(1, 1): (128, 0, 128, 128)}


def test_texture_one_pixel():
    tex = np.array([[[9, 8, 7, 100], [19, 18, 17, 255]]], np.uint8)   # 2 x 1
    t = dict(texture_width=2, texture_height=1, scale=1.0, offset=(0.0, 0.0))
    # x = 1 -> texel 1: alpha = min(round(128 / 255 * 255), 255) = 128; offset 1 -> texel 0: min(128, 100)
    assert lit(M.apply(one_pixel(), dict(texture_fill=t), tex)[0]) == {(1, 1): (19, 18, 17, 128)}
    assert lit(M.apply(one_pixel(), dict(texture_fill={**t, "offset": (1.0, 0.0)}), tex)[0]) == {(1, 1): (9, 8, 7, 100)}
    # offset 2: fmod(-1, 2) = -1, + 2 = 1 -> texel 1; scale below 0.01 is 0.01: x / 0.01 = 100 -> texel 0
    assert lit(M.apply(one_pixel(), dict(texture_fill={**t, "offset": (2.0, 0.0)}), tex)[0]) == {(1, 1): (19, 18, 17, 128)}
    assert lit(M.apply(one_pixel(), dict(texture_fill={**t, "scale": 0.001}), tex)[0]) == {(1, 1): (9, 8, 7, 100)}
    # no texture, or a zero side: the text itself
    assert lit(M.apply(one_pixel(), dict(texture_fill={**t, "texture_width": 0}), tex)[0]) == {(1, 1): (200, 100, 50, 128)}
    assert lit(M.apply(one_pixel(), dict(texture_fill=t), None)[0]) == {(1, 1): (200, 100, 50, 128)}


SPANS = {1.0: {-1: 0, 0: 1, 1: 0},
         1.25: {-1: 0, 0: 1, 1: 0},                                   # rows +-2 are within ceil(r) but 4 > 1.5625
         2.0: {-2: 0, -1: 1, 0: 2, 1: 1, 2: 0},
         7.3: {-7: 2, -6: 4, -5: 5, -4: 6, -3: 6, -2: 7, -1: 7, 0: 7, 1: 7, 2: 7, 3: 6, 4: 6, 5: 5, 6: 4, 7: 2}}   # r^2 = 53.29: 49 + 4, 36 + 16, 25 + 25, 16 + 36, 9 + 36, 4 + 49


@pytest.mark.parametrize("radius", sorted(SPANS))
def test_disc_spans(radius):
    assert dict(M.disc_spans(radius)) == SPANS[radius]


def test_disc_tap_counts():
    assert sum(2 * half + 1 for _, half in M.disc_spans(5.0)) == 81 and sum(2 * half + 1 for _, half in M.disc_spans(50.0)) == 7845
    assert M.disc_spans(0.5) == [(0, 0)]   # ceil(0.5) = 1, but the rows +-1 fail: nothing changes


def test_the_library_walks_the_same_spans():
    from paintfe_amd import textfx_span
    for radius in (0.5, 1.0, 1.25, 2.0, 7.3, 30.0, 49.99, 50.0, 63.5, 64.0):
        reach = int(np.ceil(F(radius)))
        want = dict(M.disc_spans(radius))
        assert {dy: textfx_span(radius, dy) for dy in range(-reach - 1, reach + 2)} == {dy: want.get(dy, -1) for dy in range(-reach - 1, reach + 2)}, radius
    assert textfx_span(64.5, 0) == -1 and textfx_span(0.0, 0) == -1 and textfx_span(float("nan"), 0) == -1


# ---- the u8 disc form is the f32 dilate_mask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.5, 1.0, 1.25, 2.0, 3.7, 7.3, 12.0])
def test_u8_disc_is_the_f32_dilation(radius):
    rng = np.random.default_rng(int(radius * 100))
    for shape in ((23, 37), (5, 41)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        a[rng.random(shape) < 0.5] = 0
        a[rng.random(shape) < 0.2] = 255
        cov = M.coverage(a)
        assert np.array_equal(M.coverage(M.disc_max_u8(a, radius)), M.dilate_mask(cov, radius))
        eroded_f32 = np.maximum(F(1.0) - M.dilate_mask(F(1.0) - cov, radius), F(0))
        eroded_u8 = np.maximum(F(1.0) - (F(1.0) - M.coverage(M.disc_min_u8(a, radius))), F(0))
        assert np.array_equal(eroded_u8, eroded_f32)
        # the shadow's alpha: scaling by the colour's alpha before the dilation or after it
        scaled = M.round_u8(cov * F(180)).astype(np.uint8)
        assert np.array_equal(M.disc_max_u8(scaled, radius), M.round_u8(M.dilate_mask(cov, radius) * F(180)))
    if radius == 0.5:
        assert np.array_equal(M.disc_max_u8(a, radius), a) and np.array_equal(M.disc_min_u8(a, radius), a)


# ---- bounds and the region rule ----------------------------------------------------------------------------------------------------------------------------------------
def test_tight_bounds():
    t = np.zeros((9, 11, 4), np.uint8)
    assert M.tight_bounds(t) == (0, 0, 0, 0)
    t[..., :3] = 77                      # colour without alpha is not text
    assert M.tight_bounds(t) == (0, 0, 0, 0)
    t[4, 3, 3] = 1
    assert M.tight_bounds(t) == (3, 4, 1, 1)
    t[8, 10, 3] = 255
    t[0, 5, 3] = 9
    assert M.tight_bounds(t) == (3, 0, 8, 9)


DEFAULTS = dict(outline={}, shadow={}, inner_shadow={})
PLANS = [   # effects, canvas, bounds, the rectangle worked out by hand: x, y, w, h, pad_px, full_canvas
    (DEFAULTS, (300, 200), (10, 10, 50, 20), (0, 0, 83, 53, 23, 0)),          # pad = 4 + 4 + 15 + 0 = 23 beats 2 + 2 and 2 + 2 + 9; clamped at the left and top
    (DEFAULTS, (300, 200), (100, 80, 50, 20), (77, 57, 96, 66, 23, 0)),
    (DEFAULTS, (300, 200), (260, 170, 40, 30), (237, 147, 63, 53, 23, 0)),    # clamped at the right and bottom
    ({}, (100, 100), (0, 4, 100, 42), (0, 0, 100, 50, 4, 1)),                 # no member: pad_px = 4; 100 x 50 * 2 = the canvas: the whole canvas
    ({}, (100, 100), (0, 4, 100, 41), (0, 0, 100, 49, 4, 0)),                 # one row less: the region
    (dict(outline=dict(width=7.3)), (300, 200), (100, 80, 5, 5), (90, 70, 25, 25, 10, 0)),     # ceil(7.3) + 2
    (dict(outline=dict(width=0.5)), (300, 200), (100, 80, 5, 5), (96, 76, 13, 13, 4, 0)),      # ceil(0.5) + 2 = 3: the floor of 4
    (dict(shadow=dict(offset_x=-2.5, offset_y=2.5, blur_radius=0.5, spread=0.6)), (300, 200), (100, 80, 5, 5), (92, 72, 21, 21, 8, 0)),   # ceil(2.5 + 2.5 + 1.5 + 0.6 = 7.1)
    (dict(inner_shadow=dict(offset_x=0.0, offset_y=0.0, blur_radius=50.0)), (300, 200), (140, 90, 5, 5), (0, 0, 295, 200, 150, 1)),
    (DEFAULTS, (300, 200), (0, 0, 0, 0), (0, 0, 0, 0, 0, 0)),
]


@pytest.mark.parametrize("k", range(len(PLANS)))
def test_region_rule(k):
    effects, canvas, bounds, want = PLANS[k]
    r = M.region(effects, canvas[0], canvas[1], bounds)
    assert (r["x"], r["y"], r["w"], r["h"], r["pad_px"], r["full_canvas"]) == want
    from paintfe_amd import text_effects, text_effects_plan
    g = text_effects_plan(text_effects(canvas, **effects), bounds)
    assert (g.x, g.y, g.w, g.h, g.pad_px, g.full_canvas) == want


def test_layer_documents_take_the_intended_paths():
    regions = {name: TC.expected_layer(name)[1] for name in TC.DOCUMENTS}
    assert regions["corner"]["full_canvas"] == 0 and regions["corner"]["x"] > 0 and regions["corner"]["y"] > 0
    assert regions["spread-out"]["full_canvas"] == 1
    assert regions["two-edges"]["full_canvas"] == 0 and regions["two-edges"]["x"] == 0 and regions["two-edges"]["y"] == 0
    assert regions["no-text"]["w"] == 0 and not TC.expected_layer("no-text")[0].any()
    # the region path is not the full-canvas path in disguise: the corner document's gradient starts at the region's origin
    text, effects = TC.document("corner")
    assert not np.array_equal(TC.expected_layer("corner")[0], M.apply(text, effects)[0])


# ---- no case passes empty ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_input_mix():
    a = TC.text_of(TC.MEASURED)[..., 3]
    zero, partial, full = (a == 0).mean(), ((a > 0) & (a < 255)).mean(), (a == 255).mean()
    print(f"alpha mix at {TC.MEASURED}: {zero:.2f} zero, {partial:.2f} partial, {full:.2f} full")
    assert partial > 0.05 and full > 0.05 and zero > 0.5
    t = TC.text_of(TC.MEASURED)
    assert not t[a == 0].any()


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_conditions(name):
    _, stages, kind = TC.CASES[name]
    plain = TC.expected("none", TC.MEASURED)[0]
    out, counts = TC.expected(name, TC.MEASURED)
    differing = float((out != plain).any(axis=-1).mean())
    print(f"{name}: {differing:.3f} of the pixels differ from the no-effect output; (partial, full) per stage: {counts}")
    if kind == "draws":
        assert differing >= 0.01
        for s in stages:
            assert counts[s][0] >= 50, (s, counts[s])
        for size in TC.SIZES:
            assert not np.array_equal(TC.expected(name, size)[0], TC.expected("none", size)[0]), size
    elif kind == "plain":
        for size in TC.SIZES:
            assert np.array_equal(TC.expected(name, size)[0], TC.expected("none", size)[0]), size
    else:
        for size in TC.PLAIN_SMALL_SIZES:
            assert np.array_equal(TC.expected(name, size)[0], TC.expected("none", size)[0]), size


def test_the_half_boundaries():
    """spread 0.5 and blur 0.5 are off, 0.51 is on"""
    size = TC.MEASURED
    d = TC.effects_of("shadow-spread-0.5")["shadow"]
    assert np.array_equal(TC.expected("shadow-spread-0.5", size)[0], M.apply(TC.text_of(size), dict(shadow={**d, "spread": 0.0}))[0])
    assert not np.array_equal(TC.expected("shadow-spread-0.5", size)[0], M.apply(TC.text_of(size), dict(shadow={**d, "spread": 1.0}))[0])   # (a disc of radius 0.51 is one pixel)
    b = TC.effects_of("shadow-blur-0.5")["shadow"]
    assert np.array_equal(TC.expected("shadow-blur-0.5", size)[0], M.apply(TC.text_of(size), dict(shadow={**b, "blur_radius": 0.0}))[0])
    assert not np.array_equal(TC.expected("shadow-blur-0.5", size)[0], TC.expected("shadow-blur-0.51", size)[0])


# ---- the C ABI, host only --------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_host_only_answers():
    from paintfe_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("pfx_text_effects_dev", "pfx_text_effects", "pfx_text_effects_plan", "pfx_text_layer_effects_dev"):
        assert hasattr(lib, name), name
    assert lib.pfx_abi_version() == 1
    from paintfe_amd import text_effects
    fx = text_effects((300, 200), **DEFAULTS)
    assert C.sizeof(fx) == 108
    null = C.c_void_p(None)
    buf = np.zeros(16, np.uint8).ctypes.data_as(C.c_void_p)
    # a NULL context is an error whatever else is passed; so is a NULL descriptor
    assert lib.pfx_text_effects_dev(null, C.byref(fx), buf, null, buf) == ERR_INVALID
    assert lib.pfx_text_effects(null, C.byref(fx), buf, null, buf) == ERR_INVALID
    assert lib.pfx_text_layer_effects_dev(null, C.byref(fx), buf, null, buf, null) == ERR_INVALID
    assert lib.pfx_text_effects_dev(null, null, null, null, null) == ERR_INVALID
    region = _lib.TextRegion()
    bounds = (C.c_uint32 * 4)(10, 10, 50, 20)
    assert lib.pfx_text_effects_plan(null, bounds, C.byref(region)) == ERR_INVALID
    assert lib.pfx_text_effects_plan(C.byref(fx), null, C.byref(region)) == ERR_INVALID
    assert lib.pfx_text_effects_plan(C.byref(fx), bounds, null) == ERR_INVALID
    # the known case of PLANS[0], bit for bit
    assert lib.pfx_text_effects_plan(C.byref(fx), bounds, C.byref(region)) == OK
    assert bytes(region) == np.array([0, 0, 83, 53, 23, 0], np.uint32).tobytes()
    # bounds outside the canvas, a float that is not finite, a position outside the enum, a size outside the document limit
    assert lib.pfx_text_effects_plan(C.byref(fx), (C.c_uint32 * 4)(280, 10, 50, 20), C.byref(region)) == ERR_INVALID
    for field, value in (("shadow_spread", float("nan")), ("gradient_scale", float("inf")), ("outline_position", 3), ("outline_position", -1), ("width", 0), ("height", 1 << 30)):
        bad = text_effects((300, 200), **DEFAULTS)
        setattr(bad, field, value)
        assert lib.pfx_text_effects_plan(C.byref(bad), bounds, C.byref(region)) == ERR_INVALID, field
