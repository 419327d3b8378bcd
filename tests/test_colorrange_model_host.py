"""tests/colorrange_model.py held to a plain pixel-loop transcription of the reference (src/ops/adjustments.rs :883-937, :944-1012, :1616-1673, :1705-1787) on
small images, to hand-derived answers and to the oracle's rgb_to_hsl; and tests/colorrange_cases.py held to what its cases are there for, so that no device
test passes vacuously.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from . import colorrange_cases as CC
from . import colorrange_model as CM
from . import oracle_lib as O

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- the transcription: scalars, branches, loops
def t_round(v):
    v = float(v)
    return math.copysign(math.floor(abs(v) + 0.5), v)


def t_rgb_to_hsl(r, g, b):
    mx, mn = max(max(r, g), b), min(min(r, g), b)
    l = (mx + mn) / F(2.0)
    if abs(mx - mn) < F(1e-6):
        return F(0.0), F(0.0), l
    d = mx - mn
    s = d / (F(2.0) - mx - mn) if l > F(0.5) else d / (mx + mn)
    if abs(mx - r) < F(1e-6):
        h = (g - b) / d
        if h < 0:
            h = h + F(6.0)
        h = h / F(6.0)
    elif abs(mx - g) < F(1e-6):
        h = ((b - r) / d + F(2.0)) / F(6.0)
    else:
        h = ((r - g) / d + F(4.0)) / F(6.0)
    return h, s, l


def t_hue_to_rgb(p, q, t):
    if t < 0:
        t = t + F(1.0)
    if t > F(1.0):
        t = t - F(1.0)
    if t < F(1.0) / F(6.0):
        return p + (q - p) * F(6.0) * t
    if t < F(1.0) / F(2.0):
        return q
    if t < F(2.0) / F(3.0):
        return p + (q - p) * (F(2.0) / F(3.0) - t) * F(6.0)
    return p


def t_hsl_to_rgb(h, s, l):
    if abs(s) < F(1e-6):
        return l, l, l
    q = l * (F(1.0) + s) if l < F(0.5) else l + s - l * s
    p = F(2.0) * l - q
    return t_hue_to_rgb(p, q, h + F(1.0) / F(3.0)), t_hue_to_rgb(p, q, h), t_hue_to_rgb(p, q, h - F(1.0) / F(3.0))


def t_band_weight(h_deg, centre):
    dist = np.fmod(abs(h_deg - centre), F(360.0))
    if dist > F(180.0):
        dist = F(360.0) - dist
    if dist <= F(30.0):
        return F(1.0)
    if dist < F(45.0):
        return F(1.0) - (dist - F(30.0)) / F(15.0)
    return F(0.0)


def t_hsl_bands(img, gh, gs, gl, bands, mask):
    """the dense result: the closure of :1647-1673 per selected pixel (:82-101)"""
    bands = list(bands) + [(0.0, 0.0, 0.0)] * (6 - len(bands))
    g_sat = F(1.0) + F(gs) / F(100.0)
    g_light = F(gl) * F(255.0) / F(100.0)
    out = img.copy()
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            if mask is not None and mask[y, x] == 0:
                continue
            r, g, b = (F(int(v)) for v in img[y, x, :3])
            h, s, l = t_rgb_to_hsl(r / F(255.0), g / F(255.0), b / F(255.0))
            h_deg = h * F(360.0)
            extra_hue, factor, extra_light = F(gh), g_sat, g_light
            for i in range(6):
                wgt = t_band_weight(h_deg, F(CM.BAND_CENTERS[i]))
                if wgt > 0:
                    extra_hue = extra_hue + F(bands[i][0]) * wgt
                    factor = factor + F(bands[i][1]) / F(100.0) * wgt
                    extra_light = extra_light + F(bands[i][2]) * F(255.0) / F(100.0) * wgt
            nh = np.fmod(np.fmod(h + extra_hue / F(360.0), F(1.0)) + F(1.0), F(1.0))
            ns = min(max(s * factor, F(0.0)), F(1.0))
            rgb = t_hsl_to_rgb(nh, ns, l)
            for k in range(3):
                out[y, x, k] = int(min(max(t_round(rgb[k] * F(255.0) + extra_light), 0.0), 255.0))
    return out


def t_color_range(img, hc, ht, smin, fuzz, mode, base):
    hue_center = F(hc) / F(360.0)
    hue_tol = max(F(ht) / F(360.0), F(0.001))
    fz = min(max(F(fuzz), F(0.001)), F(1.0))
    expo = F(1.0) / max(fz, F(0.01))
    new = np.zeros(img.shape[:2], np.uint8)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            if img[y, x, 3] == 0:
                continue
            h, s, _ = t_rgb_to_hsl(*(F(int(v)) / F(255.0) for v in img[y, x, :3]))
            if s < F(smin):
                continue
            diff = abs(h - hue_center)
            if diff > F(0.5):
                diff = F(1.0) - diff
            if diff > hue_tol:
                continue
            weight = F(1.0) - CM.powf_glibc(np.asarray([diff / hue_tol], F), expo)[0]
            new[y, x] = int(min(max(weight * F(255.0), F(0.0)), F(255.0)))
    out = np.zeros_like(new)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            a, b = int(new[y, x]), 0 if base is None else int(base[y, x])
            out[y, x] = (a, max(a, b), max(b - a, 0), a * b // 255)[mode]
    return out


def t_histogram(img, mask):
    hist = np.zeros((4, 256), np.uint32)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            if mask is not None and mask[y, x] == 0:
                continue
            r, g, b, a = (int(v) for v in img[y, x])
            if a == 0:
                continue
            lum = int(t_round(F(0.2126) * F(r) + F(0.7152) * F(g) + F(0.0722) * F(b)))
            hist[0, r] += 1; hist[1, g] += 1; hist[2, b] += 1; hist[3, min(lum, 255)] += 1
    return hist


def small_images():
    return {"noise": CC.noise(23, 17, 3), "knee": CC.fit(CC.knee_pixels(), 46, 33), "lattice": CC.fit(CC.lattice(), 31, 19)}


# ---------------------------------------------------------------------------------------------------------------- model against transcription and oracle
@pytest.mark.parametrize("name", ["noise", "knee", "lattice"])
def test_model_equals_the_pixel_loop_transcription(name):
    img = small_images()[name]
    h, w = img.shape[:2]
    mask = CC.selection(w, h, 9)
    for m in (None, mask):
        assert np.array_equal(CM.histogram(img, m), t_histogram(img, m))
    for set_name in ("global", "band1", "six", "max", "min"):
        gh, gs, gl, bands = CC.BAND_SETS[set_name]
        for m in (None, mask):
            assert np.array_equal(CM.hsl_bands(img, gh, gs, gl, bands, mask=m, sparse=CM.DENSE), t_hsl_bands(img, gh, gs, gl, bands, m)), (set_name, m is None)
    base = CC.grey_base(w, h)
    for i, s in enumerate(CC.RANGE_SETS):
        mode = i % 4
        got, amb = CM.color_range(img, *s, combine=mode, base=base)
        want = t_color_range(img, *s, mode, base)
        assert np.array_equal(got[~amb], want[~amb]), s
        glibc, _ = CM.color_range(img, *s, combine=mode, base=base, flavour="glibc")
        assert np.array_equal(glibc, want), s


def test_model_rgb_to_hsl_equals_the_oracle():
    px = np.concatenate([CC.knee_pixels()[::7, :3], CC.noise(40, 40, 1).reshape(-1, 4)[:, :3], [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 0, 0]]])
    h, s, l = CM.rgb_to_hsl(*(px[:, k].astype(F) / F(255.0) for k in range(3)))
    oh, os_, ol = C.c_float(), C.c_float(), C.c_float()
    for i, (r, g, b) in enumerate(px):
        O.lib().pfxo_rgb_to_hsl(C.c_float(F(r) / F(255.0)), C.c_float(F(g) / F(255.0)), C.c_float(F(b) / F(255.0)), C.byref(oh), C.byref(os_), C.byref(ol))
        assert (F(oh.value), F(os_.value), F(ol.value)) == (h[i], s[i], l[i]), (r, g, b)


def test_sparse_modes_zero_whole_chunks():
    img = CC.band_image(CC.noise(256, 256, 11), 67, 129)
    gh, gs, gl, bands = CC.BAND_SETS["six"]
    dense = CM.hsl_bands(img, gh, gs, gl, bands, sparse=CM.DENSE)
    flat = CM.hsl_bands(img, gh, gs, gl, bands, sparse=CM.FROM_FLAT)
    in_place = CM.hsl_bands(img, gh, gs, gl, bands, sparse=CM.IN_PLACE)
    assert dense[64:128, 0:64, :3].any() and not dense[64:128, 0:64, 3].any()     # the transparent chunk keeps (changed) colours in the dense mode
    assert not flat[64:128, 0:64].any() and np.array_equal(flat[:64], dense[:64]) and np.array_equal(flat[128:], dense[128:]) and np.array_equal(flat[:, 64:], dense[:, 64:])
    assert np.array_equal(in_place, flat)                                           # alpha is untouched: the populated chunks are the same before and after
    assert np.array_equal(dense[..., 3], img[..., 3])


# ---------------------------------------------------------------------------------------------------------------- hand-derived answers
def hue_deg(rgb):
    h, _, _ = CM.rgb_to_hsl(*(np.asarray([v], F) / F(255.0) for v in rgb))
    return float(h[0]) * 360.0


def test_knee_hues_sit_on_the_knees():
    for k in (1, 7, 63, 127):
        for perm, want in (((2 * k, k, 0), 30), ((k, 2 * k, 0), 90), ((0, 2 * k, k), 150), ((0, k, 2 * k), 210), ((k, 0, 2 * k), 270), ((2 * k, 0, k), 330)):
            assert abs(hue_deg(perm) - want) < 1e-3, (perm, hue_deg(perm))
    for k in (1, 9, 63):
        for perm, want in (((4 * k, 3 * k, 0), 45), ((4 * k, k, 0), 15), ((3 * k, 4 * k, 0), 75), ((k, 4 * k, 0), 105), ((4 * k, 0, k), 345), ((4 * k, 0, 3 * k), 315)):
            assert abs(hue_deg(perm) - want) < 1e-3, (perm, hue_deg(perm))
    assert hue_deg((200, 0, 0)) == 0.0 and abs(hue_deg((0, 200, 0)) - 120.0) < 1e-3 and abs(hue_deg((0, 0, 200)) - 240.0) < 1e-3 and hue_deg((77, 77, 77)) == 0.0


def test_band_weight_knees():
    w = lambda deg, c: float(CM.band_weight(np.asarray([deg], F), c)[0])
    assert w(30.0, 0.0) == 1.0 and w(37.5, 0.0) == 0.5 and w(45.0, 0.0) == 0.0 and w(44.0, 0.0) == pytest.approx(1 / 15, abs=1e-6)
    assert w(330.0, 0.0) == 1.0 and w(322.5, 0.0) == 0.5 and w(315.0, 0.0) == 0.0      # around the wheel
    assert w(90.0, 60.0) == 1.0 and w(97.5, 60.0) == 0.5 and w(15.0, 60.0) == 0.0 and w(0.0, 300.0) == 0.0 and w(337.5, 300.0) == 0.5
    assert w(0.0, 180.0) == 0.0 and w(180.0, 180.0) == 1.0


def test_combine_rules_at_the_base_bytes():
    base = np.asarray([[0, 1, 127, 128, 254, 255]], np.uint8)
    want = {0: {"add": [0, 1, 127, 128, 254, 255], "subtract": [0, 1, 127, 128, 254, 255], "intersect": [0, 0, 0, 0, 0, 0]},
            1: {"add": [1, 1, 127, 128, 254, 255], "subtract": [0, 0, 126, 127, 253, 254], "intersect": [0, 0, 0, 0, 0, 1]},
            128: {"add": [128, 128, 128, 128, 254, 255], "subtract": [0, 0, 0, 0, 126, 127], "intersect": [0, 0, 63, 64, 127, 128]},
            255: {"add": [255] * 6, "subtract": [0] * 6, "intersect": [0, 1, 127, 128, 254, 255]}}
    for n, rules in want.items():
        new = np.full_like(base, n)
        assert np.array_equal(CM.combine_masks(new, base, "replace"), new)
        assert np.array_equal(CM.combine_masks(new, None, "add"), new) and not CM.combine_masks(new, None, "subtract").any() and not CM.combine_masks(new, None, "intersect").any()
        for rule, row in rules.items():
            assert CM.combine_masks(new, base, rule).tolist() == [row], (n, rule)


def test_histogram_of_a_2x2_image():
    img = np.asarray([[[10, 20, 30, 255], [10, 20, 30, 0]], [[255, 255, 255, 128], [0, 0, 0, 1]]], np.uint8)
    hist = CM.histogram(img)
    want = np.zeros((4, 256), np.uint32)
    for r, g, b, l in ((10, 20, 30, 19), (255, 255, 255, 255), (0, 0, 0, 0)):      # 2.126 + 14.304 + 2.166 = 18.596 -> 19
        want[0, r] += 1; want[1, g] += 1; want[2, b] += 1; want[3, l] += 1
    assert np.array_equal(hist, want)
    masked = CM.histogram(img, np.asarray([[7, 255], [0, 1]], np.uint8))
    want[0, 255] -= 1; want[1, 255] -= 1; want[2, 255] -= 1; want[3, 255] -= 1
    assert np.array_equal(masked, want)
    # a tie rounds away from zero: 0.2126 * 0 + 0.7152 * 0 + 0.0722 * b is never a tie for a byte, so take the rounding helper itself
    assert CM._round_half_away(np.asarray([0.5, 1.5, 2.5, 254.5, 0.49999997], F)).tolist() == [1.0, 2.0, 3.0, 255.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------- nothing passes vacuously
def test_histogram_cases_skip_pixels_both_ways_and_reach_the_last_luminance_bin():
    for (w, h) in [s for s in CC.SMALL_SHAPES if s[0] * s[1] > 100]:
        img, mask = CC.noise(w, h, 21), CC.selection(w, h, 22)
        img[0, :5, 3] = 0
        assert ((img[..., 3] == 0) & (mask != 0)).any() and ((img[..., 3] != 0) & (mask == 0)).any() and CM.counted(img, mask).any()
    cube = CC.all_colours()
    lum, rounded = CM.luminance_bin(cube)
    # the clamp of :932 is dead code: white gives 255.00002, so no colour rounds above 255; what the cases hold is the bin it would protect, and its neighbours
    assert int(rounded.max()) == 255 and int(lum.min()) == 0 and len(np.unique(lum)) == 256
    assert np.array_equal(cube.reshape(-1, 4)[:, :3].astype(np.uint32) @ np.asarray([1, 256, 65536], np.uint32), np.arange(1 << 24, dtype=np.uint32))


def test_band_cases_hold_fractional_weights_overlaps_and_both_clamp_ends():
    for name, pixels in CC.band_inputs().items():
        for (w, h) in CC.BAND_SHAPES:
            img = CC.band_image(pixels, w, h)
            info = {}
            gh, gs, gl, bands = CC.BAND_SETS["max"]
            CM.hsl_bands(img, gh, gs, gl, bands, info=info)
            wts = np.stack(info["weights"])
            in_bands = (wts > 0).sum(axis=0)
            assert (in_bands >= 1).all() and (in_bands == 1).any() and (in_bands == 2).any(), (name, w, h)   # every hue is within 30 degrees of a centre
            if name != "knee":
                assert ((wts > 0.01) & (wts < 0.99)).any(), (name, w, h)
            else:   # the knee set: hues a rounding error away from where a weight reaches 1 (centre +- 30) and where it reaches 0 (centre +- 45)
                off = np.abs(np.fmod(info["h_deg"], F(60.0))[None, :, :] - np.asarray([15.0, 30.0, 45.0], F)[:, None, None]).min(axis=(1, 2))
                assert (off < 1e-3).all(), (name, w, h, off)
            assert (info["ns_raw"] > 1).any(), (name, w, h)
            CM.hsl_bands(img, *CC.BAND_SETS["min"][:3], CC.BAND_SETS["min"][3], info=info)
            assert (info["ns_raw"] < 0).any(), (name, w, h)
    img = CC.band_image(CC.lattice(), 67, 129)
    assert not img[64:128, 0:64, 3].any() and img[64:128, 0:64, :3].any() and img[:64, :64, 3].any() and (img[:2, :2, 3] == 0).all()


@pytest.fixture(scope="module")
def range_results():
    out = {}
    for name, img in CC.range_inputs().items():
        for s in CC.RANGE_SETS:
            info = {}
            mask, amb = CM.color_range(img, *s, info=info)
            glibc, _ = CM.color_range(img, *s, flavour="glibc")
            out[name, s] = (mask, amb, glibc, info)
    return out


def test_range_cases_hold_every_rejection_both_ends_and_soft_edges(range_results):
    for name in CC.range_inputs():
        seen = {"transparent": False, "unsaturated": False, "outside": False}
        for s in CC.RANGE_SETS:
            mask, _, _, info = range_results[name, s]
            for k in seen:
                seen[k] |= bool(info[k].any())
            assert info["live"].any(), (name, s)
            if s in CC.SOFT_SETS:
                assert len(np.unique(info["new"][info["live"]])) >= 25, (name, s, len(np.unique(info["new"][info["live"]])))
        assert all(seen.values()), (name, seen)
        every = np.concatenate([range_results[name, s][0].reshape(-1) for s in CC.RANGE_SETS])
        live = np.concatenate([range_results[name, s][3]["live"].reshape(-1) for s in CC.RANGE_SETS])
        assert (every[live] == 255).any() and (every[live] == 0).any(), name
    assert len(CC.SOFT_SETS) >= 4


def test_marked_pixels_stay_under_the_libm_cap_and_glibc_agrees_off_them(range_results):
    for (name, s), (mask, amb, glibc, info) in range_results.items():
        assert amb.mean() <= 1e-3, (name, s, int(amb.sum()))          # the project's LIBM-class bar (tests/libm_checks.py), as a cap
        assert np.array_equal(mask[~amb], glibc[~amb]), (name, s)
        assert np.abs(mask.astype(int) - glibc.astype(int)).max() <= 1, (name, s)


def test_exact_powers_are_never_marked():
    img = CC.noise(64, 64, 8)
    for s in ((30.0, 20.0, 0.0, 1.0), (200.0, 90.0, 0.0, 0.5), (90.0, 45.0, 0.0, 0.25)):   # exponents 1, 2, 4
        info = {}
        _, amb = CM.color_range(img, *s, info=info)
        assert float(info["expo"]) in (1.0, 2.0, 4.0)
        if float(info["expo"]) == 1.0:
            assert not amb.any()
    one = np.asarray([[[255, 0, 0, 255], [255, 128, 0, 255]]], np.uint8)   # q = 0 at the centre; q = 1 cannot be forced, 0 can
    mask, amb = CM.color_range(one, 0.0, 20.0, 0.0, 0.3)
    assert mask[0, 0] == 255 and not amb[0, 0]
