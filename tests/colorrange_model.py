"""CPU model of the colour dialogs' last pixel loops (reference: src/ops/adjustments.rs — compute_histogram :883-937, hue_saturation_per_band_from_flat
:1594-1674, select_color_range :1684-1792, with rgb_to_hsl / hsl_to_rgb / hue_to_rgb :944-1012 and apply_pixel_transform_from_flat :46-108), the yardstick of
tests/test_gpu_colorrange.py: no golden of the reference covers these functions.  A restatement with line citations, in np.float32 throughout: every array
operation below rounds once per element like the reference's scalar f32 expression, and nothing passes through f64 but the exact rounding helper and the
colour range's power.

The power: the reference calls f32::powf (glibc's powf on Linux, 0.82 ulp by its own claim), the device the f64 pow rounded once to f32.  `color_range` takes the
f64 route and marks a pixel *ambiguous* when moving the rounded power by one f32 ulp either way changes the output byte — unless the f64 power is itself an f32
value, which every libm within 1 ulp returns exactly.  tests/test_colorrange_model_host.py holds the marks to the 0.1 % cap and the model to glibc's powf off them."""
import ctypes
import ctypes.util
import math

import numpy as np

F = np.float32
DENSE, FROM_FLAT, IN_PLACE = 0, 1, 2
COMBINE = ("replace", "add", "subtract", "intersect")
BAND_CENTERS = (0.0, 60.0, 120.0, 180.0, 240.0, 300.0)   # :1616
EPS = F(1e-6)


def _round_half_away(v):
    """f32::round as a float64 array: |v| + 0.5 is exact in f64 for every finite f32"""
    v = np.asarray(v, F).astype(np.float64)
    return np.copysign(np.floor(np.abs(v) + 0.5), v)


def _round_u8(v):
    """`.round().clamp(0.0, 255.0) as u8`"""
    return np.clip(_round_half_away(v), 0, 255).astype(np.uint8)


def _clamp(v, lo, hi):
    """f32::clamp for values that are never NaN"""
    return np.minimum(np.maximum(v, F(lo)), F(hi)).astype(F)


def _unit(img):
    """the three colour channels as f32 k / 255.0"""
    return tuple(np.asarray(img[..., k], np.uint8).astype(F) / F(255.0) for k in range(3))


# ---------------------------------------------------------------------------------------------------------------- :944-1012
def rgb_to_hsl(r, g, b):
    mx = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    l = (mx + mn) / F(2.0)
    gray = np.abs(mx - mn) < EPS                                                  # :949
    d = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(l > F(0.5), d / (F(2.0) - mx - mn), d / (mx + mn))           # :954-958
        hr = (g - b) / d                                                          # :961
        hr = np.where(hr < 0, hr + F(6.0), hr) / F(6.0)
        hg = ((b - r) / d + F(2.0)) / F(6.0)                                      # :967
        hb = ((r - g) / d + F(4.0)) / F(6.0)                                      # :969
    h = np.where(np.abs(mx - r) < EPS, hr, np.where(np.abs(mx - g) < EPS, hg, hb))
    zero = np.zeros_like(l)
    return np.where(gray, zero, h).astype(F), np.where(gray, zero, s).astype(F), l.astype(F)


def hue_to_rgb(p, q, t):
    t = np.where(t < 0, t + F(1.0), t)                                            # :996
    t = np.where(t > F(1.0), t - F(1.0), t)                                       # :999
    up = p + (q - p) * F(6.0) * t                                                 # :1003
    down = p + (q - p) * (F(2.0) / F(3.0) - t) * F(6.0)                           # :1009
    return np.where(t < F(1.0) / F(6.0), up, np.where(t < F(1.0) / F(2.0), q, np.where(t < F(2.0) / F(3.0), down, p))).astype(F)


def hsl_to_rgb(h, s, l):
    q = np.where(l < F(0.5), l * (F(1.0) + s), l + s - l * s)                     # :981-985
    p = F(2.0) * l - q
    third = F(1.0) / F(3.0)
    gray = np.abs(s) < EPS                                                        # :977
    return tuple(np.where(gray, l, hue_to_rgb(p, q, t)).astype(F) for t in (h + third, h, h - third))


# ---------------------------------------------------------------------------------------------------------------- histogram
def luminance_bin(img):
    """min(round(0.2126 r + 0.7152 g + 0.0722 b), 255) per pixel, and the unclamped rounded value (:928-932)"""
    r, g, b = (img[..., k].astype(F) for k in range(3))
    lum = F(0.2126) * r + F(0.7152) * g + F(0.0722) * b
    rounded = _round_half_away(lum).astype(np.int64)
    return np.minimum(rounded, 255), rounded


def counted(img, mask=None):
    """the pixels compute_histogram counts: selected (:913-919) and not fully transparent (:925)"""
    keep = img[..., 3] != 0
    return keep if mask is None else keep & (np.asarray(mask) != 0)


def histogram(img, mask=None):
    """(4, 256) uint32: R, G, B, luminance"""
    img = np.asarray(img, np.uint8)
    keep = counted(img, mask)
    lum, _ = luminance_bin(img)
    rows = [np.bincount(v[keep].astype(np.int64), minlength=256) for v in (img[..., 0], img[..., 1], img[..., 2], lum)]
    return np.asarray(rows, np.uint32)


# ---------------------------------------------------------------------------------------------------------------- per-band Hue/Saturation
def band_weight(h_deg, centre):
    """:1620-1632"""
    dist = np.fmod(np.abs(h_deg - F(centre)), F(360.0))
    dist = np.where(dist > F(180.0), F(360.0) - dist, dist)
    return np.where(dist <= F(30.0), F(1.0), np.where(dist < F(45.0), F(1.0) - (dist - F(30.0)) / F(15.0), F(0.0))).astype(F)


def chunk_alpha_any(alpha):
    """per pixel: does its 64 x 64 chunk hold a non-zero alpha"""
    h, w = alpha.shape
    out = np.zeros((h, w), bool)
    for y in range(0, h, 64):
        for x in range(0, w, 64):
            out[y:y + 64, x:x + 64] = alpha[y:y + 64, x:x + 64].any()
    return out


def hsl_bands(img, global_hue=0.0, global_sat=0.0, global_light=0.0, bands=(), mask=None, sparse=FROM_FLAT, info=None):
    """hue_saturation_per_band_from_flat :1635-1674 inside apply_pixel_transform_from_flat :46-108.  bands: up to six (hue, saturation, lightness); info (a
    dict) receives `weights` (6 arrays), `ns_raw` (s * factor before the clamp) and `s`"""
    img = np.asarray(img, np.uint8)
    bands = list(bands) + [(0.0, 0.0, 0.0)] * (6 - len(bands))
    g_sat = F(1.0) + F(global_sat) / F(100.0)                                     # :1644
    g_light = F(global_light) * F(255.0) / F(100.0)                               # :1645
    h, s, l = rgb_to_hsl(*_unit(img))
    h_deg = h * F(360.0)
    extra_hue = np.full(h.shape, F(global_hue), F)
    factor = np.full(h.shape, g_sat, F)
    extra_light = np.full(h.shape, g_light, F)
    weights = []
    for (bh, bs, bl), centre in zip(bands, BAND_CENTERS):
        wgt = band_weight(h_deg, centre)
        on = wgt > 0                                                              # :1657
        extra_hue = np.where(on, extra_hue + F(bh) * wgt, extra_hue).astype(F)
        factor = np.where(on, factor + F(bs) / F(100.0) * wgt, factor).astype(F)
        extra_light = np.where(on, extra_light + F(bl) * F(255.0) / F(100.0) * wgt, extra_light).astype(F)
        weights.append(wgt)
    one = F(1.0)
    nh = np.fmod(np.fmod(h + extra_hue / F(360.0), one) + one, one).astype(F)      # :1664, Rust's % is fmod
    ns_raw = (s * factor).astype(F)
    ns = _clamp(ns_raw, 0.0, 1.0)
    rgb = hsl_to_rgb(nh, ns, l)
    out = img.copy()
    for k in range(3):
        out[..., k] = _round_u8(rgb[k] * F(255.0) + extra_light)                  # :1668, :97-99; alpha: round(a) = a
    if mask is not None:
        keep = np.asarray(mask) == 0                                              # :84-90
        out[keep] = img[keep]
    if sparse == IN_PLACE:      # apply_pixel_transform :21-42: only populated chunks are visited
        out[~chunk_alpha_any(img[..., 3])] = 0
    elif sparse == FROM_FLAT:   # :105, TiledImage::from_rgba_image drops a chunk whose alpha is all zero
        out[~chunk_alpha_any(out[..., 3])] = 0
    if info is not None:
        info.update(weights=weights, ns_raw=ns_raw, s=s, h_deg=h_deg)
    return out


# ---------------------------------------------------------------------------------------------------------------- colour range
def _per_unique(values, fn, dtype):
    """fn over the distinct values only (a scalar libm call each), scattered back"""
    u, inv = np.unique(values, return_inverse=True)
    return np.asarray([fn(v) for v in u], dtype)[inv.reshape(values.shape)]


def pow_f64(q, expo):
    """C's pow(f64(q), f64(expo)) (math.pow is the platform's libm), as float64"""
    e = float(expo)
    return _per_unique(np.asarray(q, F), lambda v: math.pow(float(v), e), np.float64)


_libm = None


def powf_glibc(q, expo):
    """the reference's flavour: the platform libm's powf, as float32"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.powf.restype = ctypes.c_float
        _libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    e = float(expo)
    return _per_unique(np.asarray(q, F), lambda v: _libm.powf(float(v), e), F)


def range_prepare(hue_center_deg, hue_tolerance_deg, sat_min, fuzziness):
    """:1705-1707 and the exponent of :1734 as f32 scalars"""
    hue_center = F(hue_center_deg) / F(360.0)
    hue_tol = np.maximum(F(hue_tolerance_deg) / F(360.0), F(0.001))
    fuzz = _clamp(F(fuzziness), 0.001, 1.0)
    expo = F(1.0) / np.maximum(fuzz, F(0.01))
    return hue_center, hue_tol, F(sat_min), F(expo)


def _range_byte(p):
    """the byte of a power: `(weight * 255.0).clamp(0.0, 255.0) as u8`"""
    weight = F(1.0) - np.asarray(p, F)
    return np.trunc(_clamp(weight * F(255.0), 0.0, 255.0)).astype(np.uint8)


def combine_masks(new, base, combine):
    """:1742-1787, select_color_range's own rule; base None = all zero"""
    mode = COMBINE.index(combine) if isinstance(combine, str) else int(combine)
    new = np.asarray(new, np.uint8)
    base = np.zeros_like(new) if base is None else np.asarray(base, np.uint8)
    if mode == 0:
        return new.copy()
    if mode == 1:
        return np.maximum(new, base)
    if mode == 2:
        return (base.astype(np.int16) - np.minimum(new, base).astype(np.int16)).astype(np.uint8)
    return (new.astype(np.uint16) * base.astype(np.uint16) // 255).astype(np.uint8)


def color_range(img, hue_center_deg, hue_tolerance_deg, sat_min, fuzziness, combine="replace", base=None, flavour="f64", info=None):
    """select_color_range :1705-1787: (mask, ambiguous).  flavour "f64": pow in f64 rounded once (the device's); "glibc": powf.  ambiguous marks the pixels
    whose new-mask byte moves when the power moves by one f32 ulp (see the module text); info receives the rejection maps and the new mask"""
    img = np.asarray(img, np.uint8)
    hue_center, hue_tol, smin, expo = range_prepare(hue_center_deg, hue_tolerance_deg, sat_min, fuzziness)
    h, s, _ = rgb_to_hsl(*_unit(img))
    transparent = img[..., 3] == 0                                                # :1713
    unsaturated = ~transparent & (s < smin)                                       # :1721
    diff = np.abs(h - hue_center)
    diff = np.where(diff > F(0.5), F(1.0) - diff, diff).astype(F)                 # :1726
    outside = ~transparent & ~unsaturated & (diff > hue_tol)                      # :1730
    live = ~(transparent | unsaturated | outside)
    q = np.where(live, diff / hue_tol, F(0.0)).astype(F)
    ambiguous = np.zeros(live.shape, bool)
    if flavour == "glibc":
        p = powf_glibc(q, expo)
    else:
        p64 = pow_f64(q, expo)
        p = p64.astype(F)
        byte = _range_byte(p)
        moved = (_range_byte(np.nextafter(p, F(np.inf))) != byte) | (_range_byte(np.nextafter(p, F(-np.inf))) != byte)
        ambiguous = live & moved & (p.astype(np.float64) != p64)
    new = np.where(live, _range_byte(p), 0).astype(np.uint8)
    if info is not None:
        info.update(transparent=transparent, unsaturated=unsaturated, outside=outside, live=live, new=new, q=q, expo=expo)
    return combine_masks(new, base, combine), ambiguous
