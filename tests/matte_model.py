"""CPU model of background removal around the model (ref: src/ops/ai.rs: preprocess_image :731, is_probability_space :675, to_probability :693,
mask_confidence_score :706, ModelProfile :621-669, the output selection :1356-1380, postprocess_mask :766, apply_mask_expansion :850, morphological_close :904,
blur_grayscale :913), restated in numpy: float32 arrays, one rounding per operation.  expf is the oracle's device flavour (glibc's algorithm restated, host-
independent; tests/test_matte_model_host.py holds it to the host's expf on every positive argument); the Lanczos3 resize is the oracle's RGBA resize — of the
replicated grey for the one-channel matte, since the crate treats channels independently.  tests/test_matte_model_host.py holds this model to a pixel-loop
transcription that hoists nothing and to hand-derived answers."""
from dataclasses import dataclass

import numpy as np

from . import oracle_lib as O

F = np.float32
MEAN = (F(0.485), F(0.456), F(0.406))
STD = (F(0.229), F(0.224), F(0.225))
F32_MAX = np.finfo(np.float32).max


@dataclass(frozen=True)
class Settings:   # RemoveBgSettings :19-37
    threshold: float = 0.5
    edge_feather: float = 0.0
    mask_expansion: int = 0
    smooth_edges: bool = True
    fill_holes: int = 0


def expf(x):
    """f32::exp per element: the device flavour of the oracle's expf, evaluated once per distinct argument"""
    x = np.asarray(x, np.float32)
    uniq, inverse = np.unique(x.ravel().view(np.uint32), return_inverse=True)
    with O.libm_flavour("device"):
        vals = O.libm_eval("exp", uniq.view(np.float32))
    return vals[inverse].reshape(x.shape)


def tensor(img, size):
    """preprocess_image: (3, size, size) float32"""
    img = np.ascontiguousarray(img, np.uint8)
    scaled = O.resize(img, size, size, "lanczos3")   # the same size: a copy, as imageops::resize does
    out = np.empty((3, size, size), np.float32)
    for c in range(3):
        out[c] = (scaled[..., c].astype(np.float32) / F(255.0) - MEAN[c]) / STD[c]
    return out


def sample_step(n):
    return max(n // 10000, 1)


def is_probability_space(values):
    v = np.asarray(values, np.float32).ravel()
    if v.size == 0:
        return False
    s = v[::sample_step(v.size)]
    s = s[~np.isnan(s)]   # f32::min / max return the other operand for a NaN
    mn = min(F(F32_MAX), s.min()) if s.size else F(F32_MAX)
    mx = max(F(-F32_MAX), s.max()) if s.size else F(-F32_MAX)
    return bool(mn >= F(-0.05) and mx <= F(1.05))


def to_probability(values, is_prob):
    v = np.asarray(values, np.float32)
    with np.errstate(all="ignore"):
        if is_prob:
            return np.where(np.isnan(v), v, np.clip(v, F(0.0), F(1.0))).astype(np.float32)   # f32::clamp keeps a NaN
        return (F(1.0) / (F(1.0) + expf(-v))).astype(np.float32)


def confidence(values):
    """mask_confidence_score: (is_probability, score)"""
    v = np.asarray(values, np.float32).ravel()
    if v.size == 0:
        return False, 0.0
    is_prob = is_probability_space(v)
    q = to_probability(v, is_prob).astype(np.float64)
    with np.errstate(invalid="ignore"):
        decisive = ~((q >= 0.1) & (q <= 0.9))   # a NaN is outside the range
    return is_prob, int(decisive.sum()) / v.size


def pick_output(input_w, input_h, confidences):
    """the selection :1356-1380 with ModelProfile::detect; a negative confidence is an output that could not be read.  None: no usable output"""
    n = len(confidences)
    preferred = n - 1 if (input_w == 1024 and input_h == 1024 and n >= 5) else 0
    usable = [i for i in range(n) if confidences[i] >= 0.0]
    if not usable:
        return None
    best = max([0.0] + [confidences[i] for i in usable])
    close = [i for i in usable if confidences[i] >= best - 0.01]
    if preferred in close:
        return preferred
    pick = close[0]
    for i in close:   # max_by keeps the last of equal maxima
        if confidences[i] >= confidences[pick]:
            pick = i
    return pick


def byte(values, is_prob, threshold, smooth_edges):
    """to_probability + postprocess_mask's first step: (prob_h, prob_w) uint8"""
    p = to_probability(values, is_prob)
    t = F(threshold)
    with np.errstate(all="ignore"):
        if smooth_edges:
            r = F(1.0) / (F(1.0) + expf((-(p - t)) * F(12.0)))
            scaled = r * F(255.0)
            return np.where(np.isnan(scaled), F(0.0), np.clip(scaled, F(0.0), F(255.0))).astype(np.uint8)   # `as u8`: truncation, NaN -> 0
        return np.where(p >= t, 255, 0).astype(np.uint8)


def expand(grey, expansion):
    """apply_mask_expansion: |expansion| iterations, each reading the previous image whole"""
    cur = np.ascontiguousarray(grey, np.uint8).copy()
    h, w = cur.shape
    dilate = expansion > 0
    for _ in range(abs(int(expansion))):
        pad = np.pad(cur, 1, constant_values=0 if dilate else 255)   # cells outside the image never act as neighbours
        windows = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
        if dilate:
            cur = np.where(cur < 128, windows.max(axis=0), cur)
        else:
            cur = np.where(cur > 128, windows.min(axis=0), cur)
    return cur


def close(grey, radius):
    return expand(expand(grey, int(radius)), -int(radius))


def resize(grey, w, h):
    """imageops::resize(GrayImage, w, h, Lanczos3): channel 0 of the RGBA resize of the replicated grey; the caller skips it at equal sizes (:816)"""
    g = np.ascontiguousarray(grey, np.uint8)
    if g.shape == (h, w):
        return g.copy()
    rgba = np.ascontiguousarray(np.repeat(g[..., None], 4, axis=2))
    return np.ascontiguousarray(O.resize(rgba, w, h, "lanczos3")[..., 0])


def feather_radius(edge_feather):
    """0 = postprocess_mask skips the blur (:828); else blur_grayscale's r (:915)"""
    if not F(edge_feather) > F(0.5):
        return 0
    return max(int(np.ceil(F(edge_feather))), 1)


def box_pass(g, r, axis):
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(g.astype(np.int64), pad, mode="edge")
    c = np.concatenate([np.zeros_like(np.take(p, [0], axis=axis)), np.cumsum(p, axis=axis)], axis=axis)
    n = g.shape[axis]
    sums = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis) - np.take(c, np.arange(n), axis=axis)
    return (sums.astype(np.float32) / F(2 * r + 1)).astype(np.uint8)   # the f32 sum of integers below 2^24 is exact; `as u8` truncates


def feather(grey, edge_feather):
    g = np.ascontiguousarray(grey, np.uint8)
    r = feather_radius(edge_feather)
    if r == 0:
        return g.copy()
    return box_pass(box_pass(g, r, 1), r, 0)


def apply(img, matte):
    out = np.ascontiguousarray(img, np.uint8).copy()
    a = out[..., 3].astype(np.float32) / F(255.0)
    m = np.asarray(matte, np.uint8).astype(np.float32) / F(255.0)
    out[..., 3] = np.clip(a * m * F(255.0), F(0.0), F(255.0)).astype(np.uint8)
    return out


def postprocess(values, img, s: Settings, is_probability=-1):
    """:1402-1445: (result image, final matte)"""
    v = np.asarray(values, np.float32)
    h, w = img.shape[:2]
    is_prob = is_probability_space(v) if is_probability < 0 else bool(is_probability)
    g = byte(v, is_prob, s.threshold, s.smooth_edges)
    if s.mask_expansion != 0:
        g = expand(g, s.mask_expansion)
    if s.fill_holes > 0:
        g = close(g, s.fill_holes)
    g = resize(g, w, h)
    if feather_radius(s.edge_feather):
        g = feather(g, s.edge_feather)
    return apply(img, g), g
