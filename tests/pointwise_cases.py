"""Inputs and parameter tables for the pointwise adjustment bank's edge tests (k_pointwise.hip / k_pointwise.h): pure Python and numpy, nothing here
touches the GPU or the oracle.  tests/test_pointwise_cases_host.py holds the tables to the conditions that make them worth running (ties, branches, dropped
chunks), tests/test_gpu_pointwise_edges.py runs them on the device against the oracle.

A parameter set is a pair (params, lut): `params` a list of floats, `lut` None or the table the op reads.  Ops are named by an id: the ops::adjustments ops by
their own name, the Rhai-flavour ops with a "rhai_" prefix (split_id)."""
from __future__ import annotations

import numpy as np

ADJUST_OPS = ["invert", "invert_alpha", "sepia", "brightness_contrast", "hsl", "exposure", "highlights_shadows", "temperature_tint", "threshold", "posterize",
              "color_balance", "gradient_map", "black_and_white", "vibrance", "lut_rgba", "desaturate"]
RHAI_OPS = ["invert", "desaturate", "sepia", "sepia_strength", "brightness_contrast", "hsl", "exposure", "levels"]
OP_IDS = ADJUST_OPS + ["rhai_" + o for o in RHAI_OPS]
DENSE, FROM_FLAT, IN_PLACE = 0, 1, 2
NAN, INF = float("nan"), float("inf")


def split_id(op_id):
    """op id -> ("adjust" | "rhai", the op's name)"""
    return ("rhai", op_id[5:]) if op_id.startswith("rhai_") else ("adjust", op_id)


def oracle_rhai_params(op, params):
    """sepia_strength: the reference clamps the script's f64 to 0..1 before the cast to f32 (scripting.rs:923); the library does that itself, the oracle's
    closure starts behind it"""
    if op != "sepia_strength":
        return list(params)
    s = float(params[0])
    s = 0.0 if s < 0.0 else s
    s = 1.0 if s > 1.0 else s
    return [s]


# ------------------------------------------------------------------ images
def colour_cube():
    """4096 x 4096: every RGB colour once, pixel i = (i & 255, (i >> 8) & 255, i >> 16), alpha a multiplicative hash of i (every value, 0.39 % zeros, no 64 x 64
    chunk without alpha: dense and sparse runs agree on it)"""
    i = np.arange(1 << 24, dtype=np.uint64)
    img = np.empty((1 << 24, 4), np.uint8)
    img[:, 0] = i & 255
    img[:, 1] = (i >> 8) & 255
    img[:, 2] = i >> 16
    img[:, 3] = ((i * 2654435761) & 0xFFFFFFFF) >> 24
    return img.reshape(4096, 4096, 4)


LATTICE_VALUES = sorted({0, 1, 2, 127, 128, 129, 253, 254, 255} | set(range(0, 256, 5)))
LATTICE_ALPHAS = (255, 0, 128, 255, 1)


def lattice():
    """every combination of LATTICE_VALUES as (r, g, b), 512 wide (rows of whole 16-byte groups: the kernel's interior path), the last row padded with
    transparent black.  Alpha cycles through LATTICE_ALPHAS: opaque, transparent-but-coloured, half and nearly transparent pixels of every colour family."""
    v = np.asarray(LATTICE_VALUES, np.uint8)
    b, g, r = np.meshgrid(v, v, v, indexing="ij")
    n, w = r.size, 512
    h = (n + w - 1) // w
    img = np.zeros((h * w, 4), np.uint8)
    img[:n, 0], img[:n, 1], img[:n, 2] = r.ravel(), g.ravel(), b.ravel()
    img[:n, 3] = np.asarray(LATTICE_ALPHAS, np.uint8)[np.arange(n) % len(LATTICE_ALPHAS)]
    return img.reshape(h, w, 4)


# shapes by the path pointwise_kernel takes (the interior branch needs no mask, w % 4 == 0 and a whole 64 x 64 chunk; the general path loads and stores
# 16 bytes per row when w % 4 == 0, pixel by pixel otherwise)
INTERIOR_SHAPES = [(64, 64), (128, 64), (192, 128)]
VEC_EDGE_SHAPES = [(68, 64), (64, 65), (132, 70)]
SCALAR_SHAPES = [(197, 141), (63, 64), (1, 1), (3, 130), (130, 1), (5, 3)]
STRIP_SHAPES = [(64 * n, 64) for n in range(1, 18)]   # xcd_swizzle's ragged tail at every residue of the chunk count mod 8
PATH_SHAPES = list(dict.fromkeys(INTERIOR_SHAPES + VEC_EDGE_SHAPES + SCALAR_SHAPES + STRIP_SHAPES))


def n_chunks(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def chunk_boxes(w, h):
    """[(x0, y0, x1, y1)] of the 64 x 64 chunks in the kernel's block order (row-major)"""
    return [(cx, cy, min(cx + 64, w), min(cy + 64, h)) for cy in range(0, h, 64) for cx in range(0, w, 64)]


def path_seeds(shape):
    """the seeds the tests run a shape with.  Three chunks hold all three roles below at once; a shape of exactly two chunks cannot (a chunk is transparent,
    opaque or single-pixel, and the transparent one is always wanted), so it runs twice: seed 0 = (transparent, opaque), seed 1 = (single pixel, transparent)."""
    return (0, 1) if n_chunks(*shape) == 2 else (0,)


def path_image(w, h, seed):
    """random RGBA, 30 % of its pixels transparent but coloured; with two or more chunks: one chunk of zero alpha (colour kept: IN_PLACE skips it, DENSE does
    not), one of alpha 255 everywhere (invert_alpha empties it: FROM_FLAT drops it) and one whose only alpha is the pixel in its last row and last column
    (one lane of one wave keeps the whole chunk alive).  Which chunk plays which role is drawn from the seed; two-chunk shapes: path_seeds."""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((h, w)) < 0.3, 0, np.maximum(img[..., 3], 1))
    boxes = chunk_boxes(w, h)
    if len(boxes) < 2:
        return img
    if len(boxes) == 2:
        roles = {"zero": 0, "full": 1} if seed % 2 == 0 else {"single": 0, "zero": 1}
    else:
        order = rng.permutation(len(boxes))
        roles = {"zero": int(order[0]), "full": int(order[1]), "single": int(order[2])}
    for role, k in roles.items():
        x0, y0, x1, y1 = boxes[k]
        img[y0:y1, x0:x1, 3] = 255 if role == "full" else 0
        if role == "single":
            img[y1 - 1, x1 - 1, 3] = 200
    return img


def path_masks(w, h, seed):
    """selection masks of test_kernel_paths: none, nothing selected, everything selected, random bytes of {0, 1, 128, 255} (any non-zero byte selects)"""
    rng = np.random.default_rng(seed + 31 * w + h)
    return [None, np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), np.asarray([0, 1, 128, 255], np.uint8)[rng.integers(0, 4, (h, w))]]


# ------------------------------------------------------------------ tables
def identity_luts():
    return np.tile(np.arange(256, dtype=np.uint8), (4, 1))


def random_luts(seed=1):
    return np.random.default_rng(seed).integers(0, 256, (4, 256), dtype=np.uint8)


def alpha_to_zero_luts():
    """R, G, B as they are, every alpha to 0: FROM_FLAT drops every chunk, DENSE and IN_PLACE keep the colours"""
    t = identity_luts()
    t[3] = 0
    return t


def random_gradient(seed=2):
    return np.random.default_rng(seed).integers(0, 256, (256, 4), dtype=np.uint8)


def ramp_gradient():
    k = np.arange(256, dtype=np.uint8)
    return np.stack([k, 255 - k, k // 2, np.full(256, 255, np.uint8)], axis=1)


def _s(*params, lut=None):
    return ([float(p) for p in params], lut)


# ------------------------------------------------------------------ every colour: the parameter sets run on colour_cube()
BC_FACTOR_1_5 = 51.47700881958008   # the f32 contrast whose factor 259 (c + 255) / (255 (259 - c)) evaluates to exactly 1.5 in f32
# At most four sets per op, each there for a branch or a rounding tie — but for HSL, whose hue family is seven values by itself (twelve sets), and posterize
# with its five level counts.
ADJUST_PARAMS = {
    "invert": [_s()], "invert_alpha": [_s()], "sepia": [_s()], "desaturate": [_s()],
    # (0, 0): factor 1; (+-100, +-100): both clamps; BC_FACTOR_1_5: factor exactly 1.5, (v - 128) * 1.5 + 128 ties on every odd v
    "brightness_contrast": [_s(0, 0), _s(100, 100), _s(-100, -100), _s(0, BC_FACTOR_1_5)],
    # hue 0 / 60 / 120 / +-180 / +-360 at saturation 0 (first: colours exactly on hue_seg's boundaries); saturation -100 = hsl_to_rgb's grey branch, +100;
    # lightness +-100; a generic triple
    "hsl": [_s(0, 0, 0), _s(60, 0, 0), _s(120, 0, 0), _s(180, 0, 0), _s(-180, 0, 0), _s(360, 0, 0), _s(-360, 0, 0), _s(0, -100, 0), _s(0, 100, 0),
            _s(0, 0, 100), _s(0, 0, -100), _s(47, 35, -12)],
    "exposure": [_s(-1.0), _s(1.0), _s(0.5), _s(-2.3)],                       # -1: gain 0.5, every odd byte on an exact .5
    "highlights_shadows": [_s(100, -100), _s(-100, 100), _s(30, -20)],
    "temperature_tint": [_s(0, 1.0), _s(100, 100), _s(-100, -100), _s(100, -100)],   # tint 1: g - 0.5
    "threshold": [_s(0), _s(127.5), _s(255), _s(255.5)],
    "posterize": [_s(2), _s(3), _s(4), _s(255), _s(256)],
    "color_balance": [_s(*[100] * 9), _s(*[-100] * 9), _s(100, -100, 50, -30, 20, 100, -100, 70, -5)],
    "gradient_map": [_s(lut=random_gradient()), _s(lut=ramp_gradient())],
    "black_and_white": [_s(30, 59, 11), _s(100, 100, 100), _s(-40, 120, -10), _s(-30, -59, -11)],
    "vibrance": [_s(100), _s(-100), _s(0), _s(50)],
    "lut_rgba": [_s(lut=identity_luts()), _s(lut=random_luts()), _s(lut=alpha_to_zero_luts())],
}
RHAI_PARAMS = {
    "invert": [_s()], "desaturate": [_s()], "sepia": [_s()],
    "sepia_strength": [_s(0), _s(0.4), _s(1), _s(7)],
    "brightness_contrast": [_s(0, 0), _s(100, 100), _s(-100, -100), _s(0.5, BC_FACTOR_1_5)],
    "hsl": [_s(0, 0, 0), _s(60, -100, 0), _s(-180, 100, 0), _s(47, 35, -12)],
    "exposure": [_s(-1.0), _s(1.0), _s(0.8)],
    "levels": [_s(0, 255, 1), _s(20, 230, 0.8), _s(10, 240, 2.2), _s(200, 50, 1.3)],   # identity, gamma != 1 both ways, in_black > in_white
}


def every_colour_sets(op_id):
    kind, op = split_id(op_id)
    return (ADJUST_PARAMS if kind == "adjust" else RHAI_PARAMS)[op]


# the sets whose unrounded result sits on k + 0.5 for many colours: (op id, index of the set)
TIE_SETS = [("exposure", 0), ("temperature_tint", 0), ("brightness_contrast", 3)]

# ------------------------------------------------------------------ parameter edges: the sets run on lattice()
EDGE_VALUES = [0.0, -0.0, NAN, INF, -INF, 3e36, -3e36, 1e38, -1e38]   # 3e36 stays finite through the host's folding, 1e38 overflows it where it multiplies


def _each_parameter(base, extra=()):
    """every EDGE_VALUES entry in every position of `base`, the other positions as in `base`; then `extra`"""
    sets = []
    for k in range(len(base)):
        for v in EDGE_VALUES:
            p = list(base)
            p[k] = v
            sets.append(_s(*p))
    return sets + [_s(*p) for p in extra]


EDGE_PARAMS = {
    # contrast 259: the factor's denominator is zero (inf); -255: its numerator is zero
    "brightness_contrast": _each_parameter([10, 20], [(0, 259), (10, 259), (0, -255), (10, -255), (128, 259), (0, 258.99), (0, 260)]),
    "hsl": _each_parameter([30, -20, 10], [(NAN, NAN, NAN), (INF, INF, INF), (720, 1e30, -1e30), (0, 0, 3e38)]),
    "exposure": _each_parameter([0.5], [(200,), (-200,), (127,), (128,), (-149,), (-150,)]),
    "highlights_shadows": _each_parameter([30, -20]),
    "temperature_tint": _each_parameter([30, 10]),
    "threshold": _each_parameter([128]),
    "posterize": _each_parameter([4], [(0,), (1,), (1.5,), (1e30,), (2,)]),
    "color_balance": _each_parameter([10, 0, -10, 5, -5, 2, -10, 0, 10]),
    "black_and_white": _each_parameter([30, 59, 11], [(1e38, 1e38, 1e38), (-1e38, -1e38, -1e38), (1e38, -1e38, 0)]),
    "vibrance": _each_parameter([50]),
    "rhai_sepia_strength": _each_parameter([0.4]),
    "rhai_brightness_contrast": _each_parameter([10, 20], [(0, 259), (0, -255)]),
    "rhai_hsl": _each_parameter([30, -20, 10]),
    "rhai_exposure": _each_parameter([0.5], [(200,), (-200,)]),
    "rhai_levels": _each_parameter([20, 230, 0.8]),
}


def non_finite_set(params):
    return not all(np.isfinite(params))
