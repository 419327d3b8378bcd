"""The resampler's window arithmetic restated in numpy, for choosing and checking test shapes: per output sample the first source sample and the tap
count of `image::imageops::resize` as pfx_resize.cpp:build_axis computes them (f32 ratio and centre, floor / ceil, clamps), and from those the widest
source-column range one 64-column output tile reaches (`span_max`), which decides between the fused kernel (8 x span_max float4 in LDS, at most 64 KiB:
span_max <= 512) and the two passes through an f32 intermediate.  No weights here: the oracle is the reference for values."""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
FILTERS = ["nearest", "bilinear", "bicubic", "lanczos3"]
SUPPORT = {"nearest": 0.0, "bilinear": 1.0, "bicubic": 2.0, "lanczos3": 3.0}
TILE_COLS, TILE_ROWS = 64, 8
COPY, FUSED, TWO_PASS = 0, 1, 2   # pfx_int_resize_last(ctx, 0)
LDS_BYTES = 64 * 1024


def build_axis(n_in: int, n_out: int, filter: str):
    """(left, count) per output sample, uint32 arrays of n_out entries"""
    ratio = F(n_in) / F(n_out)
    sratio = ratio if ratio >= F(1) else F(1)
    src_support = F(SUPPORT[filter]) * sratio
    o = np.arange(n_out, dtype=np.uint32).astype(F)
    centre = (o + F(0.5)) * ratio
    left = np.floor(centre - src_support).astype(np.int64)
    left = np.clip(left, 0, n_in - 1)
    right = np.ceil(centre + src_support).astype(np.int64)
    right = np.minimum(np.maximum(right, left + 1), n_in)
    return left.astype(np.uint32), (right - left).astype(np.uint32)


def tile_spans(n_in: int, n_out: int, filter: str):
    """the source-column range of every 64-column output tile: left[first] .. left[last] + count[last]"""
    left, count = build_axis(n_in, n_out, filter)
    spans = []
    for ox0 in range(0, n_out, TILE_COLS):
        last = min(ox0 + TILE_COLS, n_out) - 1
        spans.append(int(left[last]) + int(count[last]) - int(left[ox0]))
    return spans


def span_max(n_in: int, n_out: int, filter: str) -> int:
    return max(tile_spans(n_in, n_out, filter))


def path(w: int, h: int, nw: int, nh: int, filter: str, two_pass: bool = False) -> int:
    if (nw, nh) == (w, h):
        return COPY
    return FUSED if span_max(w, nw, filter) * TILE_ROWS * 16 <= LDS_BYTES and not two_pass else TWO_PASS


def tap_residues(n_in: int, n_out: int, filter: str):
    """the set of tap counts mod 4 over the axis: the fused kernel takes taps four at a time under an `i + k < n` guard"""
    return {int(c) % 4 for c in build_axis(n_in, n_out, filter)[1]}


def find_width_for_span(span: int, n_out: int, filter: str, lo: int = 2, hi: int = 1100):
    """the source widths whose span_max is `span` for n_out output columns"""
    return [w for w in range(lo, hi + 1) if w != n_out and span_max(w, n_out, filter) == span]


# ---------------------------------------------------------------------------------------------------------------------------------- resize cases
@functools.lru_cache(maxsize=None)
def _span_width(span, filter):
    return find_width_for_span(span, TILE_COLS, filter, lo=span - 8, hi=span + 16)[0]


@functools.lru_cache(maxsize=None)
def resize_cases():
    """(name, (w, h), (nw, nh), filters): the shapes of tests/test_gpu_resample_edges.py; tests/test_resize_model_host.py shows what each group reaches"""
    c = []
    for nw in (1, 63, 64, 65, 127, 128, 129):          # output columns around the 64-column tile, down- and upscaled
        c.append((f"width-{nw}", (100, 20), (nw, 12), FILTERS))
    for nh in (1, 7, 8, 9, 15, 16, 17):                # output rows around the 8-row tile
        c.append((f"height-{nh}", (40, 30), (33, nh), FILTERS))
    for (w, h, nw, nh) in RESIDUE_SHAPES:              # tap counts of every residue mod 4 on both axes (not nearest: always one tap)
        c.append((f"taps-{w}x{h}-{nw}x{nh}", (w, h), (nw, nh), FILTERS))
    c.append(("up-1x1", (1, 1), (65, 9), FILTERS))
    c.append(("up-1x9", (1, 9), (64, 17), FILTERS))
    c.append(("up-9x1", (9, 1), (129, 8), FILTERS))
    c.append(("up-2x2", (2, 2), (129, 9), FILTERS))
    c.append(("same-size", (37, 11), (37, 11), FILTERS))
    for f in FILTERS:
        for span in (511, 512, 513):                   # one 64-column tile reaching 511, 512, 513 source columns: fused, fused, two passes
            c.append((f"span-{span}-{f}", (_span_width(span, f), 12), (64, 5), [f]))
        c.append((f"later-tile-{f}", (LATER_TILE_WIDTH[f], 9), (130, 3), [f]))
    c.append(("last-tile-ties", (7, 5), (127, 9), FILTERS))
    return tuple(c)


RESIDUE_SHAPES = [(37, 50, 13, 7), (50, 37, 7, 13), (100, 29, 9, 11), (29, 100, 11, 9), (40, 23, 17, 5), (9, 31, 129, 7)]
# 130 output columns = three tiles; the first reaches at most 512 source columns, the second 513: span_max is a maximum over the tiles, not the first tile's
# span.  (No shape up to 1100 -> 192 columns has a LAST, partial tile that is strictly the widest — fewer columns and the right-hand clamp always make it
# narrower or equal; "last-tile-ties" is the nearest thing: the two tiles of 7 -> 127 columns reach equally far.)
LATER_TILE_WIDTH = {"nearest": 1056, "bilinear": 1023, "bicubic": 992, "lanczos3": 972}


# ---------------------------------------------------------------------------------------------------------------------------------- affine sampling
def affine_inv_scale(scale):
    s = F(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        return F(1) / s if abs(s) > F(1e-6) else F(1)


def affine_identity_matrix(cw, ch):
    """apply_affine's inverse homography without rotation (sin 0 = 0 and cos 0 = 1 exactly), in f32: transform.rs:826-976"""
    f = F(max(cw, ch)) * F(1.5)
    det = f * (f * f)
    inv = F(1) / det
    hi = np.zeros(9, F)
    hi[0] = hi[4] = hi[8] = (f * f) * inv
    return hi


def affine_coords(hi, cw, ch, scale=1.0, offset=(0.0, 0.0)):
    """(src_x, src_y, w) per canvas pixel as apply_affine computes them, f32 operation by operation"""
    hi = np.asarray(hi, F)
    cx, cy = F(cw) * F(0.5), F(ch) * F(0.5)
    inv_scale = affine_inv_scale(scale)
    with np.errstate(all="ignore"):
        v = ((np.arange(ch, dtype=F) - cy - F(offset[1])) * inv_scale)[:, None]
        u = ((np.arange(cw, dtype=F) - cx - F(offset[0])) * inv_scale)[None, :]
        base_sx, base_sy, base_sw = hi[1] * v + hi[2], hi[4] * v + hi[5], hi[7] * v + hi[8]
        w = hi[6] * u + base_sw
        inv_w = F(1) / w
        sx = (hi[0] * u + base_sx) * inv_w + cx
        sy = (hi[3] * u + base_sy) * inv_w + cy
    return sx.astype(F), sy.astype(F), w.astype(F)


AFFINE_SOURCES = [(1, 1), (1, 9), (9, 1), (2, 2), (64, 4), (65, 5)]
AFFINE_CANVASES = [(1, 1), (63, 3), (64, 4), (65, 5), (130, 9)]


def border_targets(n):
    """source coordinates on, and a quarter either side of, -2, -1, 0, n - 2, n - 1, n; and the nearest-neighbour ties at .5 around both ends"""
    t = []
    for b in (-2, -1, 0, n - 2, n - 1, n):
        t += [b - 0.25, float(b), b + 0.25]
    return sorted(set(t + [-1.5, -0.5, 0.5, n - 1.5, n - 0.5, n + 0.5]))


def border_offsets(sw, sh):
    """translations (offset_x, offset_y): canvas pixel (0, 0) samples the source at (tx, ty) — offset = -t — for every border target of either axis"""
    tx, ty = border_targets(sw), border_targets(sh)
    n = max(len(tx), len(ty))
    return [(-tx[k % len(tx)], -ty[(k * 5 + 2) % len(ty)]) for k in range(n)] + [(-tx[k % len(tx)], -ty[k % len(ty)]) for k in range(n)]


# Right angles about x / y: cosf(pi / 2 as f32) = -4.37e-8, the matrix stays invertible and w = hi[6] u + hi[7] v + hi[8] passes through zero at
# v = -hi[8] / hi[7] (u = -hi[8] / hi[6]), a few 1e-6 off the canvas centre.  On an even canvas the centre row / column is a pixel's, and these offsets — the f32
# quotients, worked out with the oracle's matrix for the 64 x 4 canvas — put it on the zero: that row (column) has |w| < 1e-8, every other pixel does not.
W_ZERO_CANVAS = (64, 4)
W_ZERO_CASES = [
    dict(rotation_x=90.0, offset=(0.0, 4.196293502900517e-06)), dict(rotation_x=270.0, offset=(0.0, 1.1447884844528744e-06)),
    dict(rotation_y=90.0, offset=(-4.196293502900517e-06, 0.0)), dict(rotation_y=270.0, offset=(-1.1447884844528744e-06, 0.0)),
    dict(rotation_x=89.9995, offset=(0.0, -0.0008426665444858372)), dict(rotation_y=90.0005, offset=(-0.0008396150078624487, 0.0))]

NAN, INF = float("nan"), float("inf")


def affine_param_cases():
    """keyword arguments of affine_transform beyond the border translations: scales around the |scale| > 1e-6 test, right angles and their neighbours,
    saturating offsets, non-finite parameters one at a time, and the two right angles that make a 1 x 1 canvas's matrix singular"""
    c = [dict(scale=s) for s in (9e-7, 1e-6, 1.1e-6, -1e-6, 1e9, 1e-30, -1.0, 0.5, 3.0)]
    c += [dict(scale=s, offset=(0.25, -0.5)) for s in (9e-7, 1.1e-6, -1e-6)]
    for axis in ("rotation_x", "rotation_y"):
        c += [{axis: a} for a in (90.0, 270.0, 89.9995, 90.0005, 269.9995, 270.0005, 89.0, 60.0)]
    c += [dict(rotation_z=a) for a in (90.0, 180.0, 33.0)] + [dict(rotation_x=90.0, rotation_y=90.0), dict(rotation_z=30.0, rotation_x=40.0, rotation_y=-25.0, scale=1.7)]
    c += W_ZERO_CASES
    for big in (1e9, -1e9, 3e9, -3e9):
        c += [dict(offset=(big, 0.0)), dict(offset=(0.0, big)), dict(offset=(big, big), scale=1e-30)]
    for bad in (NAN, INF, -INF):
        c += [dict(rotation_z=bad), dict(rotation_x=bad), dict(rotation_y=bad), dict(scale=bad), dict(offset=(bad, 0.0)), dict(offset=(0.0, bad))]
    return c
