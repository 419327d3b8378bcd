"""CPU model of the bucket fill and the magic wand: a numpy restatement of the reference's CPU flavour (src/ui/panels/tools/behavior/raster/fill_magic.rs,
tools/state.rs:574-735), independent of the library.

* the per-pixel colour distance (pixel_color_distance :1048, perceptual_distance :93): every perceptual step is one f32 rounding (numpy float32, the
  reference's association order, no fused operation); `powf` is the host's glibc through ctypes, which is what Rust's f32::powf calls on Linux; `round()` is
  half away from zero;
* the distance map two ways — the reference's 256-bucket Dijkstra (compute_flood_distance_map :950) and a whole-array relaxation to a fixed point.  The map is
  unique, so the two must agree; distance_map() checks that before it returns either (use dijkstra() alone where the agreement was checked elsewhere);
* threshold_alpha :415, merge_magic_wand_masks :486, the cumulative bounding boxes (state.rs:693), build_fill_preview_region :550 over the whole canvas, and the
  commit through the blend oracle the brush-commit tests use."""
import ctypes as C
import ctypes.util

import numpy as np

f32 = np.float32
_m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_m.powf.restype = C.c_float
_m.powf.argtypes = [C.c_float, C.c_float]

LEGACY, PERCEPTUAL = 0, 1
REPLACE, ADD, SUBTRACT, INTERSECT = range(4)


def tolerance_threshold(tolerance) -> int:
    """tolerance_threshold_u8 :78"""
    n = f32(tolerance) / f32(100.0)
    n = f32(0.0) if n < 0 else (f32(1.0) if n > 1 else n)
    v = f32(n * f32(255.0))
    if not v > 0:      # NaN as u8 == 0
        return 0
    t = np.trunc(v)
    if v - t >= f32(0.5):
        t += 1
    return int(min(t, 255))


def _srgb_to_linear_table():
    out = np.empty(256, f32)
    for k in range(256):
        v = f32(k) / f32(255.0)
        out[k] = v / f32(12.92) if v <= f32(0.04045) else f32(_m.powf(float((v + f32(0.055)) / f32(1.055)), 2.4))
    return out


_LIN = _srgb_to_linear_table()


def color_distance(img, target, mode):
    """(h, w) u8: pixel_color_distance of every pixel to `target`"""
    img = np.asarray(img, np.uint8)
    t = [int(v) for v in target]
    both_clear = (img[..., 3] == 0) & (t[3] == 0)
    if mode == LEGACY:
        d = np.abs(img.astype(np.int16) - np.array(t, np.int16)).max(axis=-1).astype(np.uint8)
    else:
        a = img[..., 3].astype(f32) / f32(255.0)
        ta = f32(t[3]) / f32(255.0)
        dr, dg, db = (_LIN[img[..., k]] * a - _LIN[t[k]] * ta for k in range(3))
        dluma = np.abs(f32(0.2126) * dr + f32(0.7152) * dg + f32(0.0722) * db)
        dchroma = np.sqrt(f32(0.5) * (dr - dg) * (dr - dg) + f32(0.5) * (dg - db) * (dg - db) + f32(0.5) * (db - dr) * (db - dr))
        color_term = np.clip(dluma * f32(0.7) + dchroma * f32(0.8), f32(0.0), f32(1.0))
        alpha_term = np.abs(a - ta)
        v = np.maximum(color_term, alpha_term) * f32(255.0)
        assert v.dtype == f32 and dchroma.dtype == f32
        r = np.trunc(v)
        r = r + (v - r >= f32(0.5))
        d = np.clip(r, 0, 255).astype(np.uint8)
    return np.where(both_clear, np.uint8(0), d)


NEIGHBOURS = {4: [(-1, 0), (1, 0), (0, -1), (0, 1)], 8: [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]}


def dijkstra(c, seed, connectivity):
    """compute_flood_distance_map :950 on the per-pixel distances c: the reference's bucket queue"""
    h, w = c.shape
    cost = c.ravel().tolist()
    dist = [255] * (w * h)
    s = seed[1] * w + seed[0]
    dist[s] = cost[s]
    buckets = [[] for _ in range(256)]
    buckets[cost[s]].append(s)
    nb = NEIGHBOURS[connectivity]
    for cur in range(256):
        b = buckets[cur]
        while b:
            i = b.pop()
            if dist[i] != cur:
                continue
            x, y = i % w, i // w
            for dx, dy in nb:
                nx, ny = x + dx, y + dy
                if nx < 0 or ny < 0 or nx >= w or ny >= h:
                    continue
                ni = ny * w + nx
                nc = cost[ni] if cost[ni] > cur else cur
                if nc < dist[ni]:
                    dist[ni] = nc
                    buckets[nc].append(ni)
    return np.array(dist, np.uint8).reshape(h, w)


def relaxation(c, seed, connectivity):
    """the same map as the fixed point of d[p] = min(d[p], max(d[q], c[p])) over all neighbours q at once"""
    h, w = c.shape
    d = np.full((h + 2, w + 2), 255, np.uint8)     # a border of 255 never lowers anything
    d[seed[1] + 1, seed[0] + 1] = c[seed[1], seed[0]]
    inner = d[1:-1, 1:-1]
    while True:
        best = np.full((h, w), 255, np.uint8)
        for dx, dy in NEIGHBOURS[connectivity]:
            np.minimum(best, d[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx], out=best)
        new = np.minimum(inner, np.maximum(best, c))
        if np.array_equal(new, inner):
            return inner.copy()
        inner[...] = new


def distance_map(img, seed, target, mode, connectivity, global_scope, check=True):
    c = color_distance(img, target, mode)
    if global_scope:
        return c
    d = dijkstra(c, seed, connectivity)
    if check:
        assert np.array_equal(d, relaxation(c, seed, connectivity)), "the model's two flood algorithms disagree"
    return d


def threshold_alpha(dist, threshold, anti_aliased):
    d = np.asarray(dist, np.uint8).astype(np.int32)
    out = np.where(d <= threshold, 255, 0)
    if anti_aliased:
        out = np.where((d > threshold) & (d == min(threshold + 1, 255)), 128, out)
    return out.astype(np.uint8)


def wand_mask(dist, threshold, anti_aliased, combine, base=None):
    raw = threshold_alpha(dist, threshold, anti_aliased).astype(np.int32)
    b = np.zeros_like(raw) if base is None else np.asarray(base, np.uint8).astype(np.int32)
    out = {REPLACE: raw, ADD: np.maximum(b, raw), SUBTRACT: np.maximum(b - raw, 0), INTERSECT: b * raw // 255}[combine]
    return out.astype(np.uint8)


def bboxes(dist):
    """the 256 cumulative boxes (x0, y0, x1, y1), -1s where {d <= t} is empty"""
    d = np.asarray(dist, np.uint8)
    out = np.full((256, 4), -1, np.int32)
    cur = None
    for t in range(256):
        ys, xs = np.nonzero(d == t)
        if len(xs):
            box = (xs.min(), ys.min(), xs.max(), ys.max())
            cur = box if cur is None else (min(cur[0], box[0]), min(cur[1], box[1]), max(cur[2], box[2]), max(cur[3], box[3]))
        if cur is not None:
            out[t] = cur
    return out


def fill_preview(dist, threshold, fill, selection=None):
    mask = threshold_alpha(dist, threshold, False)
    active = mask != 0
    if selection is not None:
        active &= np.asarray(selection, np.uint8) > 0
    out = np.zeros(mask.shape + (4,), np.uint8)
    out[active] = (int(fill[0]), int(fill[1]), int(fill[2]), (int(fill[3]) * 255 + 127) // 255)
    return out


def fill_commit(layer, dist, threshold, fill, blend_mode, selection=None):
    """commit_fill_preview_impl :1414-1446: blend_pixel_static(layer, preview, mode, 1.0) where the preview's alpha is > 0"""
    from . import oracle_lib as O
    return O.brush_commit(layer, fill_preview(dist, threshold, fill, selection), blend_mode, None)


def bucket_fill(layer, seed, tolerance, fill, blend_mode, global_fill, selection=None, check=True):
    """perform_flood_fill :1231-1273 and the commit"""
    layer = np.asarray(layer, np.uint8)
    target = layer[seed[1], seed[0]]
    d = distance_map(layer, seed, target, LEGACY, 4, global_fill, check)
    return fill_commit(layer, d, tolerance_threshold(tolerance), fill, blend_mode, selection)
