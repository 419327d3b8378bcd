"""The floating selection restated in numpy, from src/ops/clipboard.rs alone: extract_to_overlay :729, transformed_bounds :939, rasterize_for_clipboard :1048,
render_replacement_preview :1144 (apply_transformed_pixels_to_image :1167), corners_canvas :1313, commit :2032, render_preview :2168, sample_bilinear :2326,
alpha_blend :2368.

float32 arrays, one numpy operation per reference operation (numpy never contracts), round() half away from zero, `as u32` / `as i32` saturating and truncating,
cosf / sinf of the rotation from glibc through ctypes (what the reference's f32::cos resolves to; tests/shape_model.py does the same).  The scale step is
tests/oracle_lib.resize — `imageops::resize` — and the one-byte overwrite mask goes through it replicated to four channels with "nearest".

An overlay is a dict: source_w, source_h, doc_w, doc_h, center (x, y), rotation, scale (x, y), anchor (x, y), interpolation (a name of FILTERS), anti_aliasing,
overwrite_transparent.  commit / rasterize also return how many pixels took which branch, for tests/test_overlay_model_host.py's non-vacuity conditions."""
import numpy as np

from . import oracle_lib as O
from . import select_model as SM
from .shape_model import cosf, sinf

F = np.float32
FILTERS = ["nearest", "bilinear", "bicubic", "lanczos3"]   # PFX_RESIZE_*; Interpolation::to_filter, transform.rs:29-58
F32_MAX = F(3.4028234663852886e38)


def overlay(source_w, source_h, doc_w, doc_h, center, rotation=0.0, scale=(1.0, 1.0), anchor=(0.0, 0.0), interpolation="bilinear", anti_aliasing=True,
            overwrite_transparent=False):
    """PasteOverlay::new's defaults :893"""
    return dict(source_w=source_w, source_h=source_h, doc_w=doc_w, doc_h=doc_h, center=center, rotation=rotation, scale=scale, anchor=anchor,
                interpolation=interpolation, anti_aliasing=anti_aliasing, overwrite_transparent=overwrite_transparent)


def as_u32(v) -> int:
    v = F(v)
    if np.isnan(v) or v <= 0:
        return 0
    return 0xffffffff if v >= F(4294967296.0) else int(v)


def as_i32(v) -> int:
    v = F(v)
    if np.isnan(v):
        return 0
    return -2 ** 31 if v <= F(-2147483648.0) else (2 ** 31 - 1 if v >= F(2147483648.0) else int(v))


def round_away(v):
    """f32::round, scalar or array, either sign"""
    v = np.asarray(v, F)
    a = np.abs(v)
    fl = np.floor(a)
    return np.copysign(fl + (a - fl >= F(0.5)).astype(F), v).astype(F)


def _round_u8(v):
    """`v.round().clamp(0.0, 255.0) as u8` on the non-negative values it meets: floor(x) + (x - floor(x) >= 0.5)"""
    fl = np.floor(v)
    return np.clip(fl + (v - fl >= F(0.5)), 0, 255).astype(np.uint8)


def _fold(corners, min_x, min_y, max_x, max_y):
    for cx, cy in corners:
        min_x, min_y, max_x, max_y = min(min_x, cx), min(min_y, cy), max(max_x, cx), max(max_y, cy)   # finite values: f32::min / max are plain
    return F(min_x), F(min_y), F(max_x), F(max_y)


def geometry(ov):
    sw_f, sh_f = F(ov["source_w"]), F(ov["source_h"])
    cx, cy, sx, sy = F(ov["center"][0]), F(ov["center"][1]), F(ov["scale"][0]), F(ov["scale"][1])
    ax, ay = cx + F(ov["anchor"][0]), cy + F(ov["anchor"][1])                        # anchor_canvas :1292
    cw, ch = F(ov["doc_w"]), F(ov["doc_h"])
    g = {}
    with np.errstate(all="ignore"):
        g["scaled_w"] = as_u32(max(round_away(sw_f * sx), F(1.0)))                   # :2046
        g["scaled_h"] = as_u32(max(round_away(sh_f * sy), F(1.0)))
        g["cos"], g["sin"] = cosf(F(ov["rotation"])), sinf(F(ov["rotation"]))
        hx, hy = sw_f * sx / F(2.0), sh_f * sy / F(2.0)                              # scaled_half :1269
        corners = []
        for px, py in ((cx - hx, cy - hy), (cx + hx, cy - hy), (cx - hx, cy + hy), (cx + hx, cy + hy)):   # :1316-1319
            dx, dy = px - ax, py - ay                                                # rotate_point :1300
            corners.append((F(ax + dx * g["cos"] - dy * g["sin"]), F(ay + dx * g["sin"] + dy * g["cos"])))
        g["corners"] = corners
        min_x, min_y, max_x, max_y = _fold(corners, cw, ch, F(0.0), F(0.0))          # :2056-2065
        g["row_start"] = as_u32(max(np.floor(min_y), F(0.0)))
        g["row_end"] = as_u32(min(np.ceil(max_y), ch - F(1.0)))
        g["col_start"] = as_u32(max(np.floor(min_x), F(0.0)))
        g["col_end"] = as_u32(min(np.ceil(max_x), cw - F(1.0)))
        x0, y0 = as_u32(min(max(np.floor(min_x), F(0.0)), cw)), as_u32(min(max(np.floor(min_y), F(0.0)), ch))   # :954-958
        x1, y1 = as_u32(min(max(np.ceil(max_x), F(0.0)), cw)), as_u32(min(max(np.ceil(max_y), F(0.0)), ch))
        g["bounds"] = (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None
        min_x, min_y, max_x, max_y = _fold(corners, F32_MAX, F32_MAX, -F32_MAX, -F32_MAX)   # :1061-1070
        col_start, row_start, col_end, row_end = as_i32(np.floor(min_x)), as_i32(np.floor(min_y)), as_i32(np.ceil(max_x)), as_i32(np.ceil(max_y))
        g["raster"] = None if col_end < col_start or row_end < row_start else (col_start, row_start, col_end - col_start + 1, row_end - row_start + 1)
    g["anchor"] = (ax, ay)
    g["origin"] = (cx - F(g["scaled_w"]) / F(2.0), cy - F(g["scaled_h"]) / F(2.0))   # :2074
    return g


def scale_source(ov, g, source, filter_name=None):
    return O.resize(np.ascontiguousarray(source, np.uint8), g["scaled_w"], g["scaled_h"], filter_name or ov["interpolation"])


def scale_mask(g, mask):
    four = np.repeat(np.ascontiguousarray(mask, np.uint8)[..., None], 4, axis=2)
    return O.resize(four, g["scaled_w"], g["scaled_h"], "nearest")[..., 0].copy()


def sample_bilinear(img, x, y):
    """:2326 on arrays of coordinates; clamp to edge"""
    h, w = img.shape[:2]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    at = lambda sx, sy: img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(F)
    p00, p10, p01, p11 = at(xi, yi), at(xi + 1, yi), at(xi, yi + 1), at(xi + 1, yi + 1)
    inv_fx, inv_fy = F(1.0) - fx, F(1.0) - fy
    w00, w10, w01, w11 = (inv_fx * inv_fy)[..., None], (fx * inv_fy)[..., None], (inv_fx * fy)[..., None], (fx * fy)[..., None]
    return _round_u8(p00 * w00 + p10 * w10 + p01 * w01 + p11 * w11)


def alpha_blend(dst, src):
    """:2368 on (..., 4) uint8 arrays"""
    dst, src = np.asarray(dst, np.uint8), np.asarray(src, np.uint8)
    sa, da = src[..., 3].astype(F) / F(255.0), dst[..., 3].astype(F) / F(255.0)
    rest = F(1.0) - sa
    out_a = sa + da * rest
    with np.errstate(all="ignore"):
        inv = F(1.0) / out_a
        rgb = (src[..., :3].astype(F) * sa[..., None] + dst[..., :3].astype(F) * da[..., None] * rest[..., None]) * inv[..., None]
        out = np.concatenate([_round_u8(np.nan_to_num(rgb, posinf=0.0)), _round_u8(out_a * F(255.0))[..., None]], axis=-1)
    out[out_a < F(0.001)] = 0
    early_src = (src[..., 3] == 255) | (dst[..., 3] == 0)
    out[early_src] = src[early_src]
    out[src[..., 3] == 0] = dst[src[..., 3] == 0]
    return out


def _window(ov, g, px, py):
    """the inverse rotation and both window tests for pixel centres px (1, n) and py (m, 1): local x, local y, inside +-0.5, inside the tight window"""
    ax, ay = g["anchor"]
    rx, ry = px - ax, py - ay
    ur_x = rx * g["cos"] + ry * g["sin"] + ax                                        # :2094
    ur_y = -rx * g["sin"] + ry * g["cos"] + ay
    lx, ly = ur_x - g["origin"][0], ur_y - g["origin"][1]
    sw, sh = F(g["scaled_w"]), F(g["scaled_h"])
    inside = ~((lx < F(-0.5)) | (ly < F(-0.5)) | (lx >= sw + F(0.5)) | (ly >= sh + F(0.5)))
    tight = ~((lx < F(0.0)) | (ly < F(0.0)) | (lx >= sw) | (ly >= sh))
    return lx, ly, inside, tight


def _nearest_pick(img, lx, ly, valid):
    h, w = img.shape[:2]
    ix = np.minimum(np.where(valid, lx, 0).astype(np.int64), w - 1)                  # `local as u32` of a non-negative value, then .min
    iy = np.minimum(np.where(valid, ly, 0).astype(np.int64), h - 1)
    return img[iy, ix]


def _sample(ov, g, scaled, px, py, aa):
    lx, ly, inside, tight = _window(ov, g, px, py)
    valid = inside if aa else inside & tight
    if aa:
        src = sample_bilinear(scaled, np.where(valid, lx - F(0.5), F(0.0)), np.where(valid, ly - F(0.5), F(0.0)))
    else:
        src = _nearest_pick(scaled, lx, ly, valid)
    return src, lx, ly, valid, inside, tight


def commit(ov, source, base, overwrite_mask=None):
    """PasteOverlay::commit :2032 / render_replacement_preview :1144 on a copy of base: (image, branch counts)"""
    g = geometry(ov)
    out = np.array(base, np.uint8, copy=True)
    stats = dict(fringe=0, tight_rejected=0, blended=0, general=0, dst_transparent=0, skipped=0, overwritten=0, denied=0)
    if g["row_start"] > g["row_end"] or g["col_start"] > g["col_end"]:
        return out, stats
    scaled = scale_source(ov, g, source)
    ys, xs = np.arange(g["row_start"], g["row_end"] + 1), np.arange(g["col_start"], g["col_end"] + 1)
    px, py = (xs.astype(F) + F(0.5))[None, :], (ys.astype(F) + F(0.5))[:, None]      # dx as f32 + 0.5
    aa = bool(ov["anti_aliasing"])
    src, lx, ly, valid, inside, tight = _sample(ov, g, scaled, px, py, aa)
    stats["fringe"] = int((inside & ~tight).sum()) if aa else 0
    stats["tight_rejected"] = 0 if aa else int((inside & ~tight).sum())
    if ov["overwrite_transparent"]:
        if overwrite_mask is None:
            allowed = valid.copy()
        else:                                                                        # overwrite_mask_allows :1150
            smask = scale_mask(g, overwrite_mask)
            ok = valid & ~((lx < F(0.0)) | (ly < F(0.0)))
            allowed = ok & (_nearest_pick(smask, lx, ly, ok) > 0)
    else:
        allowed = np.zeros_like(valid)
    box = out[g["row_start"]:g["row_end"] + 1, g["col_start"]:g["col_end"] + 1]      # a view
    blend = valid & ~allowed & (src[..., 3] > 0)
    stats["overwritten"], stats["denied"] = int(allowed.sum()), int((valid & ~allowed).sum()) if ov["overwrite_transparent"] else 0
    stats["skipped"] = int((valid & ~allowed & (src[..., 3] == 0)).sum())
    partial = blend & (src[..., 3] < 255)
    stats["blended"], stats["dst_transparent"] = int(blend.sum()), int((partial & (box[..., 3] == 0)).sum())
    stats["general"] = int((partial & (box[..., 3] > 0)).sum())
    blended = alpha_blend(box, src)
    box[blend] = blended[blend]
    box[allowed] = src[allowed]
    return out, stats


def rasterize(ov, source):
    """rasterize_for_clipboard :1048: (image, (col_start, row_start)) or None"""
    g = geometry(ov)
    if g["raster"] is None:
        return None
    col_start, row_start, out_w, out_h = g["raster"]
    scaled = scale_source(ov, g, source)
    px = (F(col_start) + np.arange(out_w).astype(F) + F(0.5))[None, :]              # :1095: two additions
    py = (F(row_start) + np.arange(out_h).astype(F) + F(0.5))[:, None]
    src, _, _, valid, _, _ = _sample(ov, g, scaled, px, py, bool(ov["anti_aliasing"]))
    out = np.zeros((out_h, out_w, 4), np.uint8)
    keep = valid & (src[..., 3] > 0)
    out[keep] = src[keep]
    return (out, (col_start, row_start)) if (out[..., 3] > 0).any() else None


def preview(ov, source):
    """render_preview :2168 as a flat doc_h x doc_w image.  Two deviations, as include/pfx.h states them: a translation-only overlay whose origin + scaled size is
    negative draws nothing (the reference panics), and the general path draws the true column on documents wider than 65535"""
    g = geometry(ov)
    cw, ch = ov["doc_w"], ov["doc_h"]
    scaled = scale_source(ov, g, source, "nearest")                                  # :2184
    out = np.zeros((ch, cw, 4), np.uint8)
    sw, sh = g["scaled_w"], g["scaled_h"]
    if abs(F(ov["rotation"])) < F(0.0001) and abs(F(ov["anchor"][0])) < F(0.001) and abs(F(ov["anchor"][1])) < F(0.001):   # :2197
        ox, oy = as_i32(round_away(g["origin"][0])), as_i32(round_away(g["origin"][1]))
        x0, y0, x1, y1 = max(ox, 0), max(oy, 0), min(ox + sw, cw), min(oy + sh, ch)
        if x1 > x0 and y1 > y0:
            part = scaled[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
            out[y0:y1, x0:x1] = np.where(part[..., 3:4] > 0, part, 0)
        return out
    if g["row_start"] > g["row_end"] or g["col_start"] > g["col_end"]:
        return out
    ys, xs = np.arange(g["row_start"], g["row_end"] + 1), np.arange(g["col_start"], g["col_end"] + 1)
    lx, ly, _, tight = _window(ov, g, (xs.astype(F) + F(0.5))[None, :], (ys.astype(F) + F(0.5))[:, None])
    src = _nearest_pick(scaled, lx, ly, tight)
    keep = tight & (src[..., 3] > 0)
    out[g["row_start"]:g["row_end"] + 1, g["col_start"]:g["col_end"] + 1][keep] = src[keep]
    return out


def extract(layer, selection):
    """extract_to_overlay :729: (clip, clip_mask or None, the blanked layer, overlay) or None"""
    layer = np.asarray(layer, np.uint8)
    ch, cw = layer.shape[:2]
    if selection is None:
        if not (layer[..., 3] > 0).any():
            return None
        return layer.copy(), None, np.zeros_like(layer), overlay(cw, ch, cw, ch, (F(cw) / F(2.0), F(ch) / F(2.0)))
    selection = np.asarray(selection, np.uint8)
    ys, xs = np.nonzero(selection > 0)
    if len(xs) == 0:
        return None
    min_x, min_y, w, h = int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
    on = selection[min_y:min_y + h, min_x:min_x + w] > 0
    clip = np.where(on[..., None], layer[min_y:min_y + h, min_x:min_x + w], 0).astype(np.uint8)
    clip_mask = np.where(on, 255, 0).astype(np.uint8)
    center = (F(min_x) + F(w) / F(2.0), F(min_y) + F(h) / F(2.0))                    # :784
    return clip, clip_mask, SM.delete_selected(layer, selection), overlay(w, h, cw, ch, center)
