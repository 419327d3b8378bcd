"""CPU model of the line / curve tool (ref: src/ui/panels/tools/behavior/raster/bezier_math.rs :27-526, compute_line_alpha brush_render.rs:85-133,
commit_preview_to_layer_mask bezier_commit.rs:229-295, TiledImage::clear_region tiled_image.rs:954): every f32 operation of the reference, in its order, on
numpy float32 — one primitive at a time over its pixel box, the preview's alpha byte carried from primitive to primitive as the reference carries it.
`render(..., form="max")` is the form the kernel computes: the maximum pixel_alpha over the covering primitives, compared once with the start byte.
tests/test_linetool_model_host.py holds both to a scalar loop-for-loop transcription and to each other.

A tool is a dict: p (four (x, y)), size, color (r, g, b, a bytes), pattern 0 solid / 1 dotted / 2 dashed, cap_style 0 round / 1 flat, end_shape 0 none / 1 arrow,
arrow_side 0 end / 1 start / 2 both, anti_alias.

Vec2::length is taken to be emath's x.hypot(y) — a recollection, not verified against emath's source — and lives in vec2_length alone, calling the platform's
hypotf as the library does.  It moves the step count and a pattern's phase, never a pixel's arithmetic."""
import ctypes as C

import numpy as np

F = np.float32
CHUNK = 64
_libm = C.CDLL("libm.so.6")
_libm.hypotf.restype, _libm.hypotf.argtypes = C.c_float, [C.c_float, C.c_float]
_libm.fmodf.restype, _libm.fmodf.argtypes = C.c_float, [C.c_float, C.c_float]


def vec2_length(x, y):
    return F(_libm.hypotf(float(x), float(y)))


def as_u32(v):
    """Rust's `v as u32`: truncates, saturates, NaN -> 0"""
    v = float(v)
    if not v > 0.0:
        return 0
    return 0xFFFFFFFF if v >= 4294967296.0 else int(v)


def trunc_u8(a):
    """`v as u8` over an array"""
    a = np.asarray(a, F)
    return np.where(a != a, F(0), np.clip(np.trunc(a), F(0), F(255))).astype(np.uint8)


def rs_clamp(a, lo, hi):
    a = np.where(a < lo, lo, a)
    return np.where(a > hi, hi, a)       # a NaN stays


def rs_max(a, b):                        # f32::max / min: a NaN operand yields the other
    return F(np.fmax(F(a), F(b)))


def rs_min(a, b):
    return F(np.fmin(F(a), F(b)))


def bezier_point(p, t):
    t2 = t * t
    t3 = t2 * t
    mt = F(1) - t
    mt2 = mt * mt
    mt3 = mt2 * mt
    return (mt3 * p[0][0] + F(3) * mt2 * t * p[1][0] + F(3) * mt * t2 * p[2][0] + t3 * p[3][0],
            mt3 * p[0][1] + F(3) * mt2 * t * p[1][1] + F(3) * mt * t2 * p[2][1] + t3 * p[3][1])


def control_points(tool):
    return [(F(x), F(y)) for x, y in tool["p"]]


def bounds(tool, w, h):
    """get_bezier_bounds :41-73 as four f32"""
    with np.errstate(all="ignore"):
        p, size = control_points(tool), F(tool["size"])
        min_x = max_x = p[0][0]
        min_y = max_y = p[0][1]
        for q in p[1:]:
            min_x, max_x, min_y, max_y = rs_min(min_x, q[0]), rs_max(max_x, q[0]), rs_min(min_y, q[1]), rs_max(max_y, q[1])
        arrow_extra = rs_max(size * F(3), F(8)) + rs_max(size * F(1.5), F(4)) if tool["end_shape"] == 1 else F(0)
        padding = size / F(2) + F(2) + arrow_extra
        return np.array([rs_max(min_x - padding, F(0)), rs_max(min_y - padding, F(0)), rs_min(max_x + padding, F(w)), rs_min(max_y + padding, F(h))], F)


def plan(tool, w, h):
    """the dots of :131-210 before the selection test, (n, 2) f32; the arrowheads in draw order, (k, 3, 2) f32; what happened on the way"""
    with np.errstate(all="ignore"):
        p, size = control_points(tool), F(tool["size"])
        spacing = rs_max(size * F(0.1), F(0.5))
        chord = vec2_length(p[3][0] - p[0][0], p[3][1] - p[0][1])
        net = vec2_length(p[1][0] - p[0][0], p[1][1] - p[0][1]) + vec2_length(p[2][0] - p[1][0], p[2][1] - p[1][1]) + vec2_length(p[3][0] - p[2][0], p[3][1] - p[2][1])
        total = net + chord
        raw = float(np.ceil(total / spacing))
        raw_steps = 0 if raw != raw else (2 ** 64 - 1 if raw >= 2.0 ** 64 else max(int(raw), 0))
        steps = min(max(raw_steps, 20), 5000)
        pattern = tool["pattern"]
        on, off = {0: (F(0), F(0)), 1: (size * F(0.5), size * F(1.5)), 2: (size * F(2), size * F(1.5))}[pattern]
        cycle = on + off
        cumulative, prev = F(0), None
        dots, info = [], dict(steps=steps, raw_steps=raw_steps, off_canvas=0, pattern_off=0, flat_dropped=0, length=F(0))
        for i in range(steps + 1):
            t = F(i) / F(steps)
            pos = bezier_point(p, t)
            if prev is not None:
                cumulative = cumulative + vec2_length(pos[0] - prev[0], pos[1] - prev[1])
            prev = pos
            fx, fy = pos
            if not (fx >= 0 and fy >= 0 and as_u32(fx) < w and as_u32(fy) < h):
                info["off_canvas"] += 1
                continue
            if pattern != 0 and not (F(_libm.fmodf(float(cumulative), float(cycle))) < on):
                info["pattern_off"] += 1
                continue
            if tool["cap_style"] == 1 and i in (0, steps):
                info["flat_dropped"] += 1
                continue
            dots.append((fx, fy))
        info["length"] = cumulative
        return np.array(dots, F).reshape(-1, 2), arrow_triangles(tool), info


def arrow_triangles(tool):
    """:212-284: End first, then Start; each tip, wing1, wing2"""
    if tool["end_shape"] != 1:
        return np.zeros((0, 3, 2), F)
    with np.errstate(all="ignore"):
        p, size = control_points(tool), F(tool["size"])
        length, half = rs_max(size * F(3), F(8)), rs_max(size * F(1.5), F(4))
        advance = size + size / F(2)
        out = []
        if tool["arrow_side"] in (0, 2):
            tx, ty = F(3) * (p[3][0] - p[2][0]), F(3) * (p[3][1] - p[2][1])
            ln = rs_max(np.sqrt(tx * tx + ty * ty), F(0.001))
            dx, dy = tx / ln, ty / ln
            tip = (p[3][0] + dx * advance, p[3][1] + dy * advance)
            base = (tip[0] - dx * length, tip[1] - dy * length)
            px, py = -dy, dx
            out.append([tip, (base[0] + px * half, base[1] + py * half), (base[0] - px * half, base[1] - py * half)])
        if tool["arrow_side"] in (1, 2):
            tx, ty = F(3) * (p[1][0] - p[0][0]), F(3) * (p[1][1] - p[0][1])
            ln = rs_max(np.sqrt(tx * tx + ty * ty), F(0.001))
            dx, dy = tx / ln, ty / ln
            tip = (p[0][0] - dx * advance, p[0][1] - dy * advance)
            base = (tip[0] + dx * length, tip[1] + dy * length)
            px, py = -dy, dx
            out.append([tip, (base[0] + px * half, base[1] + py * half), (base[0] - px * half, base[1] - py * half)])
        return np.array(out, F).reshape(-1, 3, 2)


def clear_chunks(last_bounds, w, h):
    """:121-125 and clear_region: the half-open chunk ranges (cx0, cx1, cy0, cy1) that are dropped"""
    b = [F(v) for v in last_bounds]
    min_x, max_x = as_u32(rs_max(np.floor(b[0]), F(0))), as_u32(rs_min(np.ceil(b[2]), F(w)))
    min_y, max_y = as_u32(rs_max(np.floor(b[1]), F(0))), as_u32(rs_min(np.ceil(b[3]), F(h)))
    ncx, ncy = -(-w // CHUNK), -(-h // CHUNK)
    return min_x // CHUNK, min(-(-max_x // CHUNK), ncx), min_y // CHUNK, min(-(-max_y // CHUNK), ncy)


def clear(preview, last_bounds):
    h, w = preview.shape[:2]
    if last_bounds is None:
        preview[:] = 0
        return
    cx0, cx1, cy0, cy1 = clear_chunks(last_bounds, w, h)
    if cx0 < cx1 and cy0 < cy1:
        preview[cy0 * CHUNK:cy1 * CHUNK, cx0 * CHUNK:cx1 * CHUNK] = 0


def alpha_params(radius):
    """compute_line_alpha's (effective_radius, fade_width, solid_radius), brush_render.rs:98-118 with forced_hardness 0.95"""
    safe = rs_clamp(F(0.95), F(0), F(0.99))
    if radius < F(1.5):
        eff, fade = radius + F(1), F(1)
    elif radius < F(3):
        eff, fade = radius + F(1.5), F(1.5) + radius * (F(1) - safe)
    else:
        eff, fade = radius, rs_max(radius * (F(1) - safe), F(2))
    return F(eff), F(fade), F(eff - fade)


def dot_box(cx, cy, radius, aa, w, h):
    """:471-485; None = an empty loop range"""
    pad = (F(1.5) if radius < F(1.5) else rs_max(radius * (F(1) - F(0.95)), F(2)) + F(2)) if aa else F(1)
    outer = radius + pad
    x0, x1 = as_u32(rs_max(cx - outer, F(0))), min(as_u32(np.ceil(cx + outer)), w - 1)
    y0, y1 = as_u32(rs_max(cy - outer, F(0))), min(as_u32(np.ceil(cy + outer)), h - 1)
    return None if x0 > x1 or y0 > y1 else (x0, x1, y0, y1)


def dot_alpha(cx, cy, radius, aa, box):
    """compute_line_alpha over the box: (alpha, zone) — zone 0 none, 1 solid, 2 fade"""
    x0, x1, y0, y1 = box
    dx = np.arange(x0, x1 + 1, dtype=F)[None, :] - cx
    dy = np.arange(y0, y1 + 1, dtype=F)[:, None] - cy
    dist = np.sqrt(dx * dx + dy * dy)
    if not aa:
        inside = dist < radius
        return np.where(inside, F(1), F(0)), inside.astype(np.uint8)
    eff, fade, solid = alpha_params(radius)
    t = (dist - solid) / fade
    x = F(1) - rs_clamp(t, F(0), F(1))
    smooth = x * x * (F(3) - F(2) * x)
    alpha = np.where(dist <= solid, F(1), np.where(dist >= eff, F(0), smooth)).astype(F)
    zone = np.where(dist <= solid, 1, np.where(dist >= eff, 0, 2)).astype(np.uint8)
    return alpha, zone


def tri_box(tri, w, h):
    """:304-309; None = an empty loop range"""
    xs, ys = tri[:, 0], tri[:, 1]
    x0 = as_u32(rs_max(np.floor(rs_min(rs_min(xs[0], xs[1]), xs[2]) - F(1)), F(0)))
    x1 = min(as_u32(np.ceil(rs_max(rs_max(xs[0], xs[1]), xs[2]) + F(1))), max(w - 1, 0))
    y0 = as_u32(rs_max(np.floor(rs_min(rs_min(ys[0], ys[1]), ys[2]) - F(1)), F(0)))
    y1 = min(as_u32(np.ceil(rs_max(rs_max(ys[0], ys[1]), ys[2]) + F(1))), max(h - 1, 0))
    return None if x0 > x1 or y0 > y1 else (x0, x1, y0, y1)


def tri_sign(tri):
    a, b, c = tri
    ex, ey = b[0] - a[0], b[1] - a[1]
    cross = ex * (c[1] - a[1]) - ey * (c[0] - a[0])
    return F(1) if cross >= 0 else F(-1)


def tri_alpha(tri, src_a, box):
    """:335-359 over the box: (alpha, skipped by min_dist < -1, full) — alpha may hold NaN, which loses every comparison as in the reference"""
    x0, x1, y0, y1 = box
    px = np.arange(x0, x1 + 1, dtype=F)[None, :] + F(0.5)
    py = np.arange(y0, y1 + 1, dtype=F)[:, None] + F(0.5)
    sign = tri_sign(tri)

    def edge(v0, v1):
        ex, ey = v1[0] - v0[0], v1[1] - v0[1]
        ln = rs_max(np.sqrt(ex * ex + ey * ey), F(0.001))
        return ((ex * (py - v0[1]) - ey * (px - v0[0])) / ln) * sign

    a, b, c = tri
    min_dist = np.fmin(np.fmin(edge(a, b), edge(b, c)), edge(c, a))
    skipped = min_dist < F(-1)
    full = min_dist >= F(1)
    t = rs_clamp((min_dist + F(1)) / (F(2) * F(1)), F(0), F(1))
    smooth = t * t * (F(3) - F(2) * t)
    alpha = np.where(full, src_a, smooth * src_a).astype(F)
    return alpha, skipped, full


def color_bytes(color):
    """what a write leaves in the three colour channels: ((c as f32 / 255.0) * 255.0) as u8"""
    return [int(trunc_u8((F(c) / F(255)) * F(255))) for c in color[:3]]


def render(tool, preview, sel, last_bounds, form="serial"):
    """rasterize_bezier: (the new preview, this frame's bounds, stats).  form "serial": primitive after primitive with the alpha byte carried; "max": the
    maximum pixel_alpha over the covering primitives against the byte the frame started from"""
    out = np.ascontiguousarray(preview, np.uint8).copy()
    h, w = out.shape[:2]
    with np.errstate(all="ignore"):
        clear(out, last_bounds)
        dots, tris, info = plan(tool, w, h)
        radius, aa = F(tool["size"]) / F(2), bool(tool["anti_alias"])
        src_a = F(tool["color"][3]) / F(255)
        rgb = color_bytes(tool["color"])
        st = dict(info, n_listed=len(dots), sel_dropped=0, px_solid=0, px_fade=0, px_sel_skipped=0, writes=0, ties=0, clipped_low=0, clipped_high=0, tri_full=0,
                  tri_fade=0, tri_skipped=0, tri_empty=0, dot_chunks=set(), tri_chunks=set())
        best = np.zeros((h, w), F)

        def offer(box, pa, ok):
            x0, x1, y0, y1 = box
            region = out[y0:y1 + 1, x0:x1 + 1]
            if sel is not None:
                allowed = sel[y0:y1 + 1, x0:x1 + 1] != 0
                st["px_sel_skipped"] += int((ok & ~allowed).sum())
                ok = ok & allowed
            if form == "max":
                b = best[y0:y1 + 1, x0:x1 + 1]
                take = ok & (pa > b)
                b[take] = pa[take]
                return
            base = region[..., 3].astype(F) / F(255)
            write = ok & (pa > base)
            st["ties"] += int((ok & (pa == base)).sum())
            st["writes"] += int(write.sum())
            region[write] = np.concatenate([np.broadcast_to(np.array(rgb, np.uint8), pa.shape + (3,)), trunc_u8(pa * F(255))[..., None]], axis=-1)[write]

        for fx, fy in dots:
            if sel is not None and sel[as_u32(fy), as_u32(fx)] == 0:       # :189, the dot's own cell
                st["sel_dropped"] += 1
                continue
            box = dot_box(fx, fy, radius, aa, w, h)
            if box is None:
                continue
            st["clipped_low"] += int(fx - radius < 0 or fy - radius < 0)
            st["clipped_high"] += int(fx + radius > w - 1 or fy + radius > h - 1)
            st["dot_chunks"].update((cx, cy) for cx in range(box[0] // CHUNK, box[1] // CHUNK + 1) for cy in range(box[2] // CHUNK, box[3] // CHUNK + 1))
            alpha, zone = dot_alpha(fx, fy, radius, aa, box)
            st["px_solid"] += int((zone == 1).sum())
            st["px_fade"] += int((zone == 2).sum())
            offer(box, alpha * src_a, alpha > 0)
        for tri in tris:
            box = tri_box(tri, w, h)
            if box is None:
                st["tri_empty"] += 1
                continue
            st["tri_chunks"].update((cx, cy) for cx in range(box[0] // CHUNK, box[1] // CHUNK + 1) for cy in range(box[2] // CHUNK, box[3] // CHUNK + 1))
            alpha, skipped, full = tri_alpha(tri, src_a, box)
            st["tri_full"] += int((full & ~skipped).sum())
            st["tri_fade"] += int((~full & ~skipped & (alpha > 0)).sum())
            st["tri_skipped"] += int(skipped.sum())
            offer(box, alpha, ~skipped & ~(alpha <= 0))
        if form == "max":
            write = best > out[..., 3].astype(F) / F(255)
            st["writes"] = int(write.sum())
            out[write] = np.concatenate([np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)), trunc_u8(best * F(255))[..., None]], axis=-1)[write]
        return out, bounds(tool, w, h), st


def commit_mask(conceal, preview, sel, reveal):
    """commit_preview_to_layer_mask on the (h, w) conceal bytes"""
    old, s = conceal.astype(np.uint32), preview[..., 3].astype(np.uint32)
    new = (old * (255 - s)) // 255 if reveal else old + ((255 - old) * s) // 255
    touch = s != 0
    if sel is not None:
        touch &= sel != 0
    return np.where(touch, new, old).astype(np.uint8)
