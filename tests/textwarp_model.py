"""numpy-float32 restatement of the text block's warps, rotation and blit (ref: src/ops/text_layer/warp.rs — blit_rgba_buffer :39-70, apply_arc_warp :97-179,
arc_map_point :182-219, arc_inverse_map :222-274, apply_circular_warp :277-352, apply_path_follow_warp :355-444, apply_envelope_warp :447-539, the Bézier
helpers :546-704, bilinear_sample :707-740; raster.rs — rotate_glyph_buffer :561-653, the block's way into the layer :374-417; selection.rs —
maybe_rotate_and_blit :77-106).  Every f32 operation rounds once, in the reference's association order; `as u32` / `as i32` saturate; round() is half away
from zero; f32::min / max are fmin / fmax.

The reference has no test of any of this, so this model is the yardstick of the device kernels (k_textwarp.hip) and tests/test_textwarp_model_host.py holds
the model itself: against a scalar, pixel-loop transcription, against answers derived by hand, and by showing that each planted defect changes a case.

The per-pixel atan2 of the arc and circular warps goes through tests/shape_model.py's `Libm`: ``glibc`` is the host's atan2f, what the reference calls;
``device`` is the f64 atan2 rounded once, what the kernels evaluate, with its count of ambiguous calls.  What the reference evaluates once per image (the
arc's sin / cos of the bounds loop, the rotation's cos / sin) is the host's glibc in both flavours, as in the library.

`perturb` plants one deliberate defect: "bilinear_lerp" (the lerp form a + (b - a) t of the code base's other bilinears instead of the weight form),
"bilinear_clamp" (their taps clamped to the edge instead of transparent past it), "coarse_le" (<= in the path's coarse search: the last minimum wins),
"fmod" (fmod instead of the circular warp's two loops), "envelope_t" (t measured from the curves' own min_x, the repair the reference does not have)."""
import numpy as np

from .shape_model import F32_MAX, PI, TAU, F, Libm, as_i32, as_u8, cosf, round_away, sinf

KINDS = ["none", "arc", "circular", "path", "envelope"]
PERTURBATIONS = ["bilinear_lerp", "bilinear_clamp", "coarse_le", "fmod", "envelope_t"]
DEFAULTS = dict(bend=0.5, horizontal_distortion=0.0, vertical_distortion=0.0, radius=150.0, start_angle=float(F(-np.pi / 2)), clockwise=True,
                control_points=[(0.0, 0.0), (100.0, -50.0), (200.0, -50.0), (300.0, 0.0)],
                top_curve=[(0.0, -30.0), (100.0, -60.0), (200.0, -60.0), (300.0, -30.0)],
                bottom_curve=[(0.0, 30.0), (100.0, 60.0), (200.0, 60.0), (300.0, 30.0)])   # core.rs:230-293
MAX_START_ANGLE = F(8) * PI   # the library refuses a start angle beyond it (the reference's loops do not end for a large one)


def as_u32(v):   # `v as u32`
    v = float(v)
    if v != v:
        return 0
    return int(max(min(v, 4294967295.0), 0.0))


def fields_of(warp):
    """the warp's fields as f32, defaults filled in; `warp` = dict(kind=..., <the reference's field names>)"""
    f = DEFAULTS | {k: v for k, v in warp.items() if k != "kind"}
    out = {k: F(f[k]) for k in ("bend", "horizontal_distortion", "vertical_distortion", "radius", "start_angle")}
    out["clockwise"] = bool(f["clockwise"])
    for k in ("control_points", "top_curve", "bottom_curve"):
        out[k] = np.array([[F(p[0]), F(p[1])] for p in f[k]], F).reshape(-1, 2)
    return out


# ---- Bézier helpers :546-704 (t: an f32 scalar or array; p: (4, 2) f32) ----
def bezier(p, k, t):
    u = F(1) - t
    u2, t2 = u * u, t * t
    return u2 * u * p[0][k] + F(3) * u2 * t * p[1][k] + F(3) * u * t2 * p[2][k] + t2 * t * p[3][k]


def bezier_tangent(p, k, t):
    u = F(1) - t
    return F(3) * u * u * (p[1][k] - p[0][k]) + F(6) * u * t * (p[2][k] - p[1][k]) + F(3) * t * t * (p[3][k] - p[2][k])


def build_arc_length_table(p, steps=256):
    lengths, total = [F(0)], F(0)
    prev_x, prev_y = bezier(p, 0, F(0)), bezier(p, 1, F(0))
    for i in range(1, steps + 1):
        t = F(i) / F(steps)
        x, y = bezier(p, 0, t), bezier(p, 1, t)
        dx, dy = x - prev_x, y - prev_y
        total = total + np.sqrt(dx * dx + dy * dy)
        lengths.append(total)
        prev_x, prev_y = x, y
    return np.array(lengths, F), total


def arc_length_to_t(s, lengths, total):
    if s <= F(0):
        return F(0)
    if s >= total:
        return F(1)
    n = len(lengths) - 1
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if lengths[mid] < s:
            lo = mid + 1
        else:
            hi = mid
    if lo == 0:
        return F(0)
    seg_len = lengths[lo] - lengths[lo - 1]
    frac = (s - lengths[lo - 1]) / seg_len if seg_len > F(0) else F(0)
    return (F(lo - 1) + frac) / F(n)


# ---- the plans: the reference's bounds loops ----
class Box:
    def __init__(self):
        self.min_x, self.max_x, self.min_y, self.max_y = F32_MAX, -F32_MAX, F32_MAX, -F32_MAX

    def add(self, lo_x, hi_x, lo_y, hi_y):
        self.min_x, self.max_x = np.fmin(self.min_x, lo_x), np.fmax(self.max_x, hi_x)
        self.min_y, self.max_y = np.fmin(self.min_y, lo_y), np.fmax(self.max_y, hi_y)

    def grow(self, margin):
        self.min_x, self.min_y, self.max_x, self.max_y = self.min_x - margin, self.min_y - margin, self.max_x + margin, self.max_y + margin

    def size(self):
        return as_u32(np.ceil(self.max_x - self.min_x)), as_u32(np.ceil(self.max_y - self.min_y))

    def plan(self, out_w, out_h, **more):
        return dict(out_w=out_w, out_h=out_h, off_x=as_i32(np.floor(self.min_x)), off_y=as_i32(np.floor(self.min_y)), identity=False, min_x=self.min_x,
                    min_y=self.min_y, max_x=self.max_x, max_y=self.max_y, **more)


def identity_plan(sw, sh):
    return dict(out_w=sw, out_h=sh, off_x=0, off_y=0, identity=True, min_x=F(0), min_y=F(0), max_x=F(0), max_y=F(0))


def arc_map_point(sx, sy, w, h, radius, angle, hdist, vdist):   # :182-219
    cx = w / F(2)
    t = (sx - cx) / (w / F(2))
    theta = t * angle / F(2)
    r_sign = F(1) if angle > F(0) else F(-1)
    r_abs = np.abs(radius)
    sy_norm = sy / h
    r = r_abs - (F(1) - sy_norm) * h * r_sign
    dx = cx + r * sinf(theta)
    dy = r_abs - r * cosf(theta) * r_sign
    dx = dx + (dx - cx) * hdist
    dy = dy + (dy - h / F(2)) * vdist
    return dx, dy


def plan(warp, sw, sh):
    """the output's size, offset and f32 bounds of `warp` on a sw x sh source, with what the per-pixel loops need besides"""
    kind, f = warp.get("kind", "none"), fields_of(warp)
    w, h = F(sw), F(sh)
    with np.errstate(all="ignore"):
        if kind == "arc":
            bend, hd, vd = f["bend"], f["horizontal_distortion"], f["vertical_distortion"]
            if np.abs(bend) < F(0.001):
                return identity_plan(sw, sh)
            angle = bend * PI
            radius = w / (F(2) * sinf(angle / F(2))) if np.abs(angle) > F(0.01) else w * F(100)
            b = Box()
            for i in range(33):
                sx = (F(i) / F(32)) * w
                for sy in (F(0), h):
                    dx, dy = arc_map_point(sx, sy, w, h, radius, angle, hd, vd)
                    b.add(dx, dx, dy, dy)
            b.grow(F(2))
            out_w, out_h = b.size()
            if out_w == 0 or out_h == 0 or out_w > 8192 or out_h > 8192:
                return identity_plan(sw, sh)
            return b.plan(out_w, out_h, radius=radius, angle=angle)
        if kind == "circular":
            r = np.fmax(f["radius"], F(10))
            r_outer = r + h
            out_size = as_u32(np.ceil(r_outer * F(2) + F(4)))
            out_c = F(out_size) / F(2)
            return dict(out_w=out_size, out_h=out_size, off_x=as_i32(round_away(w / F(2) - out_c)), off_y=as_i32(round_away(h / F(2) - out_c)), identity=False,
                        min_x=F(0), min_y=F(0), max_x=F(0), max_y=F(0), r=r, r_outer=r_outer, out_c=out_c)
        if kind == "path":
            if len(f["control_points"]) < 4:
                return identity_plan(sw, sh)
            p = f["control_points"][:4]
            lengths, total = build_arc_length_table(p)
            b = Box()
            for i in range(65):
                s = (F(i) / F(64)) * total
                t = arc_length_to_t(s, lengths, total)
                px, py, ny = bezier(p, 0, t), bezier(p, 1, t), bezier_tangent(p, 1, t)
                for offset in (-h, F(0), h):
                    b.add(px - np.abs(offset), px + np.abs(offset), py + offset + np.abs(ny) * h, py - offset - np.abs(ny) * h)
            b.grow(h + F(10))
            out_w, out_h = min(b.size()[0], 4096), min(b.size()[1], 4096)
            if out_w == 0 or out_h == 0:
                return identity_plan(sw, sh)
            return b.plan(out_w, out_h, lengths=lengths, total=total)
        if kind == "envelope":
            if len(f["top_curve"]) < 4 or len(f["bottom_curve"]) < 4:
                return identity_plan(sw, sh)
            top, bot = f["top_curve"][:4], f["bottom_curve"][:4]
            b = Box()
            for i in range(65):
                t = F(i) / F(64)
                tx, ty, bx, by = bezier(top, 0, t), bezier(top, 1, t), bezier(bot, 0, t), bezier(bot, 1, t)
                b.add(np.fmin(tx, bx), np.fmax(tx, bx), np.fmin(ty, by), np.fmax(ty, by))
            b.grow(F(4))
            out_w, out_h = min(b.size()[0], 4096), min(b.size()[1], 4096)
            if out_w == 0 or out_h == 0:
                return identity_plan(sw, sh)
            return b.plan(out_w, out_h)
    assert kind == "none", kind
    return identity_plan(sw, sh)


def rotate_plan(w, h, angle, pivot=None):
    """rotate_glyph_buffer's bounds :568-600, :649-650; the identity when |angle| <= 0.001 (selection.rs:89)"""
    angle = F(angle)
    if not np.abs(angle) > F(0.001):
        return identity_plan(w, h)
    cos_a, sin_a, fw, fh = cosf(angle), sinf(angle), F(w), F(h)
    cx, cy = (F(pivot[0]), F(pivot[1])) if pivot is not None else (fw * F(0.5), fh * F(0.5))
    b = Box()
    with np.errstate(all="ignore"):
        for px, py in ((F(0), F(0)), (fw, F(0)), (F(0), fh), (fw, fh)):
            dx, dy = px - cx, py - cy
            rx, ry = dx * cos_a - dy * sin_a + cx, dx * sin_a + dy * cos_a + cy
            b.add(rx, rx, ry, ry)
        new_w, new_h = b.size()
        return b.plan(new_w + 1, new_h + 1, cos_a=cos_a, sin_a=sin_a, cx=cx, cy=cy, new_cx=cx - np.floor(b.min_x), new_cy=cy - np.floor(b.min_y))


# ---- bilinear_sample :707-740 at the pixels of `keep` ----
def gather(src, sx, sy, keep, perturb=None):
    """src (h, w, 4) u8; sx, sy f32 grids; keep: the pixels the reference samples (0 <= sx < w, 0 <= sy < h there).  The rest is transparent"""
    sh, sw = src.shape[:2]
    out = np.zeros(sx.shape + (4,), np.uint8)
    if not keep.any():
        return out
    x, y = sx[keep], sy[keep]
    x0f, y0f = np.floor(x), np.floor(y)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    fx, fy = (x - x0f)[:, None], (y - y0f)[:, None]

    def tap(xi, yi):
        inside = (xi >= 0) & (yi >= 0) & (xi < sw) & (yi < sh) if perturb != "bilinear_clamp" else np.ones(xi.shape, bool)
        return np.where(inside[:, None], src[np.clip(yi, 0, sh - 1), np.clip(xi, 0, sw - 1)].astype(F), F(0))

    p00, p10, p01, p11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    if perturb == "bilinear_lerp":
        top, bot = p00 + (p10 - p00) * fx, p01 + (p11 - p01) * fx
        v = top + (bot - top) * fy
    else:
        v = p00 * (F(1) - fx) * (F(1) - fy) + p10 * fx * (F(1) - fy) + p01 * (F(1) - fx) * fy + p11 * fx * fy
    out[keep] = as_u8(np.clip(round_away(v), F(0), F(255)))
    return out


def grids(out_w, out_h):
    return np.broadcast_to(np.arange(out_w, dtype=F)[None, :], (out_h, out_w)), np.broadcast_to(np.arange(out_h, dtype=F)[:, None], (out_h, out_w))


def inside(sx, sy, w, h):
    return (sx >= F(0)) & (sx < w) & (sy >= F(0)) & (sy < h)


def apply_warp(src, warp, libm=None, perturb=None):
    """apply_block_warp: (out, plan, painted) — the warped image, its plan and how many output pixels were sampled.  An identity plan returns the source"""
    assert perturb is None or perturb in PERTURBATIONS
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape[:2]
    kind, f, P = warp.get("kind", "none"), fields_of(warp), plan(warp, sw, sh)
    if P["identity"]:
        return src.copy(), P, int((src[..., 3] > 0).sum())
    libm = libm or Libm("glibc")
    w, h = F(sw), F(sh)
    ox, oy = grids(P["out_w"], P["out_h"])
    with np.errstate(all="ignore"):
        if kind == "arc":
            angle, radius, hd, vd = P["angle"], P["radius"], f["horizontal_distortion"], f["vertical_distortion"]
            cx, r_sign, r_abs = w / F(2), (F(1) if angle > F(0) else F(-1)), np.abs(radius)
            dx, dy = ox + P["min_x"], oy + P["min_y"]
            if np.abs(hd) > F(0.001):
                dx = cx + (dx - cx) / (F(1) + hd)
            if np.abs(vd) > F(0.001):
                dy = h / F(2) + (dy - h / F(2)) / (F(1) + vd)
            rel_x, rel_y = dx - cx, r_abs - dy * r_sign
            r = np.sqrt(rel_x * rel_x + (rel_y * r_sign) * (rel_y * r_sign))
            sy = (F(1) - (r_abs - r) / (h * r_sign)) * h
            keep = (sy >= F(0)) & (sy < h)       # sy needs no atan2: only these pixels reach it (the rejections are pure, their order is free)
            curved = np.abs(angle) > F(0.01)
            theta = np.zeros(dx.shape, F)
            if curved:
                theta[keep] = libm.atan2(rel_x[keep], (rel_y * r_sign)[keep])
                keep = keep & ~(np.abs(theta) > np.abs(angle / F(2)) + F(0.1))
                t = theta / (angle / F(2))
            else:
                t = (dx - cx) / (w / F(2))
            sx = cx + t * w / F(2)
            keep = keep & inside(sx, sy, w, h)
        elif kind == "circular":
            r, r_outer, out_c = P["r"], P["r_outer"], P["out_c"]
            assert np.abs(f["start_angle"]) <= MAX_START_ANGLE
            direction = F(1) if f["clockwise"] else F(-1)
            px, py = ox - out_c, oy - out_c
            dist = np.sqrt(px * px + py * py)
            sy = r_outer - dist
            keep = ~((dist < r) | (dist > r_outer)) & (sy >= F(0)) & (sy < h)
            rel = np.zeros(px.shape, F)
            rel[keep] = (libm.atan2(py[keep], px[keep]) - f["start_angle"]) * direction
            if perturb == "fmod":
                rel = np.fmod(rel, TAU)
                rel = np.where(rel < F(0), rel + TAU, rel)
            else:
                while (rel < F(0)).any():
                    rel = np.where(rel < F(0), rel + TAU, rel)
                while (rel >= TAU).any():
                    rel = np.where(rel >= TAU, rel - TAU, rel)
            sx = rel * r
            keep = keep & inside(sx, sy, w, h)
        elif kind == "path":
            p, lengths = f["control_points"][:4], P["lengths"]
            px, py = ox + P["min_x"], oy + P["min_y"]
            best_t, best = np.zeros(px.shape, F), np.full(px.shape, F32_MAX, F)
            for i in range(65):
                t = F(i) / F(64)
                cx, cy = bezier(p, 0, t), bezier(p, 1, t)
                d = (px - cx) * (px - cx) + (py - cy) * (py - cy)
                closer = d <= best if perturb == "coarse_le" else d < best
                best, best_t = np.where(closer, d, best), np.where(closer, t, best_t)
            step = F(1) / F(64)
            t_lo, t_hi = np.fmax(best_t - step, F(0)), np.fmin(best_t + step, F(1))
            for _ in range(8):
                t_mid = (t_lo + t_hi) / F(2)
                t_a, t_b = (t_lo + t_mid) / F(2), (t_mid + t_hi) / F(2)
                ax, ay, bx, by = bezier(p, 0, t_a), bezier(p, 1, t_a), bezier(p, 0, t_b), bezier(p, 1, t_b)
                da, db = (px - ax) * (px - ax) + (py - ay) * (py - ay), (px - bx) * (px - bx) + (py - by) * (py - by)
                t_hi, t_lo = np.where(da < db, t_mid, t_hi), np.where(da < db, t_lo, t_mid)
            t = (t_lo + t_hi) / F(2)
            cx, cy, tx, ty = bezier(p, 0, t), bezier(p, 1, t), bezier_tangent(p, 0, t), bezier_tangent(p, 1, t)
            tangent_len = np.sqrt(tx * tx + ty * ty)
            nx, ny = -ty / tangent_len, tx / tangent_len
            perp = (px - cx) * nx + (py - cy) * ny
            idx_f = t * F(256)
            idx = np.minimum(idx_f.astype(np.int64), 255)
            sx = lengths[idx] + (idx_f - idx.astype(F)) * (lengths[idx + 1] - lengths[idx])
            sy = h / F(2) - perp
            keep = ~(tangent_len < F(0.0001)) & inside(sx, sy, w, h)
        else:
            top, bot, margin = f["top_curve"][:4], f["bottom_curve"][:4], F(4)
            px, py = ox + P["min_x"], oy + P["min_y"]
            origin = P["min_x"] + margin if perturb == "envelope_t" else P["min_x"]
            t = (px - origin) / np.fmax(P["max_x"] - P["min_x"] - F(2) * margin, F(1))
            top_y, bot_y = bezier(top, 1, t), bezier(bot, 1, t)
            span = bot_y - top_y
            v = (py - top_y) / span
            sx, sy = t * w, v * h
            keep = (t >= F(0)) & (t <= F(1)) & ~(np.abs(span) < F(0.001)) & (v >= F(0)) & (v <= F(1)) & inside(sx, sy, w, h)
        return gather(src, sx, sy, keep, perturb), P, int(keep.sum())


def rotate(buf, angle, pivot=None):
    """rotate_glyph_buffer through maybe_rotate_and_blit's gate: (out, plan)"""
    buf = np.ascontiguousarray(buf, np.uint8)
    h, w = buf.shape[:2]
    P = rotate_plan(w, h, angle, pivot)
    if P["identity"]:
        return buf.copy(), P
    ox, oy = grids(P["out_w"], P["out_h"])
    fw, fh, cos_a, sin_a = F(w), F(h), P["cos_a"], P["sin_a"]
    with np.errstate(all="ignore"):
        dx, dy = ox - P["new_cx"], oy - P["new_cy"]
        sx = dx * cos_a + dy * sin_a + P["cx"]
        sy = -dx * sin_a + dy * cos_a + P["cy"]
        keep = inside(sx, sy, fw, fh)
        out = np.zeros((P["out_h"], P["out_w"], 4), np.uint8)
        x, y = sx[keep], sy[keep]
        x0f, y0f = np.floor(x), np.floor(y)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = (x - x0f)[:, None], (y - y0f)[:, None]
        p00, p10, p01, p11 = buf[y0, x0].astype(F), buf[y0, x1].astype(F), buf[y1, x0].astype(F), buf[y1, x1].astype(F)
        v = p00 * (F(1) - fx) * (F(1) - fy) + p10 * fx * (F(1) - fy) + p01 * (F(1) - fx) * fy + p11 * fx * fy
        out[keep] = as_u8(np.clip(round_away(v), F(0), F(255)))
    return out, P


def blit(canvas, buf, off_x, off_y):
    """blit_rgba_buffer :39-70, in place: alpha 0 keeps the canvas pixel, any other pixel replaces it; clipped"""
    ch, cw = canvas.shape[:2]
    bh, bw = buf.shape[:2]
    x0, y0, x1, y1 = max(0, -off_x), max(0, -off_y), min(bw, cw - off_x), min(bh, ch - off_y)
    if x1 <= x0 or y1 <= y0:
        return canvas
    part = buf[y0:y1, x0:x1]
    dst = canvas[y0 + off_y:y1 + off_y, x0 + off_x:x1 + off_x]
    opaque = part[..., 3] != 0
    dst[opaque] = part[opaque]
    return canvas


def place(canvas, src, warp, offset, rotation=0.0, pivot=None, libm=None, perturb=None):
    """raster.rs:374-417 on a copy of `canvas`: warp, rotate around the pivot (canvas coordinates) seen from the warped buffer, blit"""
    canvas = np.array(canvas, np.uint8)
    buf, P, _ = apply_warp(src, warp, libm, perturb)
    off_x, off_y = int(offset[0]) + P["off_x"], int(offset[1]) + P["off_y"]
    local = None if pivot is None else (F(pivot[0]) - F(off_x), F(pivot[1]) - F(off_y))
    buf, R = rotate(buf, rotation, local)
    return blit(canvas, buf, off_x + R["off_x"], off_y + R["off_y"])
