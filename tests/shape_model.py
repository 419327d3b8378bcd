"""numpy-float32 restatement of the reference's built-in shape rasteriser (ref: src/ops/shapes.rs): `shape_sdf` (:357-847), `coverage_from_sdf` /
`smoothstep` (:850-858, :1441-1444), the fill / outline / both colour mix and the bounding box of `rasterize_shape` (:1169-1305), and the golden
tests' `rasterize_to_canvas` (tests/visual_shapes.rs:18-41).  Every f32 operation rounds once, in the reference's association order.

Two libm flavours for the per-pixel transcendentals of the regular polygons and stars (atan2 / cos / sin; `%` is fmodf, exact by definition):

* ``glibc``  — the host's atan2f / cosf / sinf through ctypes: what the reference calls;
* ``device`` — Python's f64 ``math.*`` rounded once to f32: what the HIP kernel evaluates.  Calls whose f64 result lies within 4 f64 ulps of an f32
  rounding boundary are counted as *ambiguous*: only there may the device's f64 routine round differently.

Everything the reference evaluates once per image (rotation cos / sin, polygon and star angles, the heart's 96-vertex path) goes through the host's
glibc in both flavours, as in the library.  `perturb` plants one deliberate defect so that the tests can show the goldens reject it."""
import ctypes as C
import ctypes.util
import math

import numpy as np

F = np.float32
KINDS = ["ellipse", "rectangle", "rounded_rect", "trapezoid", "parallelogram", "triangle", "right_triangle", "pentagon", "hexagon", "octagon", "cross",
         "check", "heart", "diamond", "star5", "star6", "arrow"]  # ShapeKind, shapes.rs:159-178
FILLS = ["outline", "filled", "both"]                             # ShapeFillMode, shapes.rs:268-272
LIBM_KINDS = {"pentagon", "hexagon", "octagon", "star5", "star6"}
F32_MAX = F(3.4028234663852886e38)
TAU, PI, FRAC_PI_2 = F(6.28318530717958647692), F(3.14159265358979323846), F(1.57079632679489661923)

_m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf"):
    getattr(_m, _n).restype = C.c_float
    getattr(_m, _n).argtypes = [C.c_float]
_m.atan2f.restype = C.c_float
_m.atan2f.argtypes = [C.c_float, C.c_float]


def sinf(x):
    return F(_m.sinf(float(x)))


def cosf(x):
    return F(_m.cosf(float(x)))


class Libm:
    """the per-pixel transcendentals under one flavour; `ambiguous` counts device-flavour calls near an f32 rounding boundary"""

    def __init__(self, flavour="glibc"):
        assert flavour in ("glibc", "device")
        self.flavour, self.ambiguous = flavour, 0

    def _round_once(self, r64):
        f = r64.astype(F)
        with np.errstate(over="ignore", invalid="ignore"):
            lo, hi = np.nextafter(f, F(-np.inf)).astype(np.float64), np.nextafter(f, F(np.inf)).astype(np.float64)
            f64 = f.astype(np.float64)
            dist = np.minimum(np.abs(r64 - (f64 + lo) * 0.5), np.abs(r64 - (f64 + hi) * 0.5))
            self.ambiguous += int((dist <= 4.0 * np.spacing(np.abs(r64))).sum())
        return f

    def _map(self, f32fn, f64fn, *args):
        args = [np.asarray(a, F) for a in args]
        if self.flavour == "glibc":
            return np.frompyfunc(lambda *v: f32fn(*[float(t) for t in v]), len(args), 1)(*args).astype(F)
        return self._round_once(np.frompyfunc(lambda *v: f64fn(*[float(t) for t in v]), len(args), 1)(*args).astype(np.float64))

    def atan2(self, y, x):
        return self._map(_m.atan2f, math.atan2, y, x)

    def cos(self, x):
        return self._map(_m.cosf, math.cos, x)

    def sin(self, x):
        return self._map(_m.sinf, math.sin, x)


# ---- Rust f32 semantics ----
def rmin(a, b):   # f32::min: the non-NaN operand
    return np.fmin(a, b).astype(F)


def rmax(a, b):
    return np.fmax(a, b).astype(F)


def rclamp(x, lo, hi):   # f32::clamp: NaN stays NaN
    return np.where(x < lo, F(lo), np.where(x > hi, F(hi), x)).astype(F)


def as_u8(v):     # `v as u8`: truncates, saturates, NaN -> 0
    v = np.asarray(v, F)
    return np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0)), 0, 255)).astype(np.uint8)


def round_away(v):   # f32::round: half away from zero
    v = np.asarray(v, F)
    t = np.trunc(v)
    return np.where(np.abs(v - t) >= F(0.5), t + np.copysign(F(1), v), t).astype(F)


def as_i32(v):    # `v as i32`
    v = float(v)
    if v != v:
        return 0
    return int(max(min(v, 2147483647.0), -2147483648.0))


# ---- SDFs (negative = inside) ----
def sdf_box(px, py, hx, hy):                                     # :359
    dx, dy = np.abs(px) - hx, np.abs(py) - hy
    outside = np.sqrt(rmax(dx, F(0)) * rmax(dx, F(0)) + rmax(dy, F(0)) * rmax(dy, F(0)))
    return outside + rmin(rmax(dx, dy), F(0))


def sdf_rounded_box(px, py, hx, hy, r):                          # :369
    r = rmin(rmin(F(r), hx), hy)
    return sdf_box(px, py, hx - r, hy - r) - r


def sdf_ellipse(px, py, rx, ry):                                 # :376
    nx, ny = px / rx, py / ry
    ln = np.sqrt(nx * nx + ny * ny)
    scale = np.sqrt(rx * rx * ny * ny + ry * ry * nx * nx) / (rx * ry * ln)
    return np.where(ln < F(1e-8), -rmin(rx, ry), (ln - F(1)) / scale).astype(F)


def sdf_line_segment(px, py, ax, ay, bx, by):                    # :816
    dx, dy = bx - ax, by - ay
    t = rclamp(((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy), 0, 1)
    cx, cy = ax + t * dx, ay + t * dy
    return np.sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy))


def sdf_triangle_box(px, py, hx, hy):                            # :390
    ax, ay, bx, by, cx, cy = F(0), -hy, hx, hy, -hx, hy
    d1 = sdf_line_segment(px, py, ax, ay, bx, by)
    d2 = sdf_line_segment(px, py, bx, by, cx, cy)
    d3 = sdf_line_segment(px, py, cx, cy, ax, ay)
    edge = rmin(d1, rmin(d2, d3))
    c1 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    c2 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
    c3 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
    inside = ((c1 >= 0) & (c2 >= 0) & (c3 >= 0)) | ((c1 <= 0) & (c2 <= 0) & (c3 <= 0))
    return np.where(inside, -edge, edge).astype(F)


def sdf_polygon(px, py, r, n, lm):                               # :412
    angle = TAU / F(n)
    half = angle * F(0.5)
    theta = lm.atan2(py, px) + FRAC_PI_2
    theta = np.fmod(np.fmod(theta, angle) + angle, angle) - half
    ln = np.sqrt(px * px + py * py)
    return ln * lm.cos(theta) - r * cosf(half)


def sdf_polygon_stretched(px, py, hx, hy, n, lm):                # :425
    r = rmax(rmin(hx, hy), F(0.001))
    sx, sy = r / rmax(hx, F(0.001)), r / rmax(hy, F(0.001))
    return sdf_polygon(px * sx, py * sy, r, n, lm) / rmax(sx, sy)


def sdf_star(px, py, ro, ri, n, lm):                             # :433
    angle = PI / F(n)
    theta = lm.atan2(py, px) + FRAC_PI_2
    theta = np.fmod(np.fmod(theta, F(2) * angle) + F(2) * angle, F(2) * angle)
    ln = np.sqrt(px * px + py * py)
    cos_a, sin_a = cosf(angle), sinf(angle)
    ax, ay, bx, by = ro, F(0), ri * cos_a, ri * sin_a
    qx, qy = ln * lm.cos(theta - angle), ln * lm.sin(theta - angle)
    ex, ey, fx, fy = bx - ax, by - ay, qx - ax, qy - ay
    t = rclamp((fx * ex + fy * ey) / (ex * ex + ey * ey), 0, 1)
    cx, cy = ax + ex * t - qx, ay + ey * t - qy
    dist = np.sqrt(cx * cx + cy * cy)
    return np.where(ex * fy - ey * fx < 0, -dist, dist).astype(F)


def sdf_diamond(px, py, hx, hy):                                 # :467
    d = np.abs(px) / hx + np.abs(py) / hy - F(1)
    return d * (F(1) / np.sqrt(F(1) / (hx * hx) + F(1) / (hy * hy)))


def sdf_arrow(px, py, hx, hy):                                   # :475
    shaft_w, shaft_h, head_x = hx * F(0.55), hy * F(0.35), hx * F(0.05)
    shaft = sdf_box(px - (-hx + shaft_w) * F(0.5), py, shaft_w * F(0.5) + hx * F(0.25), shaft_h)
    tx, tw = px - head_x, hx - head_x
    max_y = hy * (F(1) - tx / tw)
    dy = np.abs(py) - max_y
    nl = np.sqrt(-hy * -hy + tw * tw)
    dpx, dpy = px - hx, np.abs(py) - F(0)
    above = rmin(rmax(dpx * (-hy / nl) + dpy * (tw / nl), F(0)), np.sqrt(dpx * dpx + dpy * dpy))
    past = np.sqrt((px - hx) * (px - hx) + py * py)
    inside = -rmax(rmin(max_y - np.abs(py), (tw - tx) * hy / np.sqrt(hy * hy + tw * tw)), F(0))
    return np.where(px < head_x, shaft, np.where(dy > 0, above, np.where(tx > tw, past, inside))).astype(F)


def sdf_polygon_path(verts, px, py):                             # :519
    min_dist = np.full(px.shape, F32_MAX, F)
    inside = np.zeros(px.shape, bool)
    prev = verts[-1]
    for curr in verts:
        min_dist = rmin(min_dist, sdf_line_segment(px, py, prev[0], prev[1], curr[0], curr[1]))
        edge_dy = prev[1] - curr[1]
        if abs(edge_dy) > F(1.1920929e-07):
            crosses = (curr[1] > py) != (prev[1] > py)
            edge_x = (prev[0] - curr[0]) * (py - curr[1]) / edge_dy + curr[0]
            inside ^= crosses & (px < edge_x)
        prev = curr
    return np.where(inside, -min_dist, min_dist).astype(F)


def heart_vertices(hx, hy):                                      # :545-573, host libm
    raw, max_x, max_y = [], F(0), F(0)
    for i in range(96):
        t = F(i) * TAU / F(96)
        s, c = sinf(t), cosf(t)
        xr = F(16) * s * s * s
        yr = F(13) * c - F(5) * cosf(F(2) * t) - F(2) * cosf(F(3) * t) - cosf(F(4) * t)
        max_x, max_y = rmax(max_x, abs(xr)), rmax(max_y, abs(yr))
        raw.append((xr, yr))
    sx = hx * F(0.98) / max_x if max_x > 0 else F(1)
    sy = hy * F(0.98) / max_y if max_y > 0 else F(1)
    return [(F(xr * sx), F(-yr * sy)) for xr, yr in raw]


def sdf_heart(px, py, hx, hy):
    return sdf_polygon_path(heart_vertices(hx, hy), px, py + hy * F(0.18))


def sdf_convex_polygon(verts, px, py):                           # :607
    n = len(verts)
    d = (px - verts[0][0]) * (px - verts[0][0]) + (py - verts[0][1]) * (py - verts[0][1])
    s = np.ones(px.shape, F)
    j = n - 1
    for i in range(n):
        ex, ey = verts[j][0] - verts[i][0], verts[j][1] - verts[i][1]
        wx, wy = px - verts[i][0], py - verts[i][1]
        t = rclamp((wx * ex + wy * ey) / (ex * ex + ey * ey), 0, 1)
        bx, by = wx - ex * t, wy - ey * t
        d = rmin(d, bx * bx + by * by)
        c1, c2, c3 = py >= verts[i][1], py < verts[j][1], ex * wy > ey * wx
        s = np.where((c1 & c2 & c3) | (~c1 & ~c2 & ~c3), -s, s)
        j = i
    return (s * np.sqrt(d)).astype(F)


def convex_vertices(kind, hx, hy):                               # :580-604
    if kind == "trapezoid":
        top = hx * F(0.55)
        return [(-top, -hy), (top, -hy), (hx, hy), (-hx, hy)]
    if kind == "parallelogram":
        skew = hx * F(0.3)
        return [(-hx, -hy), (hx, -hy), (hx + skew, hy), (-hx + skew, hy)]
    return [(-hx, hy), (hx, hy), (-hx, -hy)]


def sdf_cross(px, py, hx, hy):                                   # :784
    return rmin(sdf_box(px, py, hx * F(0.34), hy), sdf_box(px, py, hx, hy * F(0.34)))


def sdf_check(px, py, hx, hy):                                   # :793
    th = rmin(hx, hy) * F(0.2)
    d1 = sdf_line_segment(px, py, -hx * F(0.7), hy * F(0.0), -hx * F(0.1), hy * F(0.6)) - th
    d2 = sdf_line_segment(px, py, -hx * F(0.1), hy * F(0.6), hx * F(0.8), -hy * F(0.7)) - th
    return rmin(d1, d2)


def shape_sdf(kind, px, py, hx, hy, corner_radius, lm):          # :827
    if kind == "rectangle":
        return sdf_box(px, py, hx, hy)
    if kind == "ellipse":
        return sdf_ellipse(px, py, hx, hy)
    if kind == "rounded_rect":
        return sdf_rounded_box(px, py, hx, hy, corner_radius)
    if kind == "triangle":
        return sdf_triangle_box(px, py, hx, hy)
    if kind in ("right_triangle", "trapezoid", "parallelogram"):
        return sdf_convex_polygon(convex_vertices(kind, hx, hy), px, py)
    if kind == "diamond":
        return sdf_diamond(px, py, hx, hy)
    if kind in ("pentagon", "hexagon", "octagon"):
        return sdf_polygon_stretched(px, py, hx, hy, {"pentagon": 5, "hexagon": 6, "octagon": 8}[kind], lm)
    if kind == "cross":
        return sdf_cross(px, py, hx, hy)
    if kind == "check":
        return sdf_check(px, py, hx, hy)
    if kind == "star5":
        return sdf_star(px, py, rmin(hx, hy), rmin(hx, hy) * F(0.4), 5, lm)
    if kind == "star6":
        return sdf_star(px, py, rmin(hx, hy), rmin(hx, hy) * F(0.5), 6, lm)
    if kind == "arrow":
        return sdf_arrow(px, py, hx, hy)
    if kind == "heart":
        return sdf_heart(px, py, hx, hy)
    raise ValueError(kind)


def coverage_from_sdf(d, aa):                                    # :850, smoothstep(0.5, -0.5, d) :1441
    if not aa:
        return np.where(d < 0, F(1), F(0)).astype(F)
    t = rclamp((d - F(0.5)) / (F(-0.5) - F(0.5)), 0, 1)
    return t * t * (F(3) - F(2) * t)


# ---- the rasteriser ----
def shape(kind, fill, cx=64.0, cy=64.0, hw=40.0, hh=40.0, rotation=0.0, outline_width=3.0, corner_radius=0.0, primary=(255, 80, 80, 255),
          secondary=(80, 80, 255, 255), anti_alias=True):
    """a PlacedShape as a dict; the defaults are the golden tests' make_shape (tests/visual_shapes.rs:44-66)"""
    return dict(kind=kind, fill=fill, cx=F(cx), cy=F(cy), hw=F(hw), hh=F(hh), rotation=F(rotation), outline_width=F(outline_width),
                corner_radius=F(corner_radius), primary=tuple(primary), secondary=tuple(secondary), anti_alias=bool(anti_alias))


def bounds(s, canvas_w, canvas_h):
    """(x0, y0, bw, bh) of rasterize_shape (:1175-1207); an empty box is (0, 0, 0, 0)"""
    cos_r, sin_r = cosf(s["rotation"]), sinf(s["rotation"])
    hw, hh = s["hw"], s["hh"]
    if s["kind"] == "parallelogram":                             # shape_local_corners :1055
        skew = hw * F(0.3)
        corners = [(-hw, -hh), (hw, -hh), (hw + skew, hh), (-hw + skew, hh)]
    else:
        corners = [(-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh)]
    min_x = min_y = F32_MAX
    max_x = max_y = -F32_MAX
    with np.errstate(over="ignore", invalid="ignore"):
        for x, y in corners:
            rx, ry = x * cos_r - y * sin_r + s["cx"], x * sin_r + y * cos_r + s["cy"]
            min_x, min_y, max_x, max_y = rmin(min_x, rx), rmin(min_y, ry), rmax(max_x, rx), rmax(max_y, ry)
        min_x, min_y, max_x, max_y = min_x - F(2), min_y - F(2), max_x + F(2), max_y + F(2)
    x0, y0 = max(as_i32(np.floor(min_x)), 0), max(as_i32(np.floor(min_y)), 0)
    x1, y1 = min(as_i32(np.ceil(max_x)), canvas_w), min(as_i32(np.ceil(max_y)), canvas_h)
    bw, bh = max(x1 - x0, 0), max(y1 - y0, 0)
    return (0, 0, 0, 0) if bw == 0 or bh == 0 else (x0, y0, bw, bh)


def rasterize(s, canvas_w, canvas_h, flavour="glibc", perturb=None):
    """rasterize_shape's `buf` over the box: ((bh, bw, 4) uint8, (x0, y0, bw, bh), ambiguous libm calls).
    perturb: None | "trunc_alpha" (the alpha's round() replaced by truncation) | "fma_rotate" (lx's multiply-add contracted)"""
    x0, y0, bw, bh = box = bounds(s, canvas_w, canvas_h)
    if bw == 0:
        return np.zeros((0, 0, 4), np.uint8), box, 0
    lm = Libm(flavour)
    cos_r, sin_r = cosf(s["rotation"]), sinf(s["rotation"])
    inv_cos, inv_sin = cos_r, -sin_r
    pxc = (np.arange(x0, x0 + bw, dtype=np.int64).astype(F) + F(0.5))[None, :].repeat(bh, 0)
    pyc = (np.arange(y0, y0 + bh, dtype=np.int64).astype(F) + F(0.5))[:, None].repeat(bw, 1)
    with np.errstate(all="ignore"):
        dx, dy = pxc - s["cx"], pyc - s["cy"]
        if perturb == "fma_rotate":
            lx = (dx.astype(np.float64) * np.float64(inv_cos) - (dy * inv_sin).astype(np.float64)).astype(F)   # fma(dx, c, -(dy * s))
        else:
            lx = dx * inv_cos - dy * inv_sin
        ly = dx * inv_sin + dy * inv_cos
        aa, ow = s["anti_alias"], rmax(s["outline_width"], F(0))
        d = shape_sdf(s["kind"], lx, ly, s["hw"], s["hh"], s["corner_radius"], lm)
        prim, sec = np.array(s["primary"], np.uint8), np.array(s["secondary"], np.uint8)
        color = np.empty((bh, bw, 4), np.uint8)
        if s["fill"] == "filled":
            cov = coverage_from_sdf(d, aa)
            color[:] = prim
        elif s["fill"] == "outline":
            cov = rclamp(coverage_from_sdf(d, aa) - coverage_from_sdf(d + ow, aa), 0, 1)
            color[:] = prim
        else:
            fill_cov = coverage_from_sdf(d, aa)
            oa = rclamp(fill_cov - coverage_from_sdf(d + ow, aa), 0, 1)
            fa = fill_cov * (F(1) - oa)
            total = oa + fa
            mixed = np.stack([as_u8((F(prim[c]) * oa + F(sec[c]) * fa) / total) for c in range(4)], -1)
            mixed[~(total > 0)] = 0
            has_outline = oa > F(0.001)
            color[:] = np.where(has_outline[..., None], mixed, sec)
            cov = np.where(has_outline, np.where(total > 0, total, F(0)), fill_cov).astype(F)
        av = color[..., 3].astype(F) * cov
        a = as_u8(av) if perturb == "trunc_alpha" else as_u8(rmin(round_away(av), F(255)))
        buf = np.zeros((bh, bw, 4), np.uint8)
        hit = cov > F(0.001)
        buf[hit, :3] = color[hit, :3]
        buf[hit, 3] = a[hit]
    return buf, box, lm.ambiguous


def to_canvas(buf, box, canvas_w, canvas_h):
    """rasterize_to_canvas (tests/visual_shapes.rs:18-41): box pixels with a > 0 pasted on a zeroed canvas"""
    canvas = np.zeros((canvas_h, canvas_w, 4), np.uint8)
    x0, y0, bw, bh = box
    if bw:
        view = canvas[y0:y0 + bh, x0:x0 + bw]
        put = buf[..., 3] > 0
        view[put] = buf[put]
    return canvas


def preview(s, canvas_w, canvas_h, flavour="glibc", perturb=None):
    buf, box, amb = rasterize(s, canvas_w, canvas_h, flavour, perturb)
    return to_canvas(buf, box, canvas_w, canvas_h), amb
