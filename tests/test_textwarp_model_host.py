"""tests/textwarp_model.py held three ways, since the reference has no test of its text warps and the model is the device kernels' only yardstick:

1. a second transcription: `Scalar` below restates warp.rs and rotate_glyph_buffer pixel by pixel, with plain loops and np.float32 scalars, bounds loops
   included; the vectorised model equals it exactly on every kind at a small size;
2. answers derived by hand: the identity rules, the envelope between the straight edges of a 64 x 32 source, a path of coincident points, the blit's rule;
3. each case of tests/textwarp_cases.py samples at least its stated number of pixels, and each planted defect changes at least one case.

It also holds the glibc and device flavours of every arc and circular case within the LIBM class (+-1 on fewer than 0.1 % of channels) before any GPU run, and
the library's host-only plan calls to the model's plans and to the header's refusals.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from . import textwarp_cases as TC
from . import textwarp_model as M
from .libm_checks import LIBM, check_glibc
from .shape_model import _m as libm_so

F = np.float32
F32_MAX = F(3.4028234663852886e38)
PI, TAU = F(math.pi), F(2 * math.pi)


def sinf(x):
    return F(libm_so.sinf(float(x)))


def cosf(x):
    return F(libm_so.cosf(float(x)))


def atan2f(y, x):
    return F(libm_so.atan2f(float(y), float(x)))


def fmin(a, b):     # f32::min
    return b if a != a else (a if b != b else (a if a < b else b))


def fmax(a, b):
    return b if a != a else (a if b != b else (a if a > b else b))


def as_u32(v):
    v = float(v)
    return 0 if v != v else int(max(min(v, 4294967295.0), 0.0))


def as_i32(v):
    v = float(v)
    return 0 if v != v else int(max(min(v, 2147483647.0), -2147483648.0))


def rs_round(v):    # f32::round
    t = F(np.trunc(v))
    return F(t + F(math.copysign(1.0, float(v)))) if abs(F(v - t)) >= F(0.5) else t


class Scalar:
    """warp.rs and rotate_glyph_buffer line by line; every value is an np.float32 scalar"""

    @staticmethod
    def bilinear_sample(src, x, y):   # :707-740
        h, w = src.shape[:2]
        x0, y0 = int(np.floor(x)), int(np.floor(y))
        fx, fy = F(x - F(x0)), F(y - F(y0))

        def sample(sx, sy):
            if sx < 0 or sy < 0 or sx >= w or sy >= h:
                return [F(0)] * 4
            return [F(v) for v in src[sy, sx]]
        p00, p10, p01, p11 = sample(x0, y0), sample(x0 + 1, y0), sample(x0, y0 + 1), sample(x0 + 1, y0 + 1)
        out = []
        for c in range(4):
            v = p00[c] * (F(1) - fx) * (F(1) - fy) + p10[c] * fx * (F(1) - fy) + p01[c] * (F(1) - fx) * fy + p11[c] * fx * fy
            out.append(int(min(max(float(rs_round(v)), 0.0), 255.0)))
        return out

    @staticmethod
    def eval_cubic_bezier(pts, t):   # :546-559
        u = F(1) - t
        u2, t2 = u * u, t * t
        x = u2 * u * pts[0][0] + F(3) * u2 * t * pts[1][0] + F(3) * u * t2 * pts[2][0] + t2 * t * pts[3][0]
        y = u2 * u * pts[0][1] + F(3) * u2 * t * pts[1][1] + F(3) * u * t2 * pts[2][1] + t2 * t * pts[3][1]
        return x, y

    @staticmethod
    def eval_cubic_bezier_tangent(pts, t):   # :562-571
        u = F(1) - t
        dx = F(3) * u * u * (pts[1][0] - pts[0][0]) + F(6) * u * t * (pts[2][0] - pts[1][0]) + F(3) * t * t * (pts[3][0] - pts[2][0])
        dy = F(3) * u * u * (pts[1][1] - pts[0][1]) + F(6) * u * t * (pts[2][1] - pts[1][1]) + F(3) * t * t * (pts[3][1] - pts[2][1])
        return dx, dy

    @staticmethod
    def finish(out_w, out_h, min_x, min_y, src, mapper):
        """the warps' shared tail: the pixel loop over an inverse map that returns None or (sx, sy)"""
        h, w = src.shape[:2]
        out = np.zeros((out_h, out_w, 4), np.uint8)
        for oy in range(out_h):
            for ox in range(out_w):
                got = mapper(ox, oy)
                if got is not None:
                    sx, sy = got
                    if sx >= F(0) and sx < F(w) and sy >= F(0) and sy < F(h):
                        out[oy, ox] = Scalar.bilinear_sample(src, sx, sy)
        return out, as_i32(np.floor(min_x)), as_i32(np.floor(min_y))

    @staticmethod
    def arc(src, bend, hdist, vdist):   # :97-179
        bend, hdist, vdist = F(bend), F(hdist), F(vdist)
        if abs(bend) < F(0.001):
            return src.copy(), 0, 0
        w, h = F(src.shape[1]), F(src.shape[0])
        angle = bend * PI
        radius = w / (F(2) * sinf(angle / F(2))) if abs(angle) > F(0.01) else w * F(100)

        def map_point(sx, sy):   # :182-219
            cx = w / F(2)
            t = (sx - cx) / (w / F(2))
            theta = t * angle / F(2)
            r_sign = F(1) if angle > F(0) else F(-1)
            r_abs = abs(radius)
            r = r_abs - (F(1) - sy / h) * h * r_sign
            dx = cx + r * sinf(theta)
            dy = r_abs - r * cosf(theta) * r_sign
            return dx + (dx - cx) * hdist, dy + (dy - h / F(2)) * vdist

        def inverse(dx, dy):     # :222-274
            cx = w / F(2)
            r_sign = F(1) if angle > F(0) else F(-1)
            r_abs = abs(radius)
            if abs(hdist) > F(0.001):
                dx = cx + (dx - cx) / (F(1) + hdist)
            if abs(vdist) > F(0.001):
                dy = h / F(2) + (dy - h / F(2)) / (F(1) + vdist)
            rel_x = dx - cx
            rel_y = r_abs - dy * r_sign
            r = np.sqrt(rel_x * rel_x + (rel_y * r_sign) * (rel_y * r_sign))
            theta = atan2f(rel_x, rel_y * r_sign)
            if abs(angle) > F(0.01) and abs(theta) > abs(angle / F(2)) + F(0.1):
                return None
            t = theta / (angle / F(2)) if abs(angle) > F(0.01) else (dx - cx) / (w / F(2))
            sx = cx + t * w / F(2)
            sy_norm = F(1) - (r_abs - r) / (h * r_sign)
            return sx, sy_norm * h
        min_x, max_x, min_y, max_y = F32_MAX, -F32_MAX, F32_MAX, -F32_MAX
        for i in range(33):
            sx = (F(i) / F(32)) * w
            for sy in (F(0), h):
                dx, dy = map_point(sx, sy)
                min_x, max_x, min_y, max_y = fmin(min_x, dx), fmax(max_x, dx), fmin(min_y, dy), fmax(max_y, dy)
        min_x, min_y, max_x, max_y = min_x - F(2), min_y - F(2), max_x + F(2), max_y + F(2)
        out_w, out_h = as_u32(np.ceil(max_x - min_x)), as_u32(np.ceil(max_y - min_y))
        if out_w == 0 or out_h == 0 or out_w > 8192 or out_h > 8192:
            return src.copy(), 0, 0
        return Scalar.finish(out_w, out_h, min_x, min_y, src, lambda ox, oy: inverse(F(ox) + min_x, F(oy) + min_y))

    @staticmethod
    def circular(src, radius, start_angle, clockwise):   # :277-352
        w, h = F(src.shape[1]), F(src.shape[0])
        r = fmax(F(radius), F(10))
        start_angle = F(start_angle)
        direction = F(1) if clockwise else F(-1)
        r_outer = r + h
        out_size = as_u32(np.ceil(r_outer * F(2) + F(4)))
        out_c = F(out_size) / F(2)
        off_x, off_y = as_i32(rs_round(w / F(2) - out_c)), as_i32(rs_round(h / F(2) - out_c))
        out = np.zeros((out_size, out_size, 4), np.uint8)
        for oy in range(out_size):
            for ox in range(out_size):
                px, py = F(ox) - out_c, F(oy) - out_c
                dist = np.sqrt(px * px + py * py)
                if dist < r or dist > r_outer:
                    continue
                rel_angle = (atan2f(py, px) - start_angle) * direction
                while rel_angle < F(0):
                    rel_angle = rel_angle + TAU
                while rel_angle >= TAU:
                    rel_angle = rel_angle - TAU
                sx = rel_angle * r
                if sx < F(0) or sx >= w:
                    continue
                sy = r_outer - dist
                if sy < F(0) or sy >= h:
                    continue
                out[oy, ox] = Scalar.bilinear_sample(src, sx, sy)
        return out, off_x, off_y

    @staticmethod
    def path(src, points):   # :355-444
        if len(points) < 4:
            return src.copy(), 0, 0
        pts = [(F(p[0]), F(p[1])) for p in points[:4]]
        w, h = F(src.shape[1]), F(src.shape[0])
        bez, tan = Scalar.eval_cubic_bezier, Scalar.eval_cubic_bezier_tangent
        lengths, total = [F(0)], F(0)            # build_arc_length_table :575-591
        prev_x, prev_y = bez(pts, F(0))
        for i in range(1, 257):
            x, y = bez(pts, F(i) / F(256))
            dx, dy = x - prev_x, y - prev_y
            total = total + np.sqrt(dx * dx + dy * dy)
            lengths.append(total)
            prev_x, prev_y = x, y

        def arc_length_to_t(s):                  # :594-623
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

        def inverse(px, py):                     # :627-695
            best_t, best_dist_sq = F(0), F32_MAX
            for i in range(65):
                t = F(i) / F(64)
                cx, cy = bez(pts, t)
                dist_sq = (px - cx) * (px - cx) + (py - cy) * (py - cy)
                if dist_sq < best_dist_sq:
                    best_dist_sq, best_t = dist_sq, t
            step = F(1) / F(64)
            t_lo, t_hi = fmax(best_t - step, F(0)), fmin(best_t + step, F(1))
            for _ in range(8):
                t_mid = (t_lo + t_hi) / F(2)
                t_a, t_b = (t_lo + t_mid) / F(2), (t_mid + t_hi) / F(2)
                ax, ay = bez(pts, t_a)
                bx, by = bez(pts, t_b)
                da = (px - ax) * (px - ax) + (py - ay) * (py - ay)
                db = (px - bx) * (px - bx) + (py - by) * (py - by)
                if da < db:
                    t_hi = t_mid
                else:
                    t_lo = t_mid
            t = (t_lo + t_hi) / F(2)
            cx, cy = bez(pts, t)
            tx, ty = tan(pts, t)
            tangent_len = np.sqrt(tx * tx + ty * ty)
            if tangent_len < F(0.0001):
                return None
            nx, ny = -ty / tangent_len, tx / tangent_len
            perp_dist = (px - cx) * nx + (py - cy) * ny
            n = len(lengths) - 1                 # arc_length_to_t_inverse :698-704
            idx_f = t * F(n)
            idx = min(int(idx_f), n - 1)
            sx = lengths[idx] + (idx_f - F(idx)) * (lengths[idx + 1] - lengths[idx])
            return sx, h / F(2) - perp_dist
        min_x, max_x, min_y, max_y = F32_MAX, -F32_MAX, F32_MAX, -F32_MAX
        for i in range(65):
            t = arc_length_to_t((F(i) / F(64)) * total)
            px, py = bez(pts, t)
            _, ny = tan(pts, t)
            for offset in (-h, F(0), h):
                min_x, max_x = fmin(min_x, px - abs(offset)), fmax(max_x, px + abs(offset))
                min_y, max_y = fmin(min_y, py + offset + abs(ny) * h), fmax(max_y, py - offset - abs(ny) * h)
        margin = h + F(10)
        min_x, min_y, max_x, max_y = min_x - margin, min_y - margin, max_x + margin, max_y + margin
        out_w, out_h = min(as_u32(np.ceil(max_x - min_x)), 4096), min(as_u32(np.ceil(max_y - min_y)), 4096)
        if out_w == 0 or out_h == 0:
            return src.copy(), 0, 0
        return Scalar.finish(out_w, out_h, min_x, min_y, src, lambda ox, oy: inverse(F(ox) + min_x, F(oy) + min_y))

    @staticmethod
    def envelope(src, top, bottom):   # :447-539
        if len(top) < 4 or len(bottom) < 4:
            return src.copy(), 0, 0
        top, bottom = [(F(p[0]), F(p[1])) for p in top[:4]], [(F(p[0]), F(p[1])) for p in bottom[:4]]
        w, h = F(src.shape[1]), F(src.shape[0])
        bez = Scalar.eval_cubic_bezier
        min_x, max_x, min_y, max_y = F32_MAX, -F32_MAX, F32_MAX, -F32_MAX
        for i in range(65):
            t = F(i) / F(64)
            (tx, ty), (bx, by) = bez(top, t), bez(bottom, t)
            min_x, max_x = fmin(fmin(min_x, tx), bx), fmax(fmax(max_x, tx), bx)
            min_y, max_y = fmin(fmin(min_y, ty), by), fmax(fmax(max_y, ty), by)
        margin = F(4)
        min_x, min_y, max_x, max_y = min_x - margin, min_y - margin, max_x + margin, max_y + margin
        out_w, out_h = min(as_u32(np.ceil(max_x - min_x)), 4096), min(as_u32(np.ceil(max_y - min_y)), 4096)
        if out_w == 0 or out_h == 0:
            return src.copy(), 0, 0

        def mapper(ox, oy):
            px, py = F(ox) + min_x, F(oy) + min_y
            t = (px - min_x) / fmax(max_x - min_x - F(2) * margin, F(1))
            if not (F(0) <= t <= F(1)):
                return None
            _, top_y = bez(top, t)
            _, bot_y = bez(bottom, t)
            span = bot_y - top_y
            if abs(span) < F(0.001):
                return None
            v = (py - top_y) / span
            if not (F(0) <= v <= F(1)):
                return None
            return t * w, v * h
        return Scalar.finish(out_w, out_h, min_x, min_y, src, mapper)

    @staticmethod
    def rotate(buf, angle, pivot):   # raster.rs:561-653
        angle = F(angle)
        h, w = buf.shape[:2]
        cos_a, sin_a, fw, fh = cosf(angle), sinf(angle), F(w), F(h)
        cx, cy = (F(pivot[0]), F(pivot[1])) if pivot is not None else (fw * F(0.5), fh * F(0.5))
        min_x, max_x, min_y, max_y = F32_MAX, -F32_MAX, F32_MAX, -F32_MAX
        for px, py in ((F(0), F(0)), (fw, F(0)), (F(0), fh), (fw, fh)):
            dx, dy = px - cx, py - cy
            rx, ry = dx * cos_a - dy * sin_a + cx, dx * sin_a + dy * cos_a + cy
            min_x, min_y, max_x, max_y = fmin(min_x, rx), fmin(min_y, ry), fmax(max_x, rx), fmax(max_y, ry)
        new_w, new_h = as_u32(np.ceil(max_x - min_x)) + 1, as_u32(np.ceil(max_y - min_y)) + 1
        new_cx, new_cy = cx - np.floor(min_x), cy - np.floor(min_y)
        out = np.zeros((new_h, new_w, 4), np.uint8)
        for oy in range(new_h):
            for ox in range(new_w):
                dx, dy = F(ox) - new_cx, F(oy) - new_cy
                sx = dx * cos_a + dy * sin_a + cx
                sy = -dx * sin_a + dy * cos_a + cy
                if sx >= F(0) and sx < fw and sy >= F(0) and sy < fh:
                    sx0, sy0 = int(np.floor(sx)), int(np.floor(sy))
                    sx1, sy1 = min(sx0 + 1, w - 1), min(sy0 + 1, h - 1)
                    fx, fy = sx - F(sx0), sy - F(sy0)
                    for c in range(4):
                        p00, p10, p01, p11 = F(buf[sy0, sx0, c]), F(buf[sy0, sx1, c]), F(buf[sy1, sx0, c]), F(buf[sy1, sx1, c])
                        val = p00 * (F(1) - fx) * (F(1) - fy) + p10 * fx * (F(1) - fy) + p01 * (F(1) - fx) * fy + p11 * fx * fy
                        out[oy, ox, c] = int(min(max(float(rs_round(val)), 0.0), 255.0))
        return out, as_i32(np.floor(min_x)), as_i32(np.floor(min_y))

    @staticmethod
    def warp(src, warp):
        f = M.DEFAULTS | warp
        with np.errstate(all="ignore"):
            if warp["kind"] == "arc":
                return Scalar.arc(src, f["bend"], f["horizontal_distortion"], f["vertical_distortion"])
            if warp["kind"] == "circular":
                return Scalar.circular(src, f["radius"], f["start_angle"], f["clockwise"])
            if warp["kind"] == "path":
                return Scalar.path(src, f["control_points"])
            return Scalar.envelope(src, f["top_curve"], f["bottom_curve"])


# ---- 1. the second transcription ---------------------------------------------------------------------------------------------------------------------------------------
SMALL = (23, 9)
SMALL_WARPS = {
    "arc": dict(kind="arc", bend=0.5),
    "arc_1.0_distorted": dict(kind="arc", bend=1.0, horizontal_distortion=0.3, vertical_distortion=-0.2),
    "arc_negative": dict(kind="arc", bend=-0.5),
    "arc_flat_radius": dict(kind="arc", bend=0.002),
    "arc_hdist_-1": dict(kind="arc", bend=0.5, horizontal_distortion=-1.0),
    "circle_cw": dict(kind="circular", radius=12.0),
    "circle_ccw_start_2": dict(kind="circular", radius=5.0, clockwise=False, start_angle=2.0),
    "circle_start_-8pi": dict(kind="circular", radius=12.0, start_angle=-TC.EIGHT_PI),
    "path": dict(kind="path", control_points=[(0.0, 0.0), (8.0, -6.0), (16.0, -6.0), (24.0, 0.0)]),
    "path_crossing": dict(kind="path", control_points=[(0.0, 0.0), (30.0, 20.0), (-10.0, 20.0), (20.0, 0.0)]),
    "path_coincident": dict(kind="path", control_points=[(5.0, 5.0)] * 4),
    "envelope": dict(kind="envelope", top_curve=[(0.0, -4.0), (10.0, -8.0), (20.0, -8.0), (30.0, -4.0)],
                     bottom_curve=[(0.0, 4.0), (10.0, 8.0), (20.0, 8.0), (30.0, 4.0)]),
    "envelope_crossing": dict(kind="envelope", top_curve=[(0.0, -6.0), (10.0, -6.0), (20.0, 6.0), (30.0, 6.0)],
                              bottom_curve=[(0.0, 6.0), (10.0, 6.0), (20.0, -6.0), (30.0, -6.0)]),
}


@pytest.mark.parametrize("name", list(SMALL_WARPS))
def test_the_vectorised_model_equals_the_pixel_loop_transcription(name):
    src = TC.source(SMALL)
    want, off_x, off_y = Scalar.warp(src, SMALL_WARPS[name])
    got, plan, _ = M.apply_warp(src, SMALL_WARPS[name])
    assert got.shape == want.shape and (plan["off_x"], plan["off_y"]) == (off_x, off_y)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())


@pytest.mark.parametrize("angle,pivot", [(0.3, None), (-0.3, None), (0.3, (3.5, 11.25)), (float(F(math.pi / 2)), None)])
def test_the_vectorised_rotation_equals_the_pixel_loop_transcription(angle, pivot):
    src = TC.source(SMALL)
    want, off_x, off_y = Scalar.rotate(src, angle, pivot)
    got, plan = M.rotate(src, angle, pivot)
    assert got.shape == want.shape and (plan["off_x"], plan["off_y"]) == (off_x, off_y)
    assert np.array_equal(got, want) and got[..., 3].any()


# ---- 2. known answers ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.IDENTITIES)
def test_identity_rules(name):
    """|bend| < 0.001, arc bounds above 8192, fewer than four points, kind none: the source comes back at offset 0, 0"""
    size, _, _ = TC.WARPS[name]
    out, plan, _, _ = TC.expected_warp(name)
    assert plan["identity"] and (plan["out_w"], plan["out_h"], plan["off_x"], plan["off_y"]) == (size[0], size[1], 0, 0)
    assert np.array_equal(out, TC.source(size))


def test_the_identity_gate_of_the_arc_has_two_sides():
    assert TC.expected_warp("arc_0.0009_identity")[1]["identity"] and not TC.expected_warp("arc_0.0011")[1]["identity"]
    assert not M.rotate_plan(131, 37, 0.0011)["identity"] and M.rotate_plan(131, 37, 0.001)["identity"] and M.rotate_plan(131, 37, -0.001)["identity"]


def test_envelope_between_the_straight_edges_of_the_source():
    """t = ox / 64 and v = (oy - 4) / 32 are exact, the curves' y are exactly 0 and 32 (every term of the Bézier sum is a multiple of 2^-18 * 32 below 2^24
    of them), so sx = ox, sy = oy - 4 and the gather returns the source pixel itself"""
    src = TC.source(TC.POW2)
    out, plan, painted, _ = TC.expected_warp("envelope_rectangle")
    assert (plan["out_w"], plan["out_h"], plan["off_x"], plan["off_y"]) == (72, 40, -4, -4) and painted == 64 * 32
    want = np.zeros((40, 72, 4), np.uint8)
    want[4:36, :64] = src
    assert np.array_equal(out, want)


@pytest.mark.parametrize("name", TC.PAINT_NOTHING)
def test_cases_the_reference_leaves_empty(name):
    out, plan, painted, _ = TC.expected_warp(name)
    assert not plan["identity"] and painted == 0 and not out.any()


def test_blit_keeps_the_canvas_under_alpha_zero_and_replaces_elsewhere():
    canvas = np.full((4, 5, 4), 9, np.uint8)
    buf = np.zeros((2, 3, 4), np.uint8)
    buf[0, 0] = (1, 2, 3, 0)      # alpha 0 with colour: kept out
    buf[0, 1] = (4, 5, 6, 1)      # the faintest alpha replaces, it does not blend
    buf[1, 2] = (7, 8, 9, 255)
    got = M.blit(canvas.copy(), buf, 3, 3)   # column 2 and row 1 of the buffer hang off the canvas
    want = canvas.copy()
    want[3, 4] = (4, 5, 6, 1)
    assert np.array_equal(got, want)
    assert np.array_equal(M.blit(canvas.copy(), buf, 5, 0), canvas) and np.array_equal(M.blit(canvas.copy(), buf, 0, -2), canvas)   # wholly outside
    got = M.blit(canvas.copy(), buf, -2, -1)   # only buf[1, 2] lands, at the canvas's corner
    want = canvas.copy()
    want[0, 0] = (7, 8, 9, 255)
    assert np.array_equal(got, want)


def test_blit_minus_one_lands_the_opaque_corner():
    canvas = np.zeros((3, 3, 4), np.uint8)
    buf = np.zeros((2, 3, 4), np.uint8)
    buf[1, 2] = (7, 8, 9, 255)
    got = M.blit(canvas.copy(), buf, -1, -1)
    assert tuple(got[0, 1]) == (7, 8, 9, 255) and int(got.any(-1).sum()) == 1


# ---- 3. the cases draw what they are named after; the planted defects show --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.WARPS))
def test_each_warp_case_samples_its_floor(name):
    size, _, floor = TC.WARPS[name]
    out, plan, painted, _ = TC.expected_warp(name)
    print(f"{name}: {plan['out_w']} x {plan['out_h']}, {painted} sampled, floor {floor}")
    assert painted >= floor and out.shape == (plan["out_h"], plan["out_w"], 4)
    if floor:
        assert int((out[..., 3] > 0).sum()) >= floor // 2 and not plan["identity"]
    else:
        assert name in TC.IDENTITIES + TC.PAINT_NOTHING


def test_the_clamped_path_is_clamped_and_the_loops_of_the_circle_run():
    assert TC.expected_warp("path_clamped_4096")[1]["out_w"] == 4096
    assert float(TC.expected_warp("path_clamped_4096")[1]["max_x"] - TC.expected_warp("path_clamped_4096")[1]["min_x"]) > 4096
    # 8 pi and -8 pi turn the text by whole circles: the picture of start 0 read through several steps of either loop, up to the rounding of the additions
    zero = M.apply_warp(TC.source(TC.MEASURED), dict(kind="circular", radius=40.0, start_angle=0.0))[0]
    turned = TC.expected_warp("circle_start_8pi")[0]
    assert turned.shape == zero.shape and (turned != zero).any(-1).mean() < 0.05 and turned.any()


@pytest.mark.parametrize("name", list(TC.ROTATIONS))
def test_each_rotation_keeps_its_pixels(name):
    size, angle, _ = TC.ROTATIONS[name]
    out, plan = TC.expected_rotation(name)
    if name == "rotate_0.001_skipped":
        assert plan["identity"] and np.array_equal(out, TC.source(size))
    elif size == TC.DOT:
        assert out.shape == (3, 3, 4)   # one source pixel: the rotated centre misses every pixel centre or hits one
    else:
        assert int((out[..., 3] > 0).sum()) >= (size[0] * size[1]) // 2


def test_a_quarter_turn_moves_rows_to_columns():
    out, plan = TC.expected_rotation("rotate_quarter_turn")
    assert (plan["out_w"], plan["out_h"]) == (33, 65)


@pytest.mark.parametrize("name", list(TC.PLACEMENTS))
def test_each_placement_changes_the_canvas_where_it_should(name):
    canvas, _ = TC.expected_placement(name)
    changed = int((canvas != TC.start_canvas(name)).any(-1).sum())
    print(f"{name}: {changed} canvas pixels changed")
    if name == "outside":
        assert changed == 0
    else:
        assert changed >= 1000
    if name.startswith("off_the"):   # the block reaches the edge it hangs off
        edge = dict(off_the_left=canvas[:, 0], off_the_top=canvas[0], off_the_right=canvas[:, -1], off_the_bottom=canvas[-1])[name]
        assert edge.any()


def test_the_later_block_is_on_top():
    both, _ = TC.expected_placement("two_blocks")
    (size_a, warp_a, off_a, rot_a, piv_a), (size_b, warp_b, off_b, rot_b, piv_b) = TC.PLACEMENTS["two_blocks"][1]
    only_b = M.place(np.zeros_like(both), TC.source(size_b), warp_b, off_b, rot_b, piv_b)
    only_a = M.place(np.zeros_like(both), TC.source(size_a), warp_a, off_a, rot_a, piv_a)
    overlap = (only_a[..., 3] > 0) & (only_b[..., 3] > 0)
    assert overlap.sum() > 100 and np.array_equal(both[overlap], only_b[overlap])


DEFECT_KINDS = {"bilinear_lerp": None, "bilinear_clamp": None, "coarse_le": "path", "fmod": "circular", "envelope_t": "envelope"}   # None: every kind gathers


@pytest.mark.parametrize("perturb", M.PERTURBATIONS)
def test_each_planted_defect_changes_a_case(perturb):
    """searched over every case the defect's code runs in, not shown on a chosen one"""
    kind = DEFECT_KINDS[perturb]
    names = [n for n, (_, warp, floor) in TC.WARPS.items() if floor and (kind is None or warp["kind"] == kind)]
    changed = {}
    for name in names:
        good, bad = TC.expected_warp(name)[0], TC.expected_warp(name, "glibc", perturb)[0]
        n = int((good != bad).any(-1).sum()) if good.shape == bad.shape else -1
        if n:
            changed[name] = n
    print(f"{perturb}: changes {len(changed)} of {len(names)} cases: {changed}")
    assert changed


# ---- the two libm flavours ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.LIBM_WARPS)
def test_glibc_and_device_flavours_stay_within_the_libm_class(name):
    glibc, device = TC.expected_warp(name, "glibc"), TC.expected_warp(name, "device")
    d = np.abs(glibc[0].astype(np.int16) - device[0].astype(np.int16))
    print(f"{name}: {int((d > 0).sum())} of {d.size} channels differ, max {int(d.max()) if d.size else 0}, {device[3]} ambiguous calls")
    assert glibc[0].shape == device[0].shape
    check_glibc(device[0], glibc[0], LIBM, name)


# ---- the library's host-only calls --------------------------------------------------------------------------------------------------------------------------------------
def geom_tuple(g):
    return g.out_w, g.out_h, g.off_x, g.off_y, bool(g.identity)


@pytest.mark.parametrize("name", list(TC.WARPS))
def test_the_library_plans_what_the_model_plans(name):
    import paintfe_amd as P
    size, warp, _ = TC.WARPS[name]
    plan = TC.expected_warp(name)[1]
    g = P.text_warp_plan(P.text_warp(size, **warp))
    assert geom_tuple(g) == (plan["out_w"], plan["out_h"], plan["off_x"], plan["off_y"], plan["identity"])
    assert (F(g.min_x), F(g.min_y), F(g.max_x), F(g.max_y)) == (plan["min_x"], plan["min_y"], plan["max_x"], plan["max_y"])


@pytest.mark.parametrize("name", list(TC.ROTATIONS))
def test_the_library_plans_the_rotation_the_model_plans(name):
    import paintfe_amd as P
    size, angle, pivot = TC.ROTATIONS[name]
    plan = TC.expected_rotation(name)[1]
    g = P.text_rotate_plan(size[0], size[1], angle, pivot)
    assert geom_tuple(g) == (plan["out_w"], plan["out_h"], plan["off_x"], plan["off_y"], plan["identity"])


def test_the_plan_calls_refuse_what_the_header_lists():
    import paintfe_amd as P
    from paintfe_amd import _lib
    lib = _lib.load()
    g = _lib.TextWarpGeom(7, 7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
    untouched = bytes(g)

    def status(warp):
        return lib.pfx_text_warp_plan(C.byref(warp) if warp is not None else None, C.byref(g))
    ok = lambda **kw: P.text_warp(TC.MEASURED, **kw)   # noqa: E731
    assert status(None) == _lib.ERR_INVALID and lib.pfx_text_warp_plan(C.byref(ok(kind="arc")), None) == _lib.ERR_INVALID
    for kind in (-1, 5, 1 << 20):
        assert status(ok(kind=kind)) == _lib.ERR_INVALID
    for size in ((0, 5), (5, 0)):
        assert status(P.text_warp(size, kind="arc")) == _lib.ERR_INVALID
    for field in ("arc_bend", "arc_hdist", "arc_vdist", "circ_radius", "circ_start_angle"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            w = ok(kind="none")      # whatever the kind says
            setattr(w, field, bad)
            assert status(w) == _lib.ERR_INVALID, field
    for field in ("path", "top", "bottom"):
        for i in range(4):
            for k in range(2):
                w = ok(kind="arc")
                getattr(w, field)[i][k] = float("nan")
                assert status(w) == _lib.ERR_INVALID, (field, i, k)
    assert status(ok(kind="circular", start_angle=TC.BEYOND_EIGHT_PI)) == _lib.ERR_UNSUPPORTED
    assert status(ok(kind="arc", start_angle=-TC.BEYOND_EIGHT_PI)) == _lib.ERR_UNSUPPORTED
    assert status(P.text_warp((20000, 20000), kind="arc")) == _lib.ERR_UNSUPPORTED            # the source over the document limit
    assert status(P.text_warp((64, 9000), kind="circular", radius=10.0)) == _lib.ERR_UNSUPPORTED   # 18 024 squared: the planned output over it
    assert bytes(g) == untouched
    assert status(ok(kind="circular", start_angle=TC.EIGHT_PI)) == _lib.OK and status(ok(kind="circular", start_angle=-TC.EIGHT_PI)) == _lib.OK
    # the rotation
    piv = (C.c_float * 2)(1.0, 2.0)
    g = _lib.TextWarpGeom(7, 7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
    rot = lambda w, h, a, p: lib.pfx_text_rotate_plan(C.c_uint32(w), C.c_uint32(h), C.c_float(a), p, C.byref(g))   # noqa: E731
    assert rot(0, 5, 0.3, None) == _lib.ERR_INVALID and rot(5, 0, 0.3, None) == _lib.ERR_INVALID and rot(5, 5, float("nan"), None) == _lib.ERR_INVALID
    assert rot(5, 5, 0.3, (C.c_float * 2)(float("inf"), 0.0)) == _lib.ERR_INVALID and rot(20000, 20000, 0.3, None) == _lib.ERR_UNSUPPORTED
    assert rot(16000, 16000, 0.7, None) == _lib.ERR_UNSUPPORTED                               # the rotated frame over the document limit
    assert lib.pfx_text_rotate_plan(C.c_uint32(5), C.c_uint32(5), C.c_float(0.3), None, None) == _lib.ERR_INVALID
    assert bytes(g) == untouched
    assert rot(5, 5, 0.3, piv) == _lib.OK and g.out_w > 5
