"""numpy-float32 restatement of the reference's custom path shapes (ref: src/ops/shapes.rs): custom_shape_coverage :1065, custom_shape_coverage_sample :1088,
point_in_polylines :1122, distance_to_polylines :1140, distance_to_segment :1152, the custom branch of rasterize_shape :1241-1248 with the gate and the alpha
quantisation :1293-1300, and render_custom_shape_icon :122-155.  Every f32 operation rounds once, in the reference's association order; the box, the rotation
and the preview's paste rule are tests/shape_model.py's.

Vectorised over the pixels of the box and over chunks of segments.  Two things are therefore not in the reference's order, both order-free: the parity is the
count of crossings mod 2 instead of a running toggle, and the minimum distance is taken chunk by chunk.  tests/test_customshape_model_host.py holds this file
to a scalar pixel loop that hoists and reorders nothing, and to hand-derived answers.

A path is a dict: `polylines` (a list of (n, 2) float32 arrays) and `bounds` (min_x, min_y, max_x, max_y)."""
import numpy as np

from .shape_model import F, F32_MAX, bounds as shape_bounds, cosf, rclamp, rmax, rmin, round_away, sinf, as_u8, to_canvas  # noqa: F401

CHUNK = 64
EPS = F(1e-6)


def path(polylines, bounds=None):
    """bounds default to the points' own extent (kurbo's bounding box of a polygonal path)"""
    polys = [np.asarray(p, F).reshape(-1, 2) for p in polylines]
    if bounds is None:
        pts = np.concatenate([p for p in polys if len(p)] or [np.zeros((1, 2), F)])
        bounds = (pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max())
    return dict(polylines=polys, bounds=tuple(F(b) for b in bounds))


def segments(p):
    """windows(2) of every polyline, in order: (n, 4) float32 rows x1 y1 x2 y2"""
    rows = [np.concatenate([q[:-1], q[1:]], 1) for q in p["polylines"] if len(q) >= 2]
    return np.concatenate(rows).astype(F) if rows else np.zeros((0, 4), F)


def point_in_polylines(px, py, segs):                            # :1122
    inside = np.zeros(px.shape, bool)
    pxc, pyc = px[:, None], py[:, None]
    for k in range(0, len(segs), CHUNK):
        x1, y1, x2, y2 = (segs[k:k + CHUNK, c][None, :] for c in range(4))
        denom = y2 - y1
        xi = (x2 - x1) * (pyc - y1) / denom + x1
        hit = (np.abs(denom) > EPS) & ((y1 > pyc) != (y2 > pyc)) & (pxc < xi)
        inside ^= (hit.sum(1) & 1).astype(bool)
    return inside


def distance_to_polylines(px, py, segs):                         # :1140, :1152
    best = np.full(px.shape, F32_MAX, F)
    pxc, pyc = px[:, None], py[:, None]
    for k in range(0, len(segs), CHUNK):
        ax, ay, bx, by = (segs[k:k + CHUNK, c][None, :] for c in range(4))
        dx, dy = bx - ax, by - ay
        len2 = dx * dx + dy * dy
        ex, ey = pxc - ax, pyc - ay
        to_point = np.sqrt(ex * ex + ey * ey)
        t = rclamp((ex * dx + ey * dy) / len2, 0, 1)
        cx, cy = ax + dx * t, ay + dy * t
        to_segment = np.sqrt((pxc - cx) * (pxc - cx) + (pyc - cy) * (pyc - cy))
        d = np.where(len2 <= EPS, to_point, to_segment).astype(F)
        best = rmin(best, np.fmin.reduce(d, axis=1))             # f32::min: a NaN distance leaves best as it is
    return best


def scales(p, hx, hy):                                           # :1097-1101
    min_x, min_y, max_x, max_y = p["bounds"]
    bw, bh = rmax(max_x - min_x, F(1)), rmax(max_y - min_y, F(1))
    return bw / rmax(hx * F(2), F(1)), bh / rmax(hy * F(2), F(1))


def coverage_sample(p, segs, lx, ly, hx, hy, outline_width, fill):   # :1088; lx, ly: 1-D float32; returns bool
    sx, sy = scales(p, hx, hy)
    px = (lx + hx) * sx + p["bounds"][0]
    py = (ly + hy) * sy + p["bounds"][1]
    inside = point_in_polylines(px, py, segs)
    if fill == "filled":
        return inside
    edge_dist = distance_to_polylines(px, py, segs) / rmax(sx, sy)
    outline = edge_dist <= rmax(outline_width, F(1))
    return outline if fill == "outline" else (inside | outline)


def coverage(p, segs, lx, ly, hx, hy, outline_width, fill):      # :1065
    total = np.zeros(lx.shape, F)
    for ox, oy in ((F(-0.25), F(-0.25)), (F(0.25), F(-0.25)), (F(-0.25), F(0.25)), (F(0.25), F(0.25))):
        total = total + coverage_sample(p, segs, lx + ox, ly + oy, hx, hy, outline_width, fill).astype(F)
    return total * F(0.25)


def local_frame(s, box):
    """lx, ly of every pixel centre of the box (rasterize_shape :1231-1239), flattened row-major"""
    x0, y0, bw, bh = box
    cos_r, sin_r = cosf(s["rotation"]), sinf(s["rotation"])
    inv_cos, inv_sin = cos_r, -sin_r
    pxc = (np.arange(x0, x0 + bw, dtype=np.int64).astype(F) + F(0.5))[None, :].repeat(bh, 0)
    pyc = (np.arange(y0, y0 + bh, dtype=np.int64).astype(F) + F(0.5))[:, None].repeat(bw, 1)
    dx, dy = pxc - s["cx"], pyc - s["cy"]
    return (dx * inv_cos - dy * inv_sin).ravel(), (dx * inv_sin + dy * inv_cos).ravel()


def quantise(primary, cov):
    """:1293-1300 for a (n,) coverage: (n, 4) uint8"""
    out = np.zeros(cov.shape + (4,), np.uint8)
    hit = cov > F(0.001)
    out[hit, :3] = np.array(primary[:3], np.uint8)
    out[hit, 3] = as_u8(rmin(round_away(F(primary[3]) * cov), F(255)))[hit]
    return out


def rasterize(s, p, canvas_w, canvas_h):
    """rasterize_shape's `buf` with custom_shape_data = p: ((bh, bw, 4) uint8, (x0, y0, bw, bh)).  s is a tests/shape_model.py shape dict: its kind only
    shapes the box, its secondary colour, anti_alias and corner_radius are not read"""
    x0, y0, bw, bh = box = shape_bounds(s, canvas_w, canvas_h)
    if bw == 0:
        return np.zeros((0, 0, 4), np.uint8), box
    with np.errstate(all="ignore"):
        lx, ly = local_frame(s, box)
        cov = coverage(p, segments(p), lx, ly, s["hw"], s["hh"], rmax(s["outline_width"], F(0)), s["fill"])
        return quantise(s["primary"], cov).reshape(bh, bw, 4), box


def preview(s, p, canvas_w, canvas_h):
    buf, box = rasterize(s, p, canvas_w, canvas_h)
    return to_canvas(buf, box, canvas_w, canvas_h)


def icon(p, size, dark):                                         # :122-155
    fg = 235 if dark else 30
    segs = segments(p)
    ys, xs = np.mgrid[0:size, 0:size]
    x, y, fsize = xs.ravel().astype(F), ys.ravel().astype(F), F(size)
    cov = np.zeros(x.shape, F)
    with np.errstate(all="ignore"):
        for sy in range(4):
            for sx in range(4):
                lx = (x + (F(sx) + F(0.5)) * F(0.25)) / fsize * F(2) - F(1)
                ly = (y + (F(sy) + F(0.5)) * F(0.25)) / fsize * F(2) - F(1)
                cov = cov + coverage_sample(p, segs, lx, ly, F(0.82), F(0.82), F(0.04), "filled").astype(F)
        cov = rclamp(cov / F(16), 0, 1)
        out = np.zeros((size * size, 4), np.uint8)
        hit = cov > 0
        out[hit, :3] = fg
        out[hit, 3] = as_u8(round_away(F(255) * cov))[hit]
    return out.reshape(size, size, 4)
