"""numpy-float32 restatement of the reference's dab-list tools (ref: src/ui/panels/tools/behavior/raster/clone_heal.rs): clone_stamp_circle :6-98,
clone_stamp_line :101-132, heal_circle :141-259, heal_line :262-292, draw_pixel_and_get_bounds :295-367, draw_pixel_line_and_get_bounds :370-431, and
compute_brush_alpha (brush_render.rs:54-82).  Dab after dab in stroke order, exactly the reference's loop, vectorised over a dab's box; every f32 operation
rounds once, in the reference's association order.

The heal brush's ring colour of a pixel is a function of (x, y, sample_radius, layer) alone, and the model calls libm per element, so `Ring` evaluates it once
per pixel and caches it.  tests/test_dabtools_model_host.py holds the whole model to a scalar transcription that caches nothing.  cos / sin go through
tests/shape_model.py's `Libm`: ``glibc`` is what the reference calls, ``device`` is what the kernel evaluates (the f64 routine rounded once).  The two differ
by at most one f32 ulp, so `Ring` also marks a pixel *fragile* when any of its 96 sample coordinates changes as that sample's cos or sin moves one ulp either
way: at every other pixel both flavours pick the same samples and give the same bytes."""
import numpy as np

from .shape_model import F, Libm, as_u8, rclamp, round_away

TAU = F(6.28318530717958647692)
N_SAMPLES = 24


def as_u32(v):
    """`v as u32` of one f32: truncates, saturates, NaN -> 0"""
    v = float(v)
    return 0 if not v > 0.0 else min(int(v), 0xFFFFFFFF)


def as_i32_arr(v):
    """`v as i32` elementwise (finite or not)"""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=2147483647.0, neginf=-2147483648.0)), -2147483648.0, 2147483647.0)).astype(np.int64)


def brush_alpha(dist, radius, hardness, anti_aliased):
    """compute_brush_alpha, brush_render.rs:54-82"""
    dist, radius = np.asarray(dist, F), F(radius)
    if radius <= 0:
        return np.zeros(dist.shape, F)
    safe = rclamp(F(hardness), F(0), F(1))
    t = rclamp(dist / radius, F(0), F(1))
    falloff = t * t * (F(3) - F(2) * t)
    material = F(1) + (safe - F(1)) * falloff
    if anti_aliased:
        edge0, edge1 = radius + F(0.5), radius - F(0.5)
        x = rclamp((dist - edge0) / (edge1 - edge0), F(0), F(1))
        coverage = np.where(dist <= edge1, F(1), np.where(dist >= edge0, F(0), x * x * (F(3) - F(2) * x))).astype(F)
    else:
        coverage = np.where(dist <= radius, F(1), F(0)).astype(F)
    return (material * coverage).astype(F)


def heal_alpha(dist, radius, hardness):
    """heal_circle :193-200"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = rclamp(np.asarray(dist, F) / F(radius), F(0), F(1))
        hard_t = rclamp(F(hardness) * F(0.9) + F(0.1), F(0), F(1))
        s = (t - hard_t) / (F(1) - hard_t + F(1e-6))
        return np.where(t < hard_t, F(1), F(1) - s * s * (F(3) - F(2) * s)).astype(F)


def dab_box(cx, cy, radius, w, h):
    """:17-20: (min_x, max_x, min_y, max_y), saturating casts"""
    cx, cy, radius = F(cx), F(cy), F(radius)
    return (as_u32(max(cx - radius, F(0))), min(as_u32(cx + radius), w - 1), as_u32(max(cy - radius, F(0))), min(as_u32(cy + radius), h - 1))


class Dirty:
    """Rect::union of the returned rects: componentwise min / max; nothing listed = zeros"""
    def __init__(self):
        self.box = None

    def add(self, x0, y0, x1, y1):
        self.box = (x0, y0, x1, y1) if self.box is None else (min(self.box[0], x0), min(self.box[1], y0), max(self.box[2], x1), max(self.box[3], y1))

    def add_dab(self, b, w, h):   # :88-97
        self.add(max(b[0] - 1, 0), max(b[2] - 1, 0), min(b[1] + 2, w), min(b[3] + 2, h))

    def get(self):
        return (0, 0, 0, 0) if self.box is None else tuple(int(v) for v in self.box)


class Ring:
    """heal_circle :205-234 per pixel of one layer, evaluated on demand and cached: rgb bytes, `count`, and the fragile mark"""
    def __init__(self, source, sample_radius, flavour="glibc"):
        self.src, self.sr, self.libm = np.ascontiguousarray(source, np.uint8), F(sample_radius), Libm(flavour)
        self.h, self.w = self.src.shape[:2]
        self.done = np.zeros((self.h, self.w), bool)
        self.rgb = np.zeros((self.h, self.w, 3), np.uint8)
        self.count = np.zeros((self.h, self.w), np.int32)
        self.fragile = np.zeros((self.h, self.w), bool)

    def _coords(self, base, trig, rr):
        return as_i32_arr(round_away(base[:, None] + trig * rr))

    def need(self, ys, xs):
        """evaluates the pixels (ys[k], xs[k]) that are not cached yet"""
        todo = ~self.done[ys, xs]
        ys, xs = ys[todo], xs[todo]
        if ys.size == 0:
            return
        seed = (xs.astype(np.uint64) * 1619 + ys.astype(np.uint64) * 3929) & 0xFFFFFFFF
        angle_offset = seed.astype(np.uint32).astype(F) / F(4294967296.0) * TAU
        steps = (np.arange(N_SAMPLES).astype(F) / F(N_SAMPLES)) * TAU
        angle = (angle_offset[:, None] + steps[None, :]).astype(F)
        c, s = self.libm.cos(angle), self.libm.sin(angle)
        xf, yf = xs.astype(F), ys.astype(F)
        sums, count, fragile = np.zeros((ys.size, 3), F), np.zeros(ys.size, F), np.zeros(ys.size, bool)
        for i in range(N_SAMPLES):          # the reference's accumulation order: sample i at 0.75 r, then at r
            for rr in (self.sr * F(0.75), self.sr):
                sx, sy = self._coords(xf, c[:, i:i + 1], rr)[:, 0], self._coords(yf, s[:, i:i + 1], rr)[:, 0]
                inside = (sx >= 0) & (sx < self.w) & (sy >= 0) & (sy < self.h)
                px = self.src[np.clip(sy, 0, self.h - 1), np.clip(sx, 0, self.w - 1)][:, :3].astype(F)
                sums = np.where(inside[:, None], sums + px, sums).astype(F)
                count = np.where(inside, count + F(1), count).astype(F)
                for trig, base, ref in ((c, xf, sx), (s, yf, sy)):
                    v = trig[:, i:i + 1]
                    for moved in (np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))):
                        fragile |= self._coords(base, moved.astype(F), rr)[:, 0] != ref
        with np.errstate(divide="ignore", invalid="ignore"):
            self.rgb[ys, xs] = as_u8(sums / count[:, None])
        self.count[ys, xs] = count.astype(np.int32)
        self.fragile[ys, xs] = fragile
        self.done[ys, xs] = True


def new_stats():
    return dict(sel=0, far=0, faint=0, off_canvas=0, empty_ring=0, wrote=0, tie=0, kept=0, alpha0=0, inexact_rgb=0, covered=None)


def _visit(stats, w, h):
    if stats is not None and stats["covered"] is None:
        stats["covered"] = np.zeros((h, w), bool)


def clone_dab(tool, source, preview, sel, cx, cy, stats=None):
    """clone_stamp_circle on `preview` in place; tool = dict(size, hardness, anti_aliased, offset)"""
    h, w = preview.shape[:2]
    radius = F(tool["size"]) / F(2)
    b = dab_box(cx, cy, radius, w, h)
    if b[0] > b[1] or b[2] > b[3]:
        return b
    ys, xs = np.mgrid[b[2]:b[3] + 1, b[0]:b[1] + 1]
    m = np.ones(ys.shape, bool) if sel is None else sel[ys, xs] != 0
    dx, dy = xs.astype(F) - F(cx), ys.astype(F) - F(cy)
    dist = np.sqrt(dx * dx + dy * dy).astype(F)
    near = ~(dist > radius)
    geom = brush_alpha(dist, radius, tool["hardness"], tool["anti_aliased"])
    solid = ~(geom < F(0.01))
    sx = as_i32_arr(round_away(xs.astype(F) + F(tool["offset"][0])))
    sy = as_i32_arr(round_away(ys.astype(F) + F(tool["offset"][1])))
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    sp = source[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(F) / F(255)
    alpha = (geom * sp[..., 3]).astype(F)
    old = preview[ys, xs, 3].astype(F) / F(255)
    live = m & near & solid & inside
    wr = live & (alpha >= old)
    rgb = as_u8(sp[..., :3] * F(255))
    if stats is not None:
        _visit(stats, w, h)
        stats["sel"] += int((~m).sum()); stats["far"] += int((m & ~near).sum()); stats["faint"] += int((m & near & ~solid).sum())
        stats["off_canvas"] += int((m & near & solid & ~inside).sum())
        stats["wrote"] += int(wr.sum()); stats["tie"] += int((wr & (alpha == old)).sum()); stats["kept"] += int((live & ~wr).sum())
        stats["alpha0"] += int((wr & (sp[..., 3] == 0)).sum())
        stats["inexact_rgb"] += int((wr & (rgb != source[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)][..., :3]).any(axis=-1)).sum())
        stats["covered"][ys[wr], xs[wr]] = True
    preview[ys[wr], xs[wr], :3] = rgb[wr]
    preview[ys[wr], xs[wr], 3] = as_u8(alpha * F(255))[wr]
    return b


def heal_dab(tool, ring, preview, sel, cx, cy, stats=None):
    """heal_circle on `preview` in place; tool = dict(size, hardness, sample_radius), ring = a Ring over the layer"""
    h, w = preview.shape[:2]
    radius = F(tool["size"]) / F(2)
    b = dab_box(cx, cy, radius, w, h)
    if b[0] > b[1] or b[2] > b[3]:
        return b
    ys, xs = np.mgrid[b[2]:b[3] + 1, b[0]:b[1] + 1]
    m = np.ones(ys.shape, bool) if sel is None else sel[ys, xs] != 0
    dx, dy = xs.astype(F) - F(cx), ys.astype(F) - F(cy)
    dist = np.sqrt(dx * dx + dy * dy).astype(F)
    near = ~(dist > radius)
    geom = heal_alpha(dist, radius, tool["hardness"])
    solid = ~(geom < F(0.01))
    reach = m & near & solid
    ring.need(ys[reach], xs[reach])
    full = ring.count[ys, xs] >= 1
    old = preview[ys, xs, 3].astype(F) / F(255)
    live = reach & full
    wr = live & (geom >= old)
    if stats is not None:
        _visit(stats, w, h)
        stats["sel"] += int((~m).sum()); stats["far"] += int((m & ~near).sum()); stats["faint"] += int((m & near & ~solid).sum())
        stats["empty_ring"] += int((reach & ~full).sum())
        stats["wrote"] += int(wr.sum()); stats["tie"] += int((wr & (geom == old)).sum()); stats["kept"] += int((live & ~wr).sum())
        stats["covered"][ys[wr], xs[wr]] = True
    preview[ys[wr], xs[wr], :3] = ring.rgb[ys[wr], xs[wr]]
    preview[ys[wr], xs[wr], 3] = as_u8(geom * F(255))[wr]
    return b


def clone_stroke(tool, source, preview, sel, points, stats=None):
    """every dab of `points` in order: (the new preview, the dirty box)"""
    out, dirty = np.array(preview, np.uint8), Dirty()
    h, w = out.shape[:2]
    for cx, cy in np.asarray(points, F).reshape(-1, 2):
        dirty.add_dab(clone_dab(tool, source, out, sel, cx, cy, stats), w, h)
    return out, dirty.get()


def heal_stroke(tool, ring, preview, sel, points, stats=None):
    out, dirty = np.array(preview, np.uint8), Dirty()
    h, w = out.shape[:2]
    for cx, cy in np.asarray(points, F).reshape(-1, 2):
        dirty.add_dab(heal_dab(tool, ring, out, sel, cx, cy, stats), w, h)
    return out, dirty.get()


def pencil_cells(color, preview, sel, cells, stats=None):
    """draw_pixel_and_get_bounds per cell: (the new preview, the reference's dirty box — a cell the selection masks returns Rect::NOTHING)"""
    out, dirty = np.array(preview, np.uint8), Dirty()
    h, w = out.shape[:2]
    c = np.asarray(color, F)
    for x, y in np.asarray(cells, np.int64).reshape(-1, 2):
        if x < 0 or y < 0 or x >= w or y >= h:
            continue
        if sel is not None and sel[y, x] == 0:
            if stats is not None:
                stats["sel"] += 1
            continue
        old = F(out[y, x, 3]) / F(255)
        if c[3] >= old:
            out[y, x] = as_u8(c * F(255))
            if stats is not None:
                stats["wrote"] += 1; stats["tie"] += int(c[3] == old)
        elif stats is not None:
            stats["kept"] += 1
        dirty.add(max(x - 1, 0), max(y - 1, 0), min(x + 2, w), min(y + 2, h))
    return out, dirty.get()


def cells_box(cells, w, h):
    """the library's pencil box: the union over the listed in-canvas cells, the selection not consulted"""
    d = Dirty()
    for x, y in np.asarray(cells, np.int64).reshape(-1, 2):
        if 0 <= x < w and 0 <= y < h:
            d.add(max(x - 1, 0), max(y - 1, 0), min(x + 2, w), min(y + 2, h))
    return d.get()


def line_points(start, end, w, h):
    """clone_stamp_line / heal_line :108-130: the kept dab centres, (n, 2) f32"""
    x0, y0, x1, y1 = F(start[0]), F(start[1]), F(end[0]), F(end[1])
    dx, dy = x1 - x0, y1 - y0
    distance = np.sqrt(dx * dx + dy * dy)
    if distance < F(0.1):
        return np.array([[x0, y0]], F)
    steps = int(np.ceil(distance))
    out = []
    for i in range(steps + 1):
        t = F(i) / F(steps)
        x, y = x0 + dx * t, y0 + dy * t
        if x >= 0 and as_u32(x) < w and y >= 0 and as_u32(y) < h:
            out.append((x, y))
    return np.array(out, F).reshape(-1, 2)


def line_cells(start, end, w, h):
    """draw_pixel_line_and_get_bounds :389-428: the in-canvas cells, (n, 2) i32"""
    x0, y0, x1, y1 = (int(np.floor(F(v))) for v in (start[0], start[1], end[0], end[1]))
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err, out = dx - dy, []
    while True:
        if 0 <= x0 < w and 0 <= y0 < h:
            out.append((x0, y0))
        if x0 == x1 and y0 == y1:
            break
        e2 = 2 * err
        if e2 > -dy:
            err -= dy; x0 += sx
        if e2 < dx:
            err += dx; y0 += sy
    return np.array(out, np.int32).reshape(-1, 2)
