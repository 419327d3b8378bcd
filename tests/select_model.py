"""CPU model of the selection masks (the CanvasState / tools flavour), independent of the C++: a literal numpy restatement of the reference's

    SelectionShape::contains / bounds          src/canvas/selection.rs:66-116
    selection_mask_bounds, translate_selection src/canvas/canvas_state.rs:1632-1710
    apply_selection_shape                      :1713-1803  (its merge, literally, is in tests/test_select_model_host.py; here: the one combine rule)
    delete_selected_pixels, fill_selected_pixels :1806-1887
    apply_lasso_selection                      src/ui/panels/tools/behavior/raster/perspective_gradient.rs:2-38
    feather / expand / contract_selection      src/ops/adjustments.rs:1448-1591

Every float step is an np.float32 operation (one rounding each, nothing fused); Rust's `as u32` is written out: it truncates, saturates and sends NaN to 0.
Masks are (h, w) uint8, layers (h, w, 4) uint8.  Expand and contract are brute force over the disc's offsets, the feather sums its windows offset by offset;
`expand_two_pass` / `contract_two_pass` restate the formulation the device kernels use (row distances, then a column walk over the disc's row spans) so that it
is held to the brute force without a GPU."""
import math

import numpy as np

F = np.float32
REPLACE, ADD, SUBTRACT, INTERSECT = 0, 1, 2, 3
MODES = (REPLACE, ADD, SUBTRACT, INTERSECT)
LASSO_MAX_POINTS = 8192
FEATHER_MAX_RADIUS = 512
MORPH_MAX_RADIUS = 46340


def cast_u32(v) -> int:
    """Rust's `v as u32` for an f32"""
    v = F(v)
    if np.isnan(v) or v <= 0:
        return 0
    if v >= F(4294967296.0):
        return 0xFFFFFFFF
    return int(v)   # truncates


def rs_max(a, b):
    """f32::max: a NaN operand loses"""
    a, b = F(a), F(b)
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    return a if a > b else b


# ---- the combine rule ----------------------------------------------------------------------------------------------------------------------------------------
def combine(base, raw, mode):
    """raw: (h, w) of 0 / 255; base: (h, w) uint8 or None (all zero)"""
    base = np.zeros_like(raw) if base is None else np.asarray(base, np.uint8)
    on = raw == 255
    inside = {REPLACE: np.uint8(255), ADD: np.uint8(255), SUBTRACT: np.uint8(0), INTERSECT: base}[mode]
    outside = {REPLACE: np.uint8(0), ADD: base, SUBTRACT: base, INTERSECT: np.uint8(0)}[mode]
    return np.where(on, inside, outside).astype(np.uint8)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------------------------
def rect_raw(w, h, min_x, min_y, max_x, max_y):
    raw = np.zeros((h, w), np.uint8)
    bx1, by1 = min(max_x, w - 1), min(max_y, h - 1)              # bounds :96-106
    for y in range(min_y, by1 + 1):                              # an empty range when min > max
        for x in range(min_x, bx1 + 1):
            raw[y, x] = 255                                      # contains :76 holds for every pixel of the box
    return raw


def ellipse_box(w, h, cx, cy, rx, ry):
    with np.errstate(all="ignore"):
        cx, cy, rx, ry = F(cx), F(cy), F(rx), F(ry)
        bx0 = cast_u32(np.floor(rs_max(cx - rx, 0)))             # bounds :107-113
        by0 = cast_u32(np.floor(rs_max(cy - ry, 0)))
        bx1 = min(cast_u32(np.ceil(cx + rx)), w - 1)
        by1 = min(cast_u32(np.ceil(cy + ry)), h - 1)
    return bx0, by0, bx1, by1


def ellipse_raw(w, h, cx, cy, rx, ry):
    raw = np.zeros((h, w), np.uint8)
    cx, cy, rx, ry = F(cx), F(cy), F(rx), F(ry)
    bx0, by0, bx1, by1 = ellipse_box(w, h, cx, cy, rx, ry)
    if bx0 > bx1 or by0 > by1:
        return raw
    if rx <= 0 or ry <= 0:                                       # contains :83 (false for a NaN, which then fails the <= 1 below)
        return raw
    with np.errstate(all="ignore"):
        dx = (np.arange(bx0, bx1 + 1).astype(F) - cx) / rx       # :86
        dy = (np.arange(by0, by1 + 1).astype(F) - cy) / ry
        inside = (dx * dx)[None, :] + (dy * dy)[:, None] <= F(1.0)
    raw[by0:by1 + 1, bx0:bx1 + 1][inside] = 255
    return raw


def lasso_row_nodes(points, y):
    """the sorted crossings of row y (:12-27)"""
    pts = np.asarray(points, F).reshape(-1, 2)
    n = len(pts)
    if n == 0:
        return np.zeros(0, F)
    yf = F(y) + F(0.5)
    xi, yi = pts[:, 0], pts[:, 1]
    xj, yj = np.roll(xi, -1), np.roll(yi, -1)                    # j = (i + 1) % n
    cross = ((yi < yf) & (yj >= yf)) | ((yj < yf) & (yi >= yf))
    xi, yi, xj, yj = xi[cross], yi[cross], xj[cross], yj[cross]
    t = (yf - yi) / (yj - yi)
    return np.sort(xi + t * (xj - xi))


def lasso_raw(w, h, points, counts=None):
    """counts: a list that receives every row's crossing count"""
    raw = np.zeros((h, w), np.uint8)
    for y in range(h):
        nodes = lasso_row_nodes(points, y)
        if counts is not None:
            counts.append(len(nodes))
        k = 0
        while k + 1 < len(nodes):
            x_start = min(cast_u32(rs_max(nodes[k], 0)), w)
            x_end = min(cast_u32(rs_max(nodes[k + 1] + F(1.0), 0)), w)
            raw[y, x_start:x_end] = 255                          # an empty slice when x_start >= x_end
            k += 2
    return raw


def select_rect(base, w, h, min_x, min_y, max_x, max_y, mode):
    return combine(base, rect_raw(w, h, min_x, min_y, max_x, max_y), mode)


def select_ellipse(base, w, h, cx, cy, rx, ry, mode):
    return combine(base, ellipse_raw(w, h, cx, cy, rx, ry), mode)


def select_lasso(base, w, h, points, mode):
    return combine(base, lasso_raw(w, h, points), mode)


# ---- translate, bounds -----------------------------------------------------------------------------------------------------------------------------------------
def translate(mask, dx, dy):
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    out = np.zeros_like(mask)
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs.astype(np.int64) - dx, ys.astype(np.int64) - dy  # :1696-1697
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out[ok] = mask[sy[ok], sx[ok]]
    return out


def bounds(mask):
    """x0, y0, x1, y1 inclusive of mask != 0; four -1 when empty"""
    ys, xs = np.nonzero(np.asarray(mask))
    if len(xs) == 0:
        return np.full(4, -1, np.int32)
    return np.array([xs.min(), ys.min(), xs.max(), ys.max()], np.int32)


# ---- feather ---------------------------------------------------------------------------------------------------------------------------------------------------
def feather_params(radius):
    """(passes, r) (:1457-1458)"""
    radius = F(radius)
    return max(cast_u32(radius / F(2.0)), 1), max(cast_u32(radius), 1)


def _box_axis(data, r, axis):
    """one direction of a pass: the window [max(p - r, 0), min(p + r, n - 1)], `sum / count` truncating"""
    a = np.moveaxis(data, axis, 1).astype(np.uint32)
    n = a.shape[1]
    total = np.zeros_like(a)
    for d in range(-min(r, n - 1), min(r, n - 1) + 1):           # source = p + d, where it is inside
        if d >= 0:
            total[:, :n - d] += a[:, d:]
        else:
            total[:, -d:] += a[:, :n + d]
    p = np.arange(n)
    count = (np.minimum(p + r, n - 1) - np.maximum(p - r, 0) + 1).astype(np.uint32)
    return np.moveaxis((total // count[None, :]).astype(np.uint8), 1, axis)


def feather(mask, radius):
    passes, r = feather_params(radius)
    data = np.asarray(mask, np.uint8)
    for _ in range(passes):
        data = _box_axis(_box_axis(data, r, 1), r, 0)            # horizontal, then vertical, each through u8
    return data


# ---- expand / contract -----------------------------------------------------------------------------------------------------------------------------------------
def _any_in_disc(pred, r):
    """per pixel: does a pixel of the image within dx^2 + dy^2 <= r^2 satisfy pred?  Brute force, offset by offset"""
    h, w = pred.shape
    found = np.zeros((h, w), bool)
    for dy in range(-min(r, h - 1), min(r, h - 1) + 1):
        for dx in range(-min(r, w - 1), min(r, w - 1) + 1):
            if dx * dx + dy * dy > r * r:
                continue
            # found[y, x] |= pred[y + dy, x + dx] where that is inside
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            found[y0:y1, x0:x1] |= pred[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return found


def expand(mask, radius):
    mask = np.asarray(mask, np.uint8)
    r = max(int(radius), 0)
    out = mask.copy()
    out[(mask <= 127) & _any_in_disc(mask > 127, r)] = 255
    return out


def contract(mask, radius):
    mask = np.asarray(mask, np.uint8)
    r = max(int(radius), 0)
    out = mask.copy()
    out[(mask != 0) & _any_in_disc(mask == 0, r)] = 0
    return out


def span_table(r):
    """span[k] = floor(sqrt(r^2 - k^2)), k = 0 .. r"""
    return [math.isqrt(r * r - k * k) for k in range(r + 1)]


def row_distance(pred, r):
    """per pixel the distance to the nearest pred pixel of its row, saturated at r + 1"""
    h, w = pred.shape
    g = np.full((h, w), r + 1, np.int64)
    x = np.arange(w)
    for y in range(h):
        at = np.nonzero(pred[y])[0]
        if len(at):
            g[y] = np.minimum(np.abs(x[:, None] - at[None, :]).min(axis=1), r + 1)
    return g


def _any_in_disc_two_pass(pred, r):
    h, w = pred.shape
    g, span = row_distance(pred, r), span_table(r)
    found = np.zeros((h, w), bool)
    for dy in range(-min(r, h - 1), min(r, h - 1) + 1):
        y0, y1 = max(0, -dy), min(h, h - dy)
        found[y0:y1] |= g[y0 + dy:y1 + dy] <= span[abs(dy)]
    return found


def expand_two_pass(mask, radius):
    mask = np.asarray(mask, np.uint8)
    r = max(int(radius), 0)
    out = mask.copy()
    out[(mask <= 127) & _any_in_disc_two_pass(mask > 127, r)] = 255
    return out


def contract_two_pass(mask, radius):
    mask = np.asarray(mask, np.uint8)
    r = max(int(radius), 0)
    out = mask.copy()
    out[(mask != 0) & _any_in_disc_two_pass(mask == 0, r)] = 0
    return out


# ---- fill / delete -----------------------------------------------------------------------------------------------------------------------------------------------
def _round_u8(v):
    """f32::round (half away from zero) then `as u8`, for v >= 0: the f64 sum v + 0.5 is exact"""
    return np.clip(np.floor(v.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


def fill_selected(layer, mask, color):
    layer, mask = np.asarray(layer, np.uint8), np.asarray(mask, np.uint8)
    out = layer.copy()
    t = (mask.astype(F) / F(255.0))[..., None]                                     # :1870
    new = np.asarray(color, np.uint8).astype(F)[None, None, :]
    blended = _round_u8(layer.astype(F) * (F(1.0) - t) + new * t)                    # :1872
    part = (mask > 0) & (mask < 255)
    out[part] = blended[part]
    out[mask == 255] = np.asarray(color, np.uint8)
    return out


def delete_selected(layer, mask):
    layer, mask = np.asarray(layer, np.uint8), np.asarray(mask, np.uint8)
    out = layer.copy()
    factor = F(1.0) - mask.astype(F) / F(255.0)                                      # :1832
    alpha = _round_u8(layer[..., 3].astype(F) * factor)
    part = (mask > 0) & (mask < 255)
    out[..., 3][part] = alpha[part]
    out[mask == 255] = 0
    return out
