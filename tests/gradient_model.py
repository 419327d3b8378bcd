"""CPU model of the gradient tool and the perspective crop: a vectorised numpy-float32 restatement of what the reference computes (tools/state.rs rebuild_lut
:1063, apply_preset :1144; behavior/raster/perspective_gradient.rs apply_perspective_crop :94, bilinear_sample :186, render_gradient_to_preview's CPU path
:386-523, the premultiplied copy :559-572; gradient_text/gradient_controls.rs commit_gradient :63-122).  Every f32 step is one numpy float32 operation (numpy
neither fuses nor reassociates), sqrt and division are correctly rounded, np.fmod is exact, round() is half away from zero.  There is no golden and no
reference test for these tools: tests/test_gradient_model_host.py holds this file to a scalar transcription written independently and to hand-derived answers."""
import numpy as np

F = np.float32
LINEAR, REFLECTED, RADIAL, DIAMOND = range(4)
COLOR, TRANSPARENCY = 0, 1
PRESETS = ["primary_secondary", "black_white", "foreground_transparent", "rainbow"]


def gradient(start, end, shape=LINEAR, repeat=False, mode=COLOR, preview_scale=1):
    return dict(start=(float(start[0]), float(start[1])), end=(float(end[0]), float(end[1])), shape=int(shape), repeat=bool(repeat), mode=int(mode),
                preview_scale=int(preview_scale))


def round_u8(v):
    """`.round().clamp(0, 255) as u8` and `.round() as u8` alike: half away from zero, saturating, NaN -> 0; the f64 sum is exact for every f32"""
    v = np.asarray(v, np.float64)
    r = np.where(v < 0, -np.floor(-v + 0.5), np.floor(v + 0.5))
    return np.where(np.isnan(v), 0, np.clip(r, 0, 255)).astype(np.uint8)


# ---- the LUT ---------------------------------------------------------------------------------------------------------------------------------------------------------
def build_lut(stops):
    """rebuild_lut: stops = [(position, (r, g, b, a)), ...] -> (256, 4) u8"""
    lut = np.zeros((256, 4), np.uint8)
    if not stops:
        return lut
    if len(stops) == 1:
        lut[:] = stops[0][1]
        return lut
    order = sorted(range(len(stops)), key=lambda i: F(stops[i][0]))        # sorted() is stable, like sort_by
    pos = [F(stops[i][0]) for i in order]
    col = [np.array(stops[i][1], np.float32) for i in order]
    for i in range(256):
        t = F(i) / F(255.0)
        if t <= pos[0]:
            lut[i] = col[0]
        elif t >= pos[-1]:
            lut[i] = col[-1]
        else:
            l, r = 0, len(pos) - 1
            for j in range(len(pos) - 1):
                if pos[j] <= t <= pos[j + 1]:
                    l, r = j, j + 1
                    break
            span = F(pos[r] - pos[l])
            local_t = F(F(t - pos[l]) / span) if span > 0 else F(0.0)
            inv = F(F(1.0) - local_t)
            lut[i] = round_u8(col[l] * inv + col[r] * local_t)
    return lut


def preset_stops(preset, primary, secondary):
    p, s = tuple(int(v) for v in primary), tuple(int(v) for v in secondary)
    name = preset if isinstance(preset, str) else PRESETS[preset]
    return {"primary_secondary": [(0.0, p), (1.0, s)],
            "black_white": [(0.0, (0, 0, 0, 255)), (1.0, (255, 255, 255, 255))],
            "foreground_transparent": [(0.0, p), (1.0, (p[0], p[1], p[2], 0))],
            "rainbow": [(0.0, (255, 0, 0, 255)), (0.17, (255, 165, 0, 255)), (0.33, (255, 255, 0, 255)), (0.5, (0, 200, 0, 255)), (0.67, (0, 100, 255, 255)),
                        (0.83, (75, 0, 130, 255)), (1.0, (148, 0, 211, 255))]}[name]


def bake_eraser_lut(lut):
    """:395-409: rgb = 255, a = lum * a / 255 with lum = (0.299 r + 0.587 g + 0.114 b) as u8, the sum left to right in f32"""
    src = np.asarray(lut, np.uint8).reshape(256, 4).astype(np.float32)
    lum = (F(0.299) * src[:, 0] + F(0.587) * src[:, 1]) + F(0.114) * src[:, 2]
    lum = np.clip(np.trunc(lum.astype(np.float64)), 0, 255).astype(np.uint32)
    out = np.full((256, 4), 255, np.uint8)
    out[:, 3] = lum * np.asarray(lut, np.uint8).reshape(256, 4)[:, 3].astype(np.uint32) // 255
    return out


def drag_scale(w, h):
    """:291-300, the square root in f64"""
    total = int(w) * int(h)
    if total <= 1_500_000:
        return 1
    return max(int(np.ceil(np.sqrt(np.float64(total) / np.float64(1_000_000.0)))), 2)


# ---- render ------------------------------------------------------------------------------------------------------------------------------------------------------------
def rem_euclid(x, m):
    r = np.fmod(x, F(m))
    return np.where(r < 0, r + F(m), r).astype(np.float32)


def rs_clamp(x):
    """f32::clamp(0.0, 1.0): comparisons, NaN stays NaN"""
    return np.where(x < 0, F(0.0), np.where(x > 1, F(1.0), x)).astype(np.float32)


def gen_size(w, h, scale):
    return -(-w // scale), -(-h // scale)


def render(g, lut, w, h, selection=None, stats=None):
    """the (gen_h, gen_w, 4) preview.  lut is the RAW table; transparency mode bakes it.  stats, when a dict, receives the branch counts the host tests assert"""
    scale = g["preview_scale"]
    gen_w, gen_h = gen_size(w, h, scale)
    table = bake_eraser_lut(lut) if g["mode"] == TRANSPARENCY else np.asarray(lut, np.uint8).reshape(256, 4)
    ax, ay, bx, by = F(g["start"][0]), F(g["start"][1]), F(g["end"][0]), F(g["end"][1])
    with np.errstate(all="ignore"):
        dx, dy = F(bx - ax), F(by - ay)
        len_sq = F(F(dx * dx) + F(dy * dy))
        length = F(np.sqrt(len_sq))
        inv_len = F(F(1.0) / length) if length > F(1e-6) else F(0.0)
        inv_len_sq = F(F(1.0) / len_sq) if len_sq > F(1e-6) else F(0.0)
        ux, uy = F(dx * inv_len), F(dy * inv_len)
        sf = F(scale)
        px = np.arange(gen_w, dtype=np.float32) * sf + F(sf * F(0.5))
        py = np.arange(gen_h, dtype=np.float32) * sf + F(sf * F(0.5))
        rx, ry = (px - ax)[None, :], (py - ay)[:, None]
        shape, repeat = g["shape"], g["repeat"]
        if shape in (LINEAR, REFLECTED):
            raw = (rx * dx + ry * dy) * inv_len_sq
        elif shape == RADIAL:
            raw = np.sqrt(rx * rx + ry * ry) * inv_len
        else:
            raw = np.abs(rx * ux + ry * uy) * inv_len + np.abs(rx * F(-uy) + ry * ux) * inv_len
        raw = np.broadcast_to(raw, (gen_h, gen_w)).astype(np.float32)
        if shape == REFLECTED:
            if repeat:
                t_mod = rem_euclid(raw, 2.0)
                t = np.where(t_mod > 1, F(2.0) - t_mod, t_mod).astype(np.float32)
            else:
                t = F(1.0) - np.abs(F(2.0) * rs_clamp(raw) - F(1.0))
        else:
            t = rem_euclid(raw, 1.0) if repeat else rs_clamp(raw)
        scaled = t * F(255.0)
        idx = np.where(np.isnan(scaled), 0, np.trunc(scaled)).astype(np.int64)   # `as usize`: truncates, NaN -> 0
    assert idx.min() >= 0 and idx.max() <= 255, "the reference would panic"
    entry = table[idx]
    a = entry[..., 3].astype(np.uint32)
    sv = np.full((gen_h, gen_w), 255, np.uint32)
    if selection is not None:
        sel = np.asarray(selection, np.uint8).reshape(h, w)
        sv = sel[(np.arange(gen_h) * scale)[:, None], (np.arange(gen_w) * scale)[None, :]].astype(np.uint32)
    a = np.where(sv < 255, a * sv // 255, a)
    drawn = (sv != 0) & (a != 0)
    out = np.zeros((gen_h, gen_w, 4), np.uint8)
    out[..., :3] = np.where(drawn[..., None], entry[..., :3], 0)
    out[..., 3] = np.where(drawn, a, 0)
    if stats is not None:
        with np.errstate(all="ignore"):
            live = sv != 0
            bound = 2.0 if (shape == REFLECTED and repeat) else 1.0
            stats.update(outside=int((live & ((raw < 0) | (raw >= bound))).sum()), inside=int((live & (raw >= 0) & (raw < bound)).sum()),
                         negative_remainder=int((live & repeat & (np.fmod(raw, F(bound)) < 0)).sum()),
                         folded=int((live & (shape == REFLECTED) & repeat & (rem_euclid(raw, 2.0) > 1)).sum()),
                         dropped=int((sv == 0).sum()), grey=int(((sv > 0) & (sv < 255)).sum()), lut_alpha_zero=int((live & (entry[..., 3] == 0)).sum()),
                         grey_to_zero=int((live & (entry[..., 3] != 0) & (a == 0)).sum()), drawn=int(drawn.sum()))
    return out


def premultiply(preview):
    """preview_flat_buffer :559-572"""
    p = np.asarray(preview, np.uint8).astype(np.uint32)
    out = np.empty_like(preview)
    out[..., :3] = (p[..., :3] * p[..., 3:4] + 128) // 255
    out[..., 3] = preview[..., 3]
    return out


# ---- commit ------------------------------------------------------------------------------------------------------------------------------------------------------------
def commit(layer, preview, is_eraser):
    """commit_gradient :85-119: the layer after the full-resolution preview went onto it"""
    layer, preview = np.asarray(layer, np.uint8), np.asarray(preview, np.uint8)
    assert layer.shape == preview.shape
    touch = preview[..., 3] != 0
    sa = preview[..., 3].astype(np.float32) / F(255.0)
    da = layer[..., 3].astype(np.float32) / F(255.0)
    rest = F(1.0) - sa
    out = layer.copy()
    if is_eraser:
        new_a = np.maximum(da * rest, F(0.0))
        out[..., 3] = np.where(touch, round_u8(new_a * F(255.0)), layer[..., 3])
        return out
    with np.errstate(all="ignore"):
        out_a = sa + da * rest
        s, d = preview[..., :3].astype(np.float32), layer[..., :3].astype(np.float32)
        rgb = (s * sa[..., None] + d * da[..., None] * rest[..., None]) / out_a[..., None]
    blended = np.concatenate([round_u8(rgb), round_u8(out_a * F(255.0))[..., None]], axis=-1)
    return np.where((touch & (out_a > 0))[..., None], blended, layer)


def apply(g, lut, layer, selection=None):
    """the release: render at scale 1, then commit in the descriptor's mode"""
    assert g["preview_scale"] == 1
    h, w = layer.shape[:2]
    return commit(layer, render(g, lut, w, h, selection), g["mode"] == TRANSPARENCY)


# ---- perspective crop ------------------------------------------------------------------------------------------------------------------------------------------------
def crop_plan(corners, w, h):
    """:100-125: (out_w, out_h), or None where the reference returns None.  corners = [TL, TR, BR, BL]"""
    xs, ys = [F(c[0]) for c in corners], [F(c[1]) for c in corners]
    min_x, min_y = max(min(xs), F(0.0)), max(min(ys), F(0.0))
    max_x, max_y = min(max(xs), F(w)), min(max(ys), F(h))

    def as_u32(v):                                                     # (max - min).round() as u32
        v = np.float64(v)
        r = -np.floor(-v + 0.5) if v < 0 else np.floor(v + 0.5)
        return int(min(max(r, 0.0), 4294967295.0))
    out_w, out_h = as_u32(F(max_x - min_x)), as_u32(F(max_y - min_y))
    return None if out_w < 2 or out_h < 2 else (out_w, out_h)


def crop_coordinates(corners, out_w, out_h):
    c = [(F(p[0]), F(p[1])) for p in corners]
    with np.errstate(all="ignore"):
        u = ((np.arange(out_w, dtype=np.float32) + F(0.5)) / F(out_w))[None, :]
        v = ((np.arange(out_h, dtype=np.float32) + F(0.5)) / F(out_h))[:, None]
        iu, iv = F(1.0) - u, F(1.0) - v
        sx = iu * iv * c[0][0] + u * iv * c[1][0] + u * v * c[2][0] + iu * v * c[3][0]
        sy = iu * iv * c[0][1] + u * iv * c[1][1] + u * v * c[2][1] + iu * v * c[3][1]
    return sx.astype(np.float32), sy.astype(np.float32)


def crop(corners, layer, stats=None):
    """apply_perspective_crop :150-165 with bilinear_sample :186-233 on one (h, w, 4) layer; None where the plan is None"""
    layer = np.asarray(layer, np.uint8)
    h, w = layer.shape[:2]
    plan = crop_plan(corners, w, h)
    if plan is None:
        return None
    sx, sy = crop_coordinates(corners, *plan)

    def taps(coord, n):
        with np.errstate(all="ignore"):
            fl = np.floor(coord)
            frac = (coord - fl).astype(np.float32)                     # from the unclamped coordinate
        i32 = np.clip(np.where(np.isnan(fl), 0.0, fl.astype(np.float64)), -2147483648.0, 2147483647.0)
        i0 = np.clip(i32, 0, n - 1).astype(np.int64)
        return fl, i0, np.minimum(i0 + 1, n - 1), frac
    flx, x0, x1, fx = taps(sx, w)
    fly, y0, y1, fy = taps(sy, h)

    def lerp(a, b, t):
        with np.errstate(all="ignore"):
            return round_u8(a.astype(np.float32) * (F(1.0) - t)[..., None] + b.astype(np.float32) * t[..., None])
    top = lerp(layer[y0, x0], layer[y0, x1], fx)
    bottom = lerp(layer[y1, x0], layer[y1, x1], fx)
    if stats is not None:
        stats.update(left=int((flx < 0).sum()), right=int((flx > w - 1).sum()), x1_clamped=int((x0 + 1 > w - 1).sum()), above=int((fly < 0).sum()),
                     below=int((fly > h - 1).sum()), y1_clamped=int((y0 + 1 > h - 1).sum()), inside=int(((flx >= 0) & (flx < w - 1) & (fly >= 0) & (fly < h - 1)).sum()))
    return lerp(top, bottom, fy)
