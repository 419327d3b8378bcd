"""CPU model of content-aware fill: a numpy / Python restatement of the reference's `inpaint_instant_brush` (src/ops/inpaint.rs:76-192) and
`fill_region_patchmatch` (:394-520), in strict f32 and in the reference's evaluation order.

* every arithmetic step is one f32 rounding (numpy float32 scalars / arrays; no fused operation);
* `round()` is half away from zero; `as u8` / `as u32` / `as i32` truncate and saturate (NaN -> 0);
* `cosf` / `sinf` / `expf` are the host's glibc through ctypes: what Rust's f32::cos / sin / exp call on Linux;
* the LCG state is a u64 with wrap-around; `(rng >> 33) as f32 / (u32::MAX as f32)` divides by 2^32 (u32::MAX as f32 rounds up).

The whole operator is in the EXACT class: the only per-pixel transcendental is exp, and the device's `libm_exp` (k_libm.h) is glibc's expf bit for bit.

Both routines return counters beside the image.  instant(): pixels changed.  patchmatch(): peels, SSD evaluations whose integer sum reached 2^24 (the
sequential-f32 branch of the device's SSD), and boundary pixels left unfilled."""
import ctypes as C
import ctypes.util

import numpy as np

f32 = np.float32
_m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf", "expf"):
    getattr(_m, _n).restype = C.c_float
    getattr(_m, _n).argtypes = [C.c_float]

F32_MAX = f32(3.4028234663852886e38)
TAU = f32(6.283185307179586)
MASK64 = (1 << 64) - 1
LCG_MUL = 6364136223846793005


def cosf(x): return f32(_m.cosf(float(x)))
def sinf(x): return f32(_m.sinf(float(x)))


def expf(a):
    a = np.asarray(a, f32)
    return np.array([_m.expf(float(v)) for v in a.ravel()], f32).reshape(a.shape)


def rs_round(v):
    """f32::round: half away from zero (two-step form, exact)"""
    v = np.asarray(v, f32)
    t = np.trunc(v)
    d = v - t
    return np.where(np.abs(d) >= f32(0.5), t + np.copysign(f32(1.0), v), t).astype(f32)


def as_u8(v):
    v = np.asarray(v, f32)
    return np.trunc(np.clip(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0)).astype(np.uint8)


def as_u32(v):
    v = float(v)
    if not v > 0.0:
        return 0
    return 0xFFFFFFFF if v >= 4294967296.0 else int(v)


def as_i32(v):
    v = np.nan_to_num(np.asarray(v, np.float64), nan=0.0)
    return np.trunc(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- instant dabs

def ring_offsets(sample_radius):
    """:88-89, :141-147 — the 32 candidates' (cos(angle) * rr, sin(angle) * rr), interleaved x, y: what pfx_inpaint_ring_offsets returns"""
    sample_radius = f32(sample_radius)
    inner_r = sample_radius * f32(0.25)
    outer_r = sample_radius
    step = TAU / f32(32.0)
    out = np.empty(64, f32)
    for i in range(32):
        angle = f32(i) * step
        rr = inner_r + (outer_r - inner_r) * (f32(i) / f32(31.0))
        out[2 * i] = cosf(angle) * rr
        out[2 * i + 1] = sinf(angle) * rr
    return out


def instant(src, mask, out, cx, cy, brush_radius, sample_radius, hardness):
    """inpaint_instant_brush on a copy of `out`: (image, pixels changed).  Vectorised over the dab's pixel box; every expression is the reference's."""
    src = np.ascontiguousarray(src, np.uint8)
    mask = np.ascontiguousarray(mask, np.uint8)
    out = np.array(out, np.uint8, copy=True)
    h, w = mask.shape
    cx, cy, hardness = f32(cx), f32(cy), f32(hardness)
    r = max(f32(brush_radius), f32(1.0))
    min_x, max_x = as_u32(max(cx - r, f32(0.0))), min(as_u32(np.ceil(cx + r)), w - 1)
    min_y, max_y = as_u32(max(cy - r, f32(0.0))), min(as_u32(np.ceil(cy + r)), h - 1)
    if min_x > max_x or min_y > max_y:
        return out, 0
    offs = ring_offsets(sample_radius)
    ys, xs = np.mgrid[min_y:max_y + 1, min_x:max_x + 1]
    xs, ys = xs.ravel(), ys.ravel()
    keep = mask[ys, xs] != 0
    xs, ys = xs[keep], ys[keep]
    xf, yf = xs.astype(f32), ys.astype(f32)
    dx, dy = xf - cx, yf - cy
    dist = np.sqrt(dx * dx + dy * dy)
    keep = ~(dist > r)
    xs, ys, xf, yf, dist = xs[keep], ys[keep], xf[keep], yf[keep], dist[keep]
    t = np.clip(dist / r, f32(0.0), f32(1.0))
    hard_t = np.clip(hardness * f32(0.9) + f32(0.1), f32(0.0), f32(1.0)).astype(f32)
    s = (t - hard_t) / (f32(1.0) - hard_t + f32(1e-6))
    geom = np.where(t < hard_t, f32(1.0), f32(1.0) - s * s * (f32(3.0) - f32(2.0) * s)).astype(f32)
    keep = ~(geom < f32(0.01))
    xs, ys, xf, yf, geom = xs[keep], ys[keep], xf[keep], yf[keep], geom[keep]
    n = xs.size
    if n == 0:
        return out, 0
    ref = src[ys, xs].astype(f32)
    sums = np.zeros((n, 4), f32)
    wtot = np.zeros(n, f32)
    for i in range(32):
        sx = as_i32(rs_round(xf + offs[2 * i]))
        sy = as_i32(rs_round(yf + offs[2 * i + 1]))
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        ux, uy = np.where(ok, sx, 0), np.where(ok, sy, 0)
        ok &= mask[uy, ux] == 0
        if not ok.any():
            continue
        sp = src[uy, ux].astype(f32)
        dr, dg, db = sp[:, 0] - ref[:, 0], sp[:, 1] - ref[:, 1], sp[:, 2] - ref[:, 2]
        arg = -(dr * dr + dg * dg + db * db) / f32(2500.0)
        wc = np.zeros(n, f32)
        wc[ok] = expf(arg[ok])
        for c in range(4):
            sums[:, c] = np.where(ok, sums[:, c] + sp[:, c] * wc, sums[:, c])
        wtot = np.where(ok, wtot + wc, wtot)
    keep = ~(wtot < f32(1e-6))
    with np.errstate(divide="ignore", invalid="ignore"):
        filled = as_u8(np.clip(sums[:, :3] / wtot[:, None], f32(0.0), f32(255.0))).astype(f32)
    existing = out[ys, xs]
    ea = existing[:, 3].astype(f32) / f32(255.0)
    keep &= geom >= ea
    ex = existing[:, :3].astype(f32)
    new = np.empty((n, 4), np.uint8)
    new[:, :3] = as_u8(np.clip(ex + (filled - ex) * geom[:, None], f32(0.0), f32(255.0)))     # lerp_u8
    new[:, 3] = as_u8(geom * f32(255.0))
    before = out[ys[keep], xs[keep]].copy()
    out[ys[keep], xs[keep]] = new[keep]
    return out, int((before != new[keep]).any(-1).sum())


def instant_list(src, mask, out, dabs):
    """a dab list applied in order; dabs = (cx, cy, brush_radius, sample_radius, hardness) rows.  (image, pixels that differ from `out`)"""
    cur = np.array(out, np.uint8, copy=True)
    for d in dabs:
        cur, _ = instant(src, mask, cur, *d)
    return cur, int((cur != np.asarray(out)).any(-1).sum())


# ---------------------------------------------------------------------------------------------------------------- PatchMatch

def ssd_sequential(img, mask, ax, ay, bx, by, half, min_valid):
    """patch_ssd_masked :238-285, line by line"""
    h, w = mask.shape
    ssd = f32(0.0)
    count = 0
    for dy in range(-half, half + 1):
        for dx in range(-half, half + 1):
            apx, apy, bpx, bpy = ax + dx, ay + dy, bx + dx, by + dy
            if apx < 0 or apy < 0 or apx >= w or apy >= h:
                continue
            if bpx < 0 or bpy < 0 or bpx >= w or bpy >= h:
                continue
            if mask[apy, apx] > 0 or mask[bpy, bpx] > 0:
                continue
            for c in range(3):
                d = f32(img[apy, apx, c]) - f32(img[bpy, bpx, c])
                ssd = ssd + d * d
            count += 1
    return F32_MAX if count < min_valid else ssd / f32(count)


class _Counters:
    def __init__(self):
        self.peels = self.big_sums = self.unfilled = self.ssd_calls = 0


def _ssd(img, mask, ax, ay, bx, by, half, min_valid, counters):
    """patch_ssd_masked with the addends summed as integers: every addend d*d is an integer and the running sum only grows, so while the total is below 2^24
    every partial f32 sum is exact and equals the integer; at or beyond, the sequential f32 routine decides (tests hold the two forms equal)."""
    h, w = mask.shape
    counters.ssd_calls += 1
    lo_x = max(-half, -ax, -bx)
    hi_x = min(half, w - 1 - ax, w - 1 - bx)
    lo_y = max(-half, -ay, -by)
    hi_y = min(half, h - 1 - ay, h - 1 - by)
    if lo_x > hi_x or lo_y > hi_y:
        return F32_MAX
    ma = mask[ay + lo_y:ay + hi_y + 1, ax + lo_x:ax + hi_x + 1]
    mb = mask[by + lo_y:by + hi_y + 1, bx + lo_x:bx + hi_x + 1]
    ok = (ma == 0) & (mb == 0)
    count = int(ok.sum())
    if count < min_valid:
        return F32_MAX
    pa = img[ay + lo_y:ay + hi_y + 1, ax + lo_x:ax + hi_x + 1, :3].astype(np.int64)
    pb = img[by + lo_y:by + hi_y + 1, bx + lo_x:bx + hi_x + 1, :3].astype(np.int64)
    d = pa - pb
    total = int(((d * d).sum(-1) * ok).sum())
    if total >= 1 << 24:
        counters.big_sums += 1
        return ssd_sequential(img, mask, ax, ay, bx, by, half, min_valid)
    return f32(total) / f32(count)


def _is_boundary(mask):
    hole = mask != 0
    clear = ~hole
    nb = np.zeros_like(hole)
    nb[:, 1:] |= clear[:, :-1]
    nb[:, :-1] |= clear[:, 1:]
    nb[1:, :] |= clear[:-1, :]
    nb[:-1, :] |= clear[1:, :]
    return hole & nb


def _unit(rng):
    """(rng >> 33) as f32 / (u32::MAX as f32)"""
    return f32(rng >> 33) / f32(4294967296.0)


def _pass(img, mask, pixels, ox, oy, sd, half, min_valid, max_radius, it, counters):
    """patchmatch_pass :289-386"""
    h, w = mask.shape
    forward = it % 2 == 0
    for hx, hy in (pixels if forward else reversed(pixels)):
        best_ox, best_oy, best = int(ox[hy, hx]), int(oy[hy, hx]), sd[hy, hx]
        for ndx, ndy in (((-1, 0), (0, -1)) if forward else ((1, 0), (0, 1))):
            nx, ny = hx + ndx, hy + ndy
            if nx < 0 or ny < 0 or nx >= w or ny >= h:
                continue
            if sd[ny, nx] == F32_MAX:
                continue
            cx, cy = hx + int(ox[ny, nx]), hy + int(oy[ny, nx])
            if cx < 0 or cy < 0 or cx >= w or cy >= h:
                continue
            if mask[cy, cx] > 0:
                continue
            s = _ssd(img, mask, hx, hy, cx, cy, half, min_valid, counters)
            if s < best:
                best, best_ox, best_oy = s, cx - hx, cy - hy
        rng = (hx * LCG_MUL + hy * 982451653 + it * 1234567891) & MASK64
        search_r = f32(max_radius)
        while search_r >= f32(1.0):
            rng = (rng * LCG_MUL + 1442695040888963407) & MASK64
            ra = _unit(rng)
            rng = (rng * LCG_MUL + 1442695040888963407) & MASK64
            rb = _unit(rng)
            cx = int(as_i32(rs_round(f32(hx) + f32(best_ox) + (ra * f32(2.0) - f32(1.0)) * search_r)))
            cy = int(as_i32(rs_round(f32(hy) + f32(best_oy) + (rb * f32(2.0) - f32(1.0)) * search_r)))
            if 0 <= cx < w and 0 <= cy < h and mask[cy, cx] == 0:
                s = _ssd(img, mask, hx, hy, cx, cy, half, min_valid, counters)
                if s < best:
                    best, best_ox, best_oy = s, cx - hx, cy - hy
            search_r = search_r * f32(0.5)
        ox[hy, hx], oy[hy, hx], sd[hy, hx] = best_ox, best_oy, best


def patchmatch(src, hole_mask, patch_size, iterations, trace=None):
    """fill_region_patchmatch :394-520: (image, {"peels", "big_sums", "unfilled", "ssd_calls"}).  `trace`, a list, receives every peel's boundary pixels
    [(x, y)] in scan order: a read-only tap the tests derive structural conditions from"""
    src = np.ascontiguousarray(src, np.uint8)
    hole_mask = np.ascontiguousarray(hole_mask, np.uint8)
    h, w = hole_mask.shape
    ps = max(int(patch_size), 3)
    half = ps // 2
    min_valid = max((half * 2 + 1) ** 2, 4) // 4
    max_radius = f32(max(w, h))
    out = src.copy()
    live = hole_mask.copy()
    ox = np.zeros((h, w), np.int64)
    oy = np.zeros((h, w), np.int64)
    sd = np.full((h, w), F32_MAX, f32)
    k = _Counters()
    sy_, sx_ = np.nonzero(hole_mask == 0)          # row-major
    source = list(zip(sx_.tolist(), sy_.tolist()))
    if not source:
        return out, vars(k)
    pm_iters = 2 if iterations <= 3 else 4
    for _ in range((max(w, h) + 1) * 2):
        by_, bx_ = np.nonzero(_is_boundary(live))
        boundary = list(zip(bx_.tolist(), by_.tolist()))
        if not boundary:
            break
        k.peels += 1
        if trace is not None:
            trace.append(list(boundary))
        src_count = len(source)
        for hx, hy in boundary:
            sx, sy = source[(hx * 7919 + hy * 6271) % src_count]
            ox[hy, hx], oy[hy, hx] = sx - hx, sy - hy
            sd[hy, hx] = _ssd(out, live, hx, hy, sx, sy, half, min_valid, k)
            rng = (hx * 1234567891 + hy * 987654321) & MASK64
            for _i in range(4):
                rng = (rng * LCG_MUL + 1) & MASK64
                tx, ty = source[(rng >> 33) % src_count]
                s2 = _ssd(out, live, hx, hy, tx, ty, half, min_valid, k)
                if s2 < sd[hy, hx]:
                    ox[hy, hx], oy[hy, hx], sd[hy, hx] = tx - hx, ty - hy, s2
        for it in range(pm_iters):
            _pass(out, live, boundary, ox, oy, sd, half, min_valid, max_radius, it, k)
        fills = []
        for hx, hy in boundary:
            sx, sy = hx + int(ox[hy, hx]), hy + int(oy[hy, hx])
            if sd[hy, hx] == F32_MAX or sx < 0 or sy < 0 or sx >= w or sy >= h or live[sy, sx] > 0:
                k.unfilled += 1
                continue
            fills.append((hx, hy, out[sy, sx].copy()))
        for hx, hy, px in fills:
            out[hy, hx] = px
        for hx, hy in boundary:
            live[hy, hx] = 0
            source.append((hx, hy))
    return out, vars(k)
