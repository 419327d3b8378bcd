"""CPU model of removal by colour (reference: src/ops/color_removal.rs), the yardstick of tests/test_gpu_colorkey.py: no golden of the reference covers these
functions.  A restatement with line citations, in np.float32 throughout: every array operation below rounds once per element like the reference's scalar f32
expression, and nothing passes through f64 but the exact rounding helper.

The Color Remover's steps 1-2 (core and rings) are carried twice: `levels_bfs` transcribes the two queue walks of :196-333, `levels_dilation` grows whole-image
level sets.  tests/test_colorkey_model_host.py holds them to each other.  `levels_tiled` emulates the device's tile / halo / chunk scheme on the CPU."""
from collections import deque

import numpy as np

F = np.float32
NONE = 0xFFFFFFFF   # distance[] = u32::MAX: not in the dilated mask (:263)

DEFAULTS = dict(target=(255, 0, 0), tolerance=18.0, softness=35.0, strength=1.0, spill_suppression=0.35, alpha_floor=0.0, alpha_ceiling=1.0,
                protect_luminance=0.15)   # ColorToAlphaSettings::default :17-30


def _round(v):
    """f32::round (half away from zero) for v >= 0, as a float array: the f64 sum v + 0.5 is exact"""
    return np.floor(np.asarray(v, F).astype(np.float64) + 0.5)


def _as_u8(v):
    """`as u8`: saturating, truncating (no NaN reaches it)"""
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def _clamp(v, lo, hi):
    """f32::clamp for values that are never NaN"""
    return np.minimum(np.maximum(v, F(lo)), F(hi)).astype(F)


def _luma(r, g, b):
    return r * F(0.2126) + g * F(0.7152) + b * F(0.0722)   # :139-141


def prepare(settings):
    """the host-side values of :46-58 as f32 scalars"""
    s = dict(DEFAULTS, **settings)
    p = {"target": [F(int(v)) for v in s["target"][:3]]}
    p["tolerance"] = _clamp(F(s["tolerance"]) / F(255.0), 0.0, 1.0)
    p["softness"] = np.maximum(F(s["softness"]) / F(255.0), F(0.001))
    p["strength"] = _clamp(F(s["strength"]), 0.0, 1.0)
    p["spill"] = _clamp(F(s["spill_suppression"]), 0.0, 1.0)
    p["alpha_floor"] = _clamp(F(s["alpha_floor"]), 0.0, 1.0)
    p["alpha_ceiling"] = _clamp(F(s["alpha_ceiling"]), p["alpha_floor"], 1.0)
    p["protect"] = _clamp(F(s["protect_luminance"]), 0.0, 1.0)
    p["target_luma"] = _luma(*p["target"])
    return p


def color_to_alpha(img, mask=None, info=None, **settings):
    """color_to_alpha_core :32-136.  info (a dict) receives the boolean maps `changed`, `zeroed` (new_a == 0) and `partial` (written with rgb recovered)"""
    img = np.asarray(img, np.uint8)
    p = prepare(settings)
    t = p["target"]
    out = img.copy()
    r, g, b = (img[..., k].astype(F) for k in range(3))
    orig_a = img[..., 3]
    live = orig_a != 0                                                                        # :75
    if mask is not None:
        live &= np.asarray(mask, np.uint8) != 0                                               # :67-71
    max_d = np.maximum(np.maximum(np.abs(r - t[0]) / F(255.0), np.abs(g - t[1]) / F(255.0)), np.abs(b - t[2]) / F(255.0))   # :82-84
    contribution = F(1.0) - _clamp((max_d - p["tolerance"]) / p["softness"], 0.0, 1.0)        # :86
    if p["protect"] > 0:                                                                      # :87-91
        luma_delta = _clamp(np.abs(_luma(r, g, b) - p["target_luma"]) / F(255.0), 0.0, 1.0)
        protection = _clamp(luma_delta * p["protect"], 0.0, 1.0)
        contribution = contribution * (F(1.0) - protection)
    removal = _clamp(contribution * p["strength"], 0.0, 1.0)                                  # :93
    live &= removal > 0                                                                       # :94
    a = np.where(live, orig_a, 255).astype(F) / F(255.0)                                      # (the dead lanes only keep the divisions below defined)
    new_a_f = np.minimum(np.maximum(a * (F(1.0) - removal), p["alpha_floor"]), p["alpha_ceiling"]).astype(F)   # :98-99
    kept = _clamp(new_a_f / a, 0.0, 1.0)                                                      # :100-104
    new_a = _as_u8(_round(new_a_f * F(255.0)))                                                # :105
    zero_rgb = (new_a == 0) | (kept < F(0.001))                                               # :108
    kept_safe = np.where(zero_rgb, F(1.0), kept).astype(F)
    spill_amount = p["spill"] * contribution * (F(1.0) - kept)                                # :123
    keep_factor = F(1.0) - _clamp(spill_amount, 0.0, 1.0)                                     # :148
    rgb = np.zeros(img.shape[:2] + (3,), np.uint8)
    for k, ch in enumerate((r, g, b)):
        v = _clamp((ch - t[k] * removal) / kept_safe, 0.0, 255.0)                             # :115-117
        if p["spill"] > 0 and t[k] > 0:                                                       # :122, :145
            v = v * keep_factor
        rgb[..., k] = _as_u8(_round(v))                                                       # :129-131
    rgb[zero_rgb] = 0                                                                         # :109-111
    out[..., :3][live] = rgb[live]
    out[..., 3][live] = new_a[live]                                                           # :106
    if info is not None:
        info.update(changed=live, zeroed=live & (new_a == 0), partial=live & ~zero_rgb)
    return out


# ---- the Color Remover ---------------------------------------------------------------------------------------------------------------------------------------------
def tol_sq(tolerance):
    t = F(tolerance) * F(2.55)                                                                # :189
    return t * t


def _dist_sq(img, seed_rgb):
    d = img[..., :3].astype(F) - np.asarray(seed_rgb, F)                                      # :429-433 (integers below 2^24: exact)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def passable(img, seed, tolerance, selection=None):
    """what the contiguous flood may enter (:219-235): selected, and fully transparent or within the tolerance"""
    img = np.asarray(img, np.uint8)
    ok = (img[..., 3] == 0) | (_dist_sq(img, img[seed[1], seed[0], :3]) <= tol_sq(tolerance))
    if selection is not None:
        ok &= np.asarray(selection, np.uint8) != 0
    return ok


def is_noop(img, seed, selection=None):
    """:172-187: the reference returns an empty change list"""
    h, w = img.shape[:2]
    if seed[0] >= w or seed[1] >= h:
        return True
    if selection is not None and selection[seed[1], seed[0]] == 0:
        return True
    return img[seed[1], seed[0], 3] == 0


def levels_bfs(img, seed, tolerance, smoothness, contiguous=True, selection=None):
    """:196-333 with its two queues, pixel by pixel: the (h, w) uint32 distance map, NONE = not in the dilated mask"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    sel = None if selection is None else np.asarray(selection, np.uint8)
    near = _dist_sq(img, img[seed[1], seed[0], :3]) <= tol_sq(tolerance)
    alpha = img[..., 3]
    core = np.zeros((h, w), bool)
    if contiguous:                                                                             # :198-237
        core[seed[1], seed[0]] = True
        queue = deque([seed])
        while queue:
            px, py = queue.popleft()
            for nx, ny in ((px - 1, py), (px + 1, py), (px, py - 1), (px, py + 1)):
                if nx < 0 or ny < 0 or nx >= w or ny >= h or core[ny, nx]:
                    continue
                if sel is not None and sel[ny, nx] == 0:
                    continue
                if alpha[ny, nx] == 0 or near[ny, nx]:                                         # :225-235
                    core[ny, nx] = True
                    queue.append((nx, ny))
    else:                                                                                      # :238-256
        core = near & (alpha != 0)
        if sel is not None:
            core &= sel != 0
    dist = np.where(core, 0, NONE).astype(np.uint32)                                           # :264-267
    if smoothness > 0:                                                                         # :269-333
        frontier = deque()
        for y in range(h):
            for x in range(w):
                if not core[y, x]:
                    continue
                for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if nx < 0 or ny < 0 or nx >= w or ny >= h:
                        continue
                    if not core[ny, nx] and dist[ny, nx] == NONE:
                        if sel is not None and sel[ny, nx] == 0:
                            continue
                        dist[ny, nx] = 1
                        frontier.append((nx, ny))
        while frontier:
            px, py = frontier.popleft()
            cur = int(dist[py, px])
            if cur >= smoothness:
                continue
            for nx, ny in ((px - 1, py), (px + 1, py), (px, py - 1), (px, py + 1)):
                if nx < 0 or ny < 0 or nx >= w or ny >= h or dist[ny, nx] != NONE:
                    continue
                if sel is not None and sel[ny, nx] == 0:
                    continue
                dist[ny, nx] = cur + 1
                frontier.append((nx, ny))
    return dist


def _grow4(m):
    """the 4-neighbourhood dilation of a boolean map (without the map itself)"""
    g = np.zeros_like(m)
    g[1:, :] |= m[:-1, :]
    g[:-1, :] |= m[1:, :]
    g[:, 1:] |= m[:, :-1]
    g[:, :-1] |= m[:, 1:]
    return g


def core_dilation(img, seed, tolerance, contiguous=True, selection=None):
    img = np.asarray(img, np.uint8)
    ok = passable(img, seed, tolerance, selection)
    if not contiguous:
        return ok & (img[..., 3] != 0)
    core = np.zeros(img.shape[:2], bool)
    core[seed[1], seed[0]] = True                 # the seed is in the core unconditionally (:201)
    while True:
        new = _grow4(core) & ok & ~core
        if not new.any():
            return core
        core |= new


def rings_dilation(core, smoothness, selection=None):
    """level sets: ring k + 1 is every unreached selected pixel beside ring k"""
    dist = np.where(core, 0, NONE).astype(np.uint32)
    open_ = ~core if selection is None else (~core & (np.asarray(selection, np.uint8) != 0))
    ring = core
    for k in range(1, smoothness + 1):
        ring = _grow4(ring) & open_ & (dist == NONE)
        if not ring.any():
            break
        dist[ring] = k
    return dist


def levels_dilation(img, seed, tolerance, smoothness, contiguous=True, selection=None):
    return rings_dilation(core_dilation(img, seed, tolerance, contiguous, selection), smoothness, selection)


def levels_masked_l1(core, smoothness, selection=None):
    """what the rings are NOT: the plain L1 distance to the core, capped, then cut by the selection"""
    dist = rings_dilation(core, smoothness, None)
    if selection is not None:
        dist[(np.asarray(selection, np.uint8) == 0) & ~core] = NONE
    return dist


def levels_tiled(core, smoothness, selection=None, tile=8, chunk=4):
    """the device's scheme on the CPU: per chunk of at most `chunk` levels, every tile of edge `tile` loads a window with a halo of k pixels (outside the image
    and unselected = blocked), runs k in-window steps and writes back its interior only; the chunks ping-pong between two whole-image maps"""
    h, w = core.shape
    blocked_img = np.zeros((h, w), bool) if selection is None else (np.asarray(selection, np.uint8) == 0)
    cur = np.where(core, 0, NONE).astype(np.uint32)
    base = 0
    while base < smoothness:
        k = min(chunk, smoothness - base)
        nxt = cur.copy()
        for y0 in range(0, h, tile):
            for x0 in range(0, w, tile):
                side = tile + 2 * k
                win = np.full((side, side), NONE, np.uint32)
                blocked = np.ones((side, side), bool)
                ys, xs = np.arange(y0 - k, y0 + tile + k), np.arange(x0 - k, x0 + tile + k)
                iy, ix = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                win[np.ix_(iy, ix)] = cur[np.ix_(ys[iy], xs[ix])]
                blocked[np.ix_(iy, ix)] = blocked_img[np.ix_(ys[iy], xs[ix])]
                for j in range(1, k + 1):
                    win[_grow4(win == base + j - 1) & (win == NONE) & ~blocked] = base + j
                y1, x1 = min(y0 + tile, h), min(x0 + tile, w)
                nxt[y0:y1, x0:x1] = win[k:k + y1 - y0, k:k + x1 - x0]
        cur, base = nxt, base + k
    return cur


def apply_levels(img, seed, dist, smoothness, info=None):
    """step 3, :344-415, then apply_color_removal :421.  info receives the boolean maps `skipped` (the removal < 0.004 rule) and `changed`"""
    img = np.asarray(img, np.uint8)
    out = img.copy()
    sr, sg, sb = (F(int(v)) for v in img[seed[1], seed[0], :3])
    r, g, b = (img[..., k].astype(F) for k in range(3))
    orig_a = img[..., 3]
    live = (dist != NONE) & (orig_a != 0)                                                     # :348, :354
    max_d = np.maximum(np.maximum(np.abs(r - sr) / F(255.0), np.abs(g - sg) / F(255.0)), np.abs(b - sb) / F(255.0))   # :364-367
    removal = F(1.0) - max_d                                                                  # :372
    if smoothness > 0:                                                                        # :375-378
        d = np.where(dist == NONE, 0, dist).astype(F)
        fade = F(1.0) - d / (F(smoothness) + F(1.0))
        removal = np.where(dist > 0, removal * fade, removal).astype(F)
    removal = _clamp(removal, 0.0, 1.0)                                                       # :380
    skipped = live & (removal < F(0.004))                                                     # :381
    live &= ~skipped
    new_a_f = (orig_a.astype(F) / F(255.0)) * (F(1.0) - removal)                              # :386
    new_a = _as_u8(_round(new_a_f * F(255.0)))                                                # :387
    kept = F(1.0) - removal                                                                   # :398
    tiny = kept < F(0.001)                                                                    # :402 (not reachable with new_a != 0)
    kept_safe = np.where(tiny, F(1.0), kept).astype(F)
    rgb = np.zeros(img.shape[:2] + (3,), np.uint8)
    for k, (ch, s) in enumerate(((r, sr), (g, sg), (b, sb))):
        val = (ch - s * removal) / kept_safe                                                  # :405
        val = np.where(val < 0, F(0.0), val)                                                  # round() of a negative stays below 0 and clamps to 0 (:406)
        rgb[..., k] = np.where(tiny, img[..., k], _as_u8(_round(val)))
    gone = new_a == 0                                                                         # :389-393
    rgb[gone] = 0
    out[..., :3][live] = rgb[live]
    out[..., 3][live] = new_a[live]
    if info is not None:
        info.update(skipped=skipped, changed=live)
    return out


def color_removal(img, seed, tolerance, smoothness=3, contiguous=True, selection=None, info=None, levels=levels_dilation):
    """img.clone() then apply_color_removal(compute_color_removal(..)): the tool's result image"""
    img = np.asarray(img, np.uint8)
    if is_noop(img, seed, selection):
        return img.copy()
    dist = levels(img, seed, tolerance, smoothness, contiguous, selection)
    if info is not None:
        info["levels"] = dist
    return apply_levels(img, seed, dist, smoothness, info)
