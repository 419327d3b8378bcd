"""Inputs of the libm-model tests (tests/test_gpu_libm_model.py on the device, tests/test_libm_model_host.py on the host):
the effects and the Liquify dabs whose kernels evaluate a transcendental per pixel.  One module, so the host test's
discrimination checks run on exactly the inputs the GPU test compares."""
from __future__ import annotations

import math

import numpy as np

from . import inputs as I

# ---------------------------------------------------------------- twist
TWIST_ANGLES = [0.0, 45.0, -45.0, -300.0, 3000.0, -3000.0]
TWIST_ORIGINS = [(0.5, 0.5), (0.37, 0.81), (0.0, 1.0), (1.0, 0.0), (1.7, -0.4)]   # inside, on the border, off the canvas (clamped)
TWIST_SHAPES = [(203, 117), (256, 64), (1, 1), (1, 77), (300, 1)]


def image(w, h, seed):
    return I.random_rgba(w, h, seed)


def selection(w, h, seed):
    return (np.random.default_rng(seed).random((h, w)) < 0.6).astype(np.uint8) * 255


def twist_cases(angle):
    """(img, kwargs, mask) for one angle: every shape x origin, without and with a selection"""
    out = []
    for (w, h) in TWIST_SHAPES:
        img = image(w, h, 3 * w + h)
        for origin in TWIST_ORIGINS:
            for masked in (False, True):
                out.append((img, dict(angle_deg=angle, origin=origin), selection(w, h, w + h) if masked else None))
    return out


# ---------------------------------------------------------------- add_noise (gaussian)
NOISE_W, NOISE_H = 203, 117
NOISE_SCALES = [1.0, 3.7, 0.01]


def _hash_u32(x):
    x = x * np.uint32(0x9E3779B9); x ^= x >> np.uint32(16)
    x = x * np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13)
    x = x * np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)
    return x


def hash24(qx, qy, seed):
    """effects.rs hash_f32's integer part: hash_f32 = hash24 / 2^24"""
    with np.errstate(over="ignore"):
        qx = np.asarray(qx, np.uint32)
        qy = np.asarray(qy, np.uint32)
        return _hash_u32(qx * np.uint32(374761393) + qy * np.uint32(668265263) + np.uint32(seed)) & np.uint32(0xFFFFFF)


def noise_seeds():
    """six seeds whose scale-1 canvas (q = pixel) holds the edges of the Box-Muller draw: two where hash_f32 falls under
    the 1e-4 clamp of u1, two where u2 lies within 2^-20 of 0 and two where it lies within 2^-20 of 1 (a seeded search)"""
    yy, xx = np.mgrid[0:NOISE_H, 0:NOISE_W]
    want = {"u1_clamp": [], "u2_near_0": [], "u2_near_1": []}
    rng = np.random.default_rng(2024)
    while any(len(v) < 2 for v in want.values()):
        seed = int(rng.integers(0, 2 ** 32))
        u1 = hash24(xx, yy, seed)
        u2 = hash24(xx, yy, (seed + 7) & 0xFFFFFFFF)
        hits = {"u1_clamp": (u1 < 1677).any(), "u2_near_0": (u2 < 16).any(), "u2_near_1": (u2 >= (1 << 24) - 16).any()}
        for k, hit in hits.items():
            if hit and len(want[k]) < 2:
                want[k].append(seed)
                break
    return [s for v in want.values() for s in v]


def noise_cases():
    """(img, kwargs, mask): six seeds x three scales, gaussian monochrome, amount 30 and 100, half of them under a selection"""
    img = image(NOISE_W, NOISE_H, 91)
    mask = selection(NOISE_W, NOISE_H, 5)
    out = []
    for i, seed in enumerate(noise_seeds()):
        for j, scale in enumerate(NOISE_SCALES):
            out.append((img, dict(amount=30.0 if (i + j) % 2 else 100.0, noise_type="gaussian", monochrome=True, seed=seed, scale=scale, octaves=1),
                        mask if (i + j) % 3 == 0 else None))
    return out


def noise_knife_edge(O):
    """a gaussian-noise case built so that the glibc and device flavours must round one output byte differently: among the
    scale-1 pixels of the first seed where the two flavours' noise values differ, one whose `amount` can be tuned so that
    r + noise * strength lands between the two values' rounding points.  Returns (img, kwargs) or None."""
    seed = noise_seeds()[0]
    yy, xx = np.mgrid[0:NOISE_H, 0:NOISE_W]
    u1 = np.maximum(hash24(xx, yy, seed).astype(np.float32) / np.float32(16777216.0), np.float32(0.0001)).ravel()
    u2 = (hash24(xx, yy, (seed + 7) & 0xFFFFFFFF).astype(np.float32) / np.float32(16777216.0)).ravel()
    a = (np.float32(2.0) * np.float32(3.14159265358979323846) * u2).astype(np.float32)

    def nv(flavour):
        with O.libm_flavour(flavour):
            lg, cs = O.libm_eval("log", u1), O.libm_eval("cos", a)
        return (np.sqrt((np.float32(-2.0) * lg).astype(np.float32)) * cs * np.float32(0.33)).astype(np.float32)

    g, d = nv("glibc"), nv("device")
    img = image(NOISE_W, NOISE_H, 91)

    def out_byte(base, p):   # round_u8(r + nr): f32 add, then roundf (half away from zero) on a value in (0, 255)
        return math.floor(float(np.float32(np.float32(base) + p)) + 0.5)

    for i in np.flatnonzero(g != d):
        if abs(float(g[i])) < 0.05:
            continue
        base = 25 if g[i] > 0 else 230
        target = 200.5 if g[i] > 0 else -200.5   # base + noise * strength at the rounding point 225.5 / 29.5
        est = np.float32(target / (float(g[i]) + float(d[i])) * 2.0 * 100.0 / 255.0)
        for direction in (np.inf, -np.inf):     # walk the f32 amounts away from the estimate, up then down
            amount = est
            for _step in range(400):
                s = np.float32(np.float32(amount * np.float32(255.0)) / np.float32(100.0))
                if out_byte(base, np.float32(g[i] * s)) != out_byte(base, np.float32(d[i] * s)):
                    y, x = divmod(int(i), NOISE_W)
                    img = img.copy()
                    img[y, x, :3] = base
                    return img, dict(amount=float(amount), noise_type="gaussian", monochrome=True, seed=seed, scale=1.0, octaves=1)
                amount = np.nextafter(amount, np.float32(direction), dtype=np.float32)
    return None


# ---------------------------------------------------------------- reduce_noise, vignette
REDUCE_RADII = [0, 1, 2, 5, 16, 64]
REDUCE_STRENGTHS = [0.0, 0.5, 40.0, 1e4, float("nan")]


def reduce_noise_cases(radius):
    w, h = (70, 50) if radius == 64 else ((120, 80) if radius == 16 else (203, 117))
    img = image(w, h, 40 + radius)
    img[: h // 3, : w // 3] = img[0, 0]                     # a flat patch: equal pixels, range term 0
    out = []
    for k, st in enumerate(REDUCE_STRENGTHS):
        out.append((img, dict(strength=st, radius=radius), selection(w, h, radius) if k % 2 else None))
    return out


VIGNETTE_AMOUNTS = [0.0, 0.8, 2.5]
VIGNETTE_SOFTNESS = [0.0, 0.5, 1.0]


def vignette_cases():
    img = image(203, 117, 12)
    mask = selection(203, 117, 13)
    return [(img, dict(amount=a, softness=s), m) for a in VIGNETTE_AMOUNTS for s in VIGNETTE_SOFTNESS for m in (None, mask)]


# ---------------------------------------------------------------- Liquify dabs (DisplacementField brushes)
def dab_batches():
    """(name, w, h, start field, list of dab batches); a dab is (mode, cx, cy, dx, dy, radius, strength).

    compact: a 300 x 200 field, 70 dabs in the first batch (the kernel culls dabs 64 at a time, so a second round), all five
    modes, overlapping, partly or wholly off the canvas, radius < 1 (clamped to 1) and integer radii whose edge falls on
    pixel centres; then a second batch on the same field.  spread: dabs far apart on a 1700 x 1300 field, which takes the
    chunk launch."""
    rng = np.random.default_rng(12)
    w, h = 300, 200
    dabs = [(int(k % 5), float(rng.uniform(-20, w + 20)), float(rng.uniform(-20, h + 20)), float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8)),
             float(rng.uniform(0.2, 60)), float(rng.uniform(0.1, 1.0))) for k in range(60)]
    dabs += [(0, 16.0, 16.0, 3.0, 0.0, 10.0, 0.8), (1, 100.0, 100.0, 0.0, 0.0, 25.0, 1.0), (2, 150.0, 60.0, 0.0, 0.0, 5.0, 0.9),
             (3, 200.0, 120.0, 0.0, 0.0, 12.0, 0.6), (4, 201.0, 121.0, 0.0, 0.0, 13.0, 0.6), (0, 5000.0, 5000.0, 1.0, 1.0, 10.0, 1.0),
             (0, 40.5, 40.5, -2.0, 1.5, 0.4, 1.0), (3, 80.25, 9.75, 0.0, 0.0, 0.0, 1.0), (1, 299.0, 199.0, 0.0, 0.0, 30.0, 0.7),
             (2, -5.0, 100.0, 0.0, 0.0, 20.0, 1.0)]
    second = [(int(rng.integers(0, 5)), float(rng.uniform(0, w)), float(rng.uniform(0, h)), float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8)),
               float(rng.uniform(3, 40)), float(rng.uniform(0.1, 1.0))) for _ in range(12)]
    start = np.zeros((h, w, 2), np.float32)
    start[::3, ::4] = -0.0
    start[50:90, 30:130] = np.float32(1.25)
    start[120:125, 200:260, 1] = np.float32(-0.75)
    out = [("compact", w, h, start, [dabs, second])]

    w, h = 1700, 1300
    rng = np.random.default_rng(21)
    centres = [(90.0, 80.0), (1600.0, 1210.0), (850.0, 640.0), (1650.0, 70.0), (63.5, 1240.0)]
    sp = []
    for k in range(30):
        cx, cy = centres[k % len(centres)]
        sp.append((int(rng.integers(0, 5)), cx + float(rng.uniform(-30, 30)), cy + float(rng.uniform(-30, 30)), float(rng.uniform(-8, 8)),
                   float(rng.uniform(-8, 8)), float(rng.uniform(5, 70)), float(rng.uniform(0.1, 1.0))))
    start = np.zeros((h, w, 2), np.float32)
    start[::7, ::5] = -0.0
    start[300:310, 400:420] = 3.25
    out.append(("spread", w, h, start, [sp]))
    return out


def oracle_field(O, start, batches):
    f = start.copy()
    for batch in batches:
        for d in batch:
            O.displacement_brush(f, *d)
    return f
