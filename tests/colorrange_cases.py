"""Inputs and parameter sets of the histogram, per-band Hue/Saturation and colour-range tests (tests/test_colorrange_model_host.py holds them to what they are
meant to contain, tests/test_gpu_colorrange.py runs them on the device).  Everything is deterministic; images are (h, w, 4) uint8, masks (h, w) uint8."""
import itertools

import numpy as np

# (hue_center, tolerance, sat_min, fuzziness) of select_color_range
RANGE_SETS = [(30.0, 20.0, 0.1, 0.5), (0.0, 45.0, 0.0, 1.0), (200.0, 10.0, 0.3, 0.001), (359.0, 90.0, 0.0, 0.25), (120.0, 0.1, 0.0, 0.7), (60.0, 180.0, 0.0, 0.05),
              (240.0, 33.3, 0.2, 0.9), (90.0, 60.0, 0.0, 0.3), (300.0, 25.0, 0.5, 0.013)]
# the sets with a wide soft edge: a fuzziness of at least 0.25 over a tolerance of at least 10 degrees
SOFT_SETS = [s for s in RANGE_SETS if s[3] >= 0.25 and s[1] >= 10.0]
COMBINE = ("replace", "add", "subtract", "intersect")

_ONE = (40.0, 50.0, -20.0)
_SIX = [(30.0, -40.0, 10.0), (-60.0, 80.0, -15.0), (90.0, 25.0, 30.0), (-120.0, -75.0, -5.0), (150.0, 60.0, 20.0), (-170.0, -20.0, -35.0)]
# name -> (global_hue, global_sat, global_light, bands) of hue_saturation_per_band
BAND_SETS = {"zero": (0.0, 0.0, 0.0, []), "global": (25.0, -30.0, 12.0, [])}
for _i in range(6):
    BAND_SETS[f"band{_i}"] = (0.0, 0.0, 0.0, [(0.0, 0.0, 0.0)] * _i + [_ONE])
BAND_SETS["six"] = (-15.0, 20.0, 5.0, _SIX)
BAND_SETS["max"] = (180.0, 100.0, 100.0, [(180.0, 100.0, 100.0)] * 6)
BAND_SETS["min"] = (-180.0, -100.0, -100.0, [(-180.0, -100.0, -100.0)] * 6)

SMALL_SHAPES = [(1, 1), (3, 5), (67, 129), (257, 3)]   # (w, h): one pixel; below one lane group; odd, several 64 x 64 chunks; wider than tall, w % 4 == 1
BAND_SHAPES = [(67, 129), (257, 3)]
LATTICE_VALUES = list(range(0, 249, 4)) + [255]


def noise(w, h, seed):
    """uniform bytes in all four channels: about one pixel in 256 is fully transparent"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def lattice():
    """the 64^3 lattice r, g, b in {0, 4, .., 248, 255} as 512 x 512, r fastest; alpha 255 but for every 97th pixel (0) and every 5th (128)"""
    v = np.asarray(LATTICE_VALUES, np.uint8)
    i = np.arange(64 ** 3)
    img = np.empty((64 ** 3, 4), np.uint8)
    img[:, 0], img[:, 1], img[:, 2] = v[i % 64], v[(i // 64) % 64], v[i // 4096]
    img[:, 3] = np.where(i % 97 == 0, 0, np.where(i % 5 == 1, 128, 255))
    return img.reshape(512, 512, 4)


def all_colours():
    """every one of the 2^24 rgb values once, alpha 255, as 4096 x 4096"""
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.empty((1 << 24, 4), np.uint8)
    img[:, 0], img[:, 1], img[:, 2], img[:, 3] = i & 255, (i >> 8) & 255, (i >> 16) & 255, 255
    return img.reshape(4096, 4096, 4)


def knee_pixels():
    """every (2k, k, 0), (4k, 3k, 0), (4k, k, 0) and their channel permutations: hues on the multiples of 30 degrees and on 45 and 15 degrees either side of every
    band centre, where band_weight has its knees; alpha 255"""
    out = []
    for k in range(1, 128):
        triples = [(2 * k, k, 0)] + ([(4 * k, 3 * k, 0), (4 * k, k, 0)] if 4 * k <= 255 else [])
        for t in triples:
            out += [p + (255,) for p in itertools.permutations(t)]
    return np.asarray(out, np.uint8)


def fit(pixels, w, h):
    """w * h pixels of an image or a pixel list, taken with a stride coprime to its length so that a small crop still spans the whole list"""
    flat = np.asarray(pixels, np.uint8).reshape(-1, 4)
    n = len(flat)
    step = next(s for s in range(max(n // (w * h), 1) | 1, n + 2, 2) if np.gcd(s, n) == 1)
    return flat[(np.arange(w * h, dtype=np.int64) * step) % n].reshape(h, w, 4).copy()


def with_zero_alpha_chunks(img):
    """the 64 x 64 chunk at rows 64 .. 127, columns 0 .. 63 (where the image has one) made fully transparent with its colours kept — PFX_FROM_FLAT zeroes it, PFX_DENSE
    does not — and a transparent 2 x 2 patch inside a chunk that stays populated"""
    out = img.copy()
    out[64:128, 0:64, 3] = 0
    out[0:2, 0:2, 3] = 0
    return out


def band_inputs():
    """name -> the source pixels of the per-band cases"""
    return {"lattice": lattice(), "noise": noise(256, 256, 11), "knee": knee_pixels()}


def band_image(pixels, w, h):
    return with_zero_alpha_chunks(fit(pixels, w, h))


def selection(w, h, seed):
    """a selection mask: about a third 0, the rest any byte, 1 and 255 among them"""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 256, (h, w), dtype=np.uint8)
    m[rng.random((h, w)) < 0.34] = 0
    flat = m.reshape(-1)
    if flat.size >= 3:
        flat[[0, 1, 2]] = (0, 1, 255)
    return m


def grey_base(w, h):
    """a base mask that holds 0, 1, 127, 128, 254, 255 and everything between"""
    edge = np.asarray([0, 1, 127, 128, 254, 255], np.uint8)
    flat = (np.arange(w * h, dtype=np.int64) * 37 % 256).astype(np.uint8)
    flat[:min(6, flat.size)] = edge[:flat.size]
    return flat.reshape(h, w)


def range_inputs():
    """name -> image of the colour-range cases"""
    return {"noise": noise(256, 256, 5), "lattice": lattice()}
