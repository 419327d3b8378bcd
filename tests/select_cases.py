"""Seeded inputs of the selection tests (tests/test_select_model_host.py, tests/test_gpu_select.py).  Every expectation comes from tests/select_model.py; model
results are cached, so the host test and the GPU test of one session share them.  Sizes are (w, h)."""
import functools

import numpy as np

from . import select_model as M

# what the kernels are built around (the GPU test checks that the library reports the same): the pixels a row-walking workgroup takes per step — a row segment
# is a multiple of it —, the rows of the feather's smallest vertical band, the shape kernel's bytes per lane
SEG, BAND, VEC = 256, 32, 4
SIZES = [(1, 1), (1, 97), (97, 1), (63, 5), (64, 64), (65, 66), (130, 70), (259, 131)]
BIG = (65, 66)          # the size that also gets a radius beyond both of its sides
NAN = float("nan")


def size_id(size):
    return f"{size[0]}x{size[1]}"


def random_bytes(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------------------------
def rect_cases(w, h):
    return [(0, 0, w // 2, h // 2),                      # left and top borders
            (w // 2, h // 2, w - 1, h - 1),              # right and bottom borders
            (0, 0, w - 1, h - 1),                        # all four
            (w // 3, h // 3, w + 10, h + 10),            # max past the canvas
            (0, 0, 0xFFFFFFFF, 0xFFFFFFFF),
            (5, 0, 2, h - 1),                            # min > max
            (0, h, w - 1, h - 1),                        # min_y > clamped max_y
            (w, 0, w + 5, h - 1)]                        # min_x >= w


def ellipse_cases(w, h):
    return [(w / 2 + 0.25, h / 2 - 0.5, 33.3, 20.7),     # fractional centre and radii
            (w / 3, h / 3, 9.5, 4.25),
            (w / 2, h / 2, 4.25, 33.3),
            (-5.5, h / 2, 20.7, 9.5),                    # the centre outside on each side
            (w + 3.0, h + 2.0, 33.3, 20.7),
            (w / 2, -40.0, 9.5, 20.7),                   # wholly outside: the box's max clamps to row 0
            (w / 2, h / 2, 1e6, 1e6),                    # everything
            (w / 2, h / 2, 0.0, 9.5),                    # rx = 0
            (w / 2, h / 2, 9.5, -4.25),                  # negative ry
            (w / 2, h / 2, NAN, 9.5),                    # NaN rx
            (NAN, h / 2, 9.5, 9.5)]


def star(w, h, n=1000, seed=3):
    """n vertices alternating between an inner and an outer radius: a row near the centre crosses most spikes"""
    rng = np.random.default_rng(seed)
    ang = np.arange(n) * (2 * np.pi / n)
    rad = np.where(np.arange(n) % 2 == 0, 0.49, 0.04) * min(w, h) * rng.uniform(0.9, 1.0, n)
    return np.stack([w / 2 + rad * np.cos(ang) * (w / min(w, h)), h / 2 + rad * np.sin(ang) * (h / min(w, h))], axis=1).astype(np.float32)


def lasso_cases(w, h):
    tri = np.array([(w * 0.1, h * 0.1), (w * 0.9, h * 0.3), (w * 0.4, h * 0.95)], np.float32)
    return {"triangle": tri,
            "bow-tie": np.array([(2, 2), (w - 3, h - 3), (w - 3, 2), (2, h - 3)], np.float32),
            "half-rows": np.array([(1.0, 2.5), (w * 0.75, 2.5), (w - 1.0, float(h // 2)), (w * 0.5, h // 2 + 0.5), (0.5, float(h - 2))], np.float32),
            "far-outside": np.array([(-500, -300), (w + 700, -200.25), (w + 900.5, h + 400), (w * 0.5, h * 0.5), (-1000.75, h + 800)], np.float32),
            "star": star(w, h),
            "n0": tri[:0], "n1": tri[:1], "n2": tri[:2]}


@functools.lru_cache(maxsize=None)
def lasso_raw(size, name):
    """(the polygon's raw 0 / 255 mask, the largest crossing count of a row)"""
    counts = []
    raw = M.lasso_raw(size[0], size[1], lasso_cases(*size)[name], counts)
    raw.setflags(write=False)
    return raw, max(counts)


# ---- expand / contract -----------------------------------------------------------------------------------------------------------------------------------------
MORPH_RADII = [0, 1, 2, 5, 17, -4]
BIG_RADIUS = 70         # >= max(BIG)
RAMP = np.array([0, 1, 127, 128, 200, 255], np.uint8)


def morph_masks(w, h):
    corners = np.zeros((h, w), np.uint8)
    corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = 255
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(7)
    sparse = np.where(rng.random((h, w)) < 0.02, rng.integers(0, 256, (h, w)), 0).astype(np.uint8)
    return {"corners": corners, "corner-holes": 255 - corners, "ramp": RAMP[(x // 7 + y // 5) % 6], "full": np.full((h, w), 255, np.uint8),
            "empty": np.zeros((h, w), np.uint8), "sparse": sparse, "sparse-holes": np.where(sparse > 127, 0, 255 - sparse // 2).astype(np.uint8)}


def morph_radii(size):
    return MORPH_RADII + ([BIG_RADIUS] if size == BIG else [])


@functools.lru_cache(maxsize=None)
def morph_expected(size, name, op, radius):
    return (M.expand if op == "expand" else M.contract)(morph_masks(*size)[name], radius)


# ---- feather -----------------------------------------------------------------------------------------------------------------------------------------------------
FEATHER_RADII = [-3.0, 0.4, 1.0, 2.9, 5.0, 9.0]
BIG_FEATHER = 70.0      # on BIG: the window is wider than the image, 35 passes


def feather_masks(w, h):
    y, x = np.mgrid[0:h, 0:w]
    disc = np.where((x - w / 2) ** 2 + (y - h / 2) ** 2 <= (0.35 * max(min(w, h), 4)) ** 2, 255, 0).astype(np.uint8)
    corner = np.zeros((h, w), np.uint8)
    corner[h - 1, w - 1] = 255
    return {"disc": disc, "corner": corner, "random": random_bytes(w, h, 13)}


def feather_radii(size):
    return FEATHER_RADII + ([BIG_FEATHER] if size == BIG else [])


@functools.lru_cache(maxsize=None)
def feather_expected(size, name, radius):
    return M.feather(feather_masks(*size)[name], radius)


# ---- fill / delete -----------------------------------------------------------------------------------------------------------------------------------------------
def grey_mask(w, h):
    """a 16 x 16 ramp of every byte value, tiled (a thin image gets the ramp along its long side)"""
    if w >= 16 and h >= 16:
        return np.tile(np.arange(256, dtype=np.uint8).reshape(16, 16), ((h + 15) // 16, (w + 15) // 16))[:h, :w].copy()
    return (np.arange(w * h) % 256).astype(np.uint8).reshape(h, w)


def layer(w, h, seed=17):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
