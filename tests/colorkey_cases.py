"""Seeded inputs of the colour-removal tests (tests/test_colorkey_model_host.py, tests/test_gpu_colorkey.py).  No golden of the reference covers colour to alpha
or the Color Remover, so every expectation comes from tests/colorkey_model.py.  Model results are cached: the host test and the GPU test of one session share
them, read-only."""
import functools

import numpy as np

from . import colorkey_model as M
from . import flood_cases as FC

TILE, CHUNK = 64, 32   # the ring kernel's tile edge and levels per launch the sizes below are chosen around (the GPU test checks that the library reports them)


# ---- colour to alpha -------------------------------------------------------------------------------------------------------------------------------------------------
def cta_image(w, h, target, seed=3):
    """colours scattered around `target` with every kind of alpha (0 and 1 included), plus a 64 x 64 block of the exact target colour where it fits"""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 4), np.uint8)
    img[..., :3] = np.clip(np.asarray(target, np.int64)[None, None, :] + rng.integers(-70, 71, (h, w, 3)), 0, 255)
    img[..., 3] = rng.choice(np.array([255, 255, 200, 128, 1, 0], np.uint8), (h, w))
    far = rng.random((h, w)) < 0.1
    img[far, :3] = rng.integers(0, 256, (int(far.sum()), 3))     # and some colours anywhere
    if w >= 74 and h >= 67:
        img[3:67, 10:74, :3] = target
        img[3:67, 10:74, 3] = rng.choice(np.array([255, 255, 128, 1], np.uint8), (64, 64))
    return img


def grey_mask(w, h, seed=8):
    """0 / 1 / 7 / 255: everything but 0 selects"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0, 1, 7, 255, 255], np.uint8), (h, w))


RED, ORANGE = (255, 0, 0), (230, 120, 20)   # a target with zero channels (no spill suppression on them) and one without
# name -> settings; the defaults and each knob varied alone
CTA_SETTINGS = {
    "default": dict(target=RED),
    "strength-half": dict(target=RED, strength=0.5),
    "spill-0": dict(target=RED, spill_suppression=0.0),
    "protect-0": dict(target=RED, protect_luminance=0.0),
    "floor-ceiling": dict(target=RED, alpha_floor=0.2, alpha_ceiling=0.8),
    "tolerance-0-softness-0": dict(target=RED, tolerance=0.0, softness=0.0),    # softness / 255 meets its 0.001 floor: a hard key
    "target-no-zero-channel": dict(target=ORANGE),
}
CTA_SIZES = [(130, 70), (1, 1), (257, 3)]


@functools.lru_cache(maxsize=None)
def cta_expected(name, w, h, masked):
    """(image, mask or None, expected, info), all read-only"""
    s = CTA_SETTINGS[name]
    img = cta_image(w, h, s["target"])
    mask = grey_mask(w, h) if masked else None
    info = {}
    want = M.color_to_alpha(img, mask, info, **s)
    for a in (img, want) + (() if mask is None else (mask,)) + tuple(info.values()):
        a.setflags(write=False)
    return img, mask, want, info


# ---- the Color Remover: the flood test's images -----------------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "checker", "clear", "gradient")
REMOVER_CASES = [c for c in FC.DISTANCE_CASES if c[3] in KINDS]   # 1 x 1, a 200 x 1 row, a 1 x 200 column, 64 x 64, 65 x 65 with seeds on the tile border, 130 x 70
TOLERANCES = (5.0, 15.0, 20.0)
SMOOTHNESS = (0, 3, 20)


def remover_image(case):
    return FC.IMAGES[case[3]](case[1], case[2]), case[4]


@functools.lru_cache(maxsize=None)
def remover_expected(case_name, tolerance, smoothness, contiguous, with_selection=False):
    """(image, seed, selection or None, expected, info)"""
    case = next(c for c in REMOVER_CASES if c[0] == case_name)
    img, seed = remover_image(case)
    sel = FC.selection(case[1], case[2]) if with_selection else None
    info = {}
    want = M.color_removal(img, seed, tolerance, smoothness, contiguous, sel, info)
    for a in (img, want) + (() if sel is None else (sel,)) + tuple(info.values()):
        a.setflags(write=False)
    return img, seed, sel, want, info


# ---- the walled case ---------------------------------------------------------------------------------------------------------------------------------------------------
WALL_W, WALL_H, WALL_SEED, WALL_TOLERANCE = 130, 70, (5, 20), 4.0
WALL_SMOOTHNESS = (0, 1, 20, 32, 33, 70)
WALL_POCKET = (slice(30, 34), slice(10, 20))   # rows, columns of the alpha-0 pocket


def walled_image(seed=1):
    """left 40 columns (250, 10, 10), the rest (10, 250, 250), each +-3 noise, mixed alpha, a 10 x 4 pocket of alpha 0 inside the left block.  The seed pixel is the
    block's base colour, so every pixel of the block is within 3 * 3^2 = 27 < (4 * 2.55)^2 = 104.04 of it: the contiguous core is the whole block"""
    rng = np.random.default_rng(seed)
    img = np.empty((WALL_H, WALL_W, 4), np.uint8)
    img[:, :40, :3] = (250, 10, 10)
    img[:, 40:, :3] = (10, 250, 250)
    img[..., :3] = img[..., :3].astype(np.int16) + rng.integers(-3, 4, (WALL_H, WALL_W, 3))
    img[..., 3] = rng.choice(np.array([255, 255, 200, 128, 1], np.uint8), (WALL_H, WALL_W))
    img[WALL_POCKET][..., 3] = 0
    img[WALL_SEED[1], WALL_SEED[0]] = (250, 10, 10, 255)
    return img


def walled_selection():
    """255 but: column 42 is unselected in rows 0 .. 59 (a wall with a gap at the bottom), columns >= 100 are unselected, and a patch holds 7 (selected)"""
    sel = np.full((WALL_H, WALL_W), 255, np.uint8)
    sel[0:60, 42] = 0
    sel[:, 100:] = 0
    sel[45:66, 50:80] = 7
    return sel


@functools.lru_cache(maxsize=None)
def walled_expected(smoothness, contiguous):
    """(image, selection, expected, info); info has `levels`, `skipped`, `changed`"""
    img, sel = walled_image(), walled_selection()
    info = {}
    want = M.color_removal(img, WALL_SEED, WALL_TOLERANCE, smoothness, contiguous, sel, info)
    for a in (img, sel, want) + tuple(info.values()):
        a.setflags(write=False)
    return img, sel, want, info


def ring_launches(smoothness, chunk=CHUNK):
    return (smoothness + chunk - 1) // chunk
