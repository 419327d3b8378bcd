"""The floating selection's test cases, shared by tests/test_overlay_model_host.py (no device) and tests/test_gpu_overlay.py.

The smallest shapes that still cross a 64-column wave edge and a 256-thread block edge (widths 130 and 257, box heights that are no multiple of 4), with
clipping on all four sides, an empty box, a one-pixel scaled image and a source larger than the canvas.  The model's results are computed once per
(case, anti-aliasing, mode) and shared."""
import functools

import numpy as np

from . import overlay_model as M

ALPHAS = np.array([0, 0, 1, 128, 200, 255, 255], np.uint8)


def image(w, h, seed):
    """uniform bytes, then alpha redrawn from ALPHAS: transparent, nearly transparent, partial and opaque pixels"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = rng.choice(ALPHAS, (h, w))
    return img


def layer(w, h):
    return image(w, h, 1)


def source(w, h):
    return image(w, h, 2)


def overwrite_mask(w, h):
    return ((np.random.default_rng(3).random((h, w)) < 0.6) * 255).astype(np.uint8)


# name: (canvas, source, centre, the rest of M.overlay's arguments)
CASES = {
    "identity-1x1": ((67, 5), (1, 1), (33.5, 2.5), {}),
    "aligned-copy": ((130, 70), (64, 64), (52.0, 36.0), {}),
    "half-pixel": ((130, 70), (65, 33), (60.0, 30.0), {}),
    "rot-0.3": ((130, 70), (65, 33), (61.25, 33.5), dict(rotation=0.3)),
    "rot-quarter-anchor": ((130, 70), (65, 33), (70.0, 35.0), dict(rotation=1.5707964, anchor=(-20.0, 9.5))),
    "off-top-left": ((130, 70), (64, 64), (3.0, -2.5), dict(rotation=-0.7)),
    "off-bottom-right": ((130, 70), (64, 64), (128.0, 69.0), dict(rotation=2.4)),
    "wholly-outside": ((130, 70), (20, 20), (-40.0, 200.0), dict(rotation=0.5)),
    "shrink-lanczos": ((130, 70), (65, 33), (64.0, 35.0), dict(rotation=0.3, scale=(0.5, 0.75), interpolation="lanczos3")),
    "grow-bicubic": ((257, 67), (65, 33), (120.5, 30.25), dict(rotation=-0.2, scale=(2.0, 1.5), interpolation="bicubic")),
    "to-one-pixel": ((67, 5), (65, 33), (30.0, 2.0), dict(rotation=0.9, scale=(0.001, 0.001))),
    "covers-canvas": ((67, 5), (64, 64), (33.0, 2.0), dict(rotation=0.1, scale=(3.0, 3.0), interpolation="nearest")),
}
NAMES = list(CASES)
MODES = ["blend", "overwrite", "overwrite-masked"]
BRANCHY = ["half-pixel", "rot-0.3", "rot-quarter-anchor", "off-top-left", "off-bottom-right"]   # the cases the non-vacuity conditions are stated on


def overlay_of(name, anti_aliasing=True, mode="blend", **changes):
    (cw, ch), (sw, sh), centre, rest = CASES[name]
    return M.overlay(sw, sh, cw, ch, centre, anti_aliasing=anti_aliasing, overwrite_transparent=mode != "blend", **dict(rest, **changes))


def inputs(name, mode="blend"):
    """layer, source, overwrite mask (None unless the mode is the masked one)"""
    (cw, ch), (sw, sh), _, _ = CASES[name]
    return layer(cw, ch), source(sw, sh), overwrite_mask(sw, sh) if mode == "overwrite-masked" else None


@functools.lru_cache(maxsize=None)
def committed(name, anti_aliasing, mode):
    """the model's commit: (image, branch counts); callers do not modify it"""
    base, src, mask = inputs(name, mode)
    out, stats = M.commit(overlay_of(name, anti_aliasing, mode), src, base, mask)
    out.setflags(write=False)
    return out, stats


@functools.lru_cache(maxsize=None)
def previewed(name, own_scale):
    (_, _), (sw, sh), _, _ = CASES[name]
    out = M.preview(overlay_of(name) if own_scale else overlay_of(name, scale=(1.0, 1.0)), source(sw, sh))
    out.setflags(write=False)
    return out


def selection(w, h, seed=4, values=(0, 0, 1, 7, 255, 255)):
    return np.random.default_rng(seed).choice(np.array(values, np.uint8), (h, w))
