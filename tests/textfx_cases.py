"""Shared inputs and cases of the text-style tests (tests/test_textfx_model_host.py, tests/test_gpu_textfx.py).  The text-like input is a seeded handful of
soft-edged rings: alpha with a one-to-two pixel ramp on both rims (glyph edges), random rgb, rgb zero where alpha is zero.  Expected images come from
tests/textfx_model.py once per (case, size) and are shared; nothing here needs a device."""
import functools

import numpy as np

from . import textfx_model as M

SIZES = [(67, 5), (131, 70), (200, 133)]       # odd width above one tile and fewer rows than any radius | two tile seams across, one down | rows of whole dwords
MEASURED = (131, 70)                            # the size the conditions below are stated at
CANVAS = (300, 200)                             # the layer documents


def text_image(w, h, seed=1, box=None, rings=5):
    """(h, w, 4) uint8: `rings` soft rings inside box = (x, y, bw, bh) (the whole image by default), nothing outside it"""
    rng = np.random.default_rng(seed)
    bx, by, bw, bh = box or (0, 0, w, h)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    a = np.zeros((h, w))
    big = max(8.0, 0.35 * min(bw, bh))
    for _ in range(rings):
        cx, cy = bx + rng.uniform(0, bw), by + rng.uniform(0, bh)
        radius, thick, soft = rng.uniform(4.0, big), rng.uniform(3.0, 7.0), rng.uniform(1.0, 2.0)
        d = np.abs(np.hypot(xs - cx, ys - cy) - radius)
        a = np.maximum(a, np.clip((thick / 2 - d) / soft + 0.5, 0.0, 1.0))
    inside = (xs >= bx) & (xs < bx + bw) & (ys >= by) & (ys < by + bh)
    alpha = np.where(inside, np.round(a * 255.0), 0).astype(np.uint8)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = alpha
    img[alpha == 0] = 0
    return img


TEXTURE = np.random.default_rng(77).integers(0, 256, (3, 7, 4), dtype=np.uint8)   # 7 x 3, every alpha


def _tex(**kw):
    return dict(texture_width=7, texture_height=3, **kw)


# name -> (effects, the stage the case is about, what it must do: "draws" | "plain" (equal to the no-effect output at every size) |
#          "plain-small" (equal to it at the sizes in PLAIN_SMALL_SIZES: the shadow is shifted off the image there))
CASES = {
    "defaults": (dict(outline={}, shadow={}, inner_shadow={}), ("outline", "shadow", "inner"), "draws"),
    "center-2.5": (dict(outline=dict(width=2.5, position="center", color=(200, 30, 10, 200))), ("outline",), "draws"),
    "inside-7.3": (dict(outline=dict(width=7.3, position="inside", color=(10, 200, 30, 255))), ("outline",), "draws"),
    "outside-50": (dict(outline=dict(width=50.0, color=(10, 30, 200, 255))), ("outline",), "draws"),
    "outside-0.5": (dict(outline=dict(width=0.5)), ("outline",), "plain"),
    "shadow-spread-unblurred": (dict(shadow=dict(offset_x=-2.5, offset_y=2.5, blur_radius=0.5, spread=0.6, color=(90, 0, 40, 180))), ("shadow",), "draws"),
    "shadow-far": (dict(shadow=dict(offset_x=100.0, offset_y=-100.0, blur_radius=5.0, spread=30.0)), ("shadow",), "plain-small"),
    "shadow-spread-0.5": (dict(shadow=dict(spread=0.5, blur_radius=0.0)), ("shadow",), "draws"),
    "shadow-blur-0.5": (dict(shadow=dict(blur_radius=0.5, color=(0, 60, 90, 200))), ("shadow",), "draws"),
    "shadow-blur-0.51": (dict(shadow=dict(blur_radius=0.51, color=(0, 60, 90, 200))), ("shadow",), "draws"),
    "shadow-spread-30": (dict(shadow=dict(offset_x=3.0, offset_y=-2.0, blur_radius=2.0, spread=30.0, color=(20, 20, 20, 255))), ("shadow",), "draws"),
    "inner-unblurred": (dict(inner_shadow=dict(offset_x=-3.0, offset_y=1.0, blur_radius=0.5, color=(255, 255, 0, 220))), ("inner",), "draws"),
    "inner-blur-50": (dict(inner_shadow=dict(offset_x=0.0, offset_y=0.0, blur_radius=50.0)), ("inner",), "draws"),
    "gradient-repeat": (dict(gradient_fill=dict(angle_degrees=37.0, scale=30.0, offset=(200.5, 90.25), repeat=True, start_color=(255, 0, 0, 255),
                                                end_color=(0, 0, 255, 90))), ("fill",), "draws"),
    "gradient-clamp": (dict(gradient_fill=dict(angle_degrees=37.0, scale=150.0, offset=(60.0, 90.25), start_color=(255, 255, 0, 200), end_color=(0, 80, 255, 255))),
                       ("fill",), "draws"),
    "gradient-scale-0.3": (dict(gradient_fill=dict(angle_degrees=37.0, scale=0.3, offset=(40.0, 20.0), repeat=True, end_color=(0, 128, 0, 128))), ("fill",), "draws"),
    "texture-0.01": (dict(texture_fill=_tex(scale=0.01, offset=(-3.5, -1.25))), ("fill",), "draws"),
    "texture-2.5": (dict(texture_fill=_tex(scale=2.5, offset=(-10.5, -7.0))), ("fill",), "draws"),
    "texture-w0": (dict(texture_fill=dict(texture_width=0, texture_height=3, scale=2.5)), ("fill",), "plain"),
    "gradient-and-texture": (dict(gradient_fill=dict(angle_degrees=90.0, scale=40.0, repeat=True), texture_fill=_tex(scale=2.5)), ("fill",), "draws"),
    "everything": (dict(outline=dict(width=3.0, position="inside", color=(255, 255, 255, 160)), shadow=dict(spread=2.0), inner_shadow={},
                        texture_fill=_tex(scale=1.0, offset=(0.0, 0.0))), ("outline", "shadow", "inner", "fill"), "draws"),
    "none": (dict(), (), "plain"),
}
NAMES = list(CASES)
PLAIN_SMALL_SIZES = [(67, 5), (131, 70)]


def effects_of(name):
    return CASES[name][0]


def texture_of(name):
    return TEXTURE if "texture_fill" in CASES[name][0] else None


@functools.lru_cache(maxsize=None)
def text_of(size):
    img = text_image(size[0], size[1], seed=size[0])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(name, size):
    """(image, counts) of the model for a case at a size; read only"""
    out, counts = M.apply(text_of(size), effects_of(name), texture_of(name))
    out.setflags(write=False)
    return out, counts


# ---- the layer documents: name -> (text, effects) on the CANVAS ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def document(name):
    w, h = CANVAS
    if name == "corner":          # a block in one corner: the region path, and a gradient whose origin is the region's
        return text_image(w, h, seed=5, box=(30, 25, 90, 60)), dict(outline={}, shadow={}, inner_shadow={}, gradient_fill=dict(scale=60.0, angle_degrees=20.0))
    if name == "spread-out":      # text all over the canvas: the full-canvas path
        return text_image(w, h, seed=6, rings=9), dict(outline={}, shadow={}, inner_shadow={})
    if name == "two-edges":       # the block touches the top and the left edge: the region is clamped there
        return text_image(w, h, seed=7, box=(0, 0, 70, 50), rings=6), dict(outline=dict(width=7.3, position="inside"), shadow=dict(spread=3.0))
    if name == "no-text":
        return np.zeros((h, w, 4), np.uint8), dict(outline={}, shadow={}, inner_shadow={})
    raise KeyError(name)


DOCUMENTS = ["corner", "spread-out", "two-edges", "no-text"]


@functools.lru_cache(maxsize=None)
def expected_layer(name):
    text, effects = document(name)
    out, region = M.layer(text, effects)
    out.setflags(write=False)
    return out, region
