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


# ---- inputs on which every tap of the disc counts (tests/textfx_disc_cases.py has the planes) -------------------------------------------------------------------------
# The rings above saturate under a large maximum and vanish under a large minimum.  `slab` is for the minimum: one opaque block flush with the left, top and
# bottom borders (the outside of the image must not count), a ragged soft edge on its right, a few small holes of distinct partial alpha, the lowest of them
# near the bottom so that the disc's top row alone reaches it from far above; rgb 0, so that a white inside outline shows.  `dots` is for the maximum: the
# `clear` plane as alpha (one pixel of 255 alone in the window of the largest disc, eight lower ones on the border) with random rgb.
SLAB_HOLES = [(0.15, 0.95, 40), (0.42, 0.30, 90), (0.62, 0.62, 140), (0.30, 0.55, 200), (0.75, 0.12, 0)]   # x, y as fractions of the size; alpha


@functools.lru_cache(maxsize=None)
def slab_image(w, h, seed=11):
    rng = np.random.default_rng(seed)
    edge = w - max(6, w // 12) - rng.integers(0, 4, h)                # the last opaque column of each row
    xs = np.arange(w)[None, :]
    alpha = np.clip(np.round((edge[:, None] - xs + 1.5) / 3.0 * 255.0), 0, 255).astype(np.uint8)   # 255 up to the edge, two partial columns, then 0
    for k, (fx, fy, a) in enumerate(SLAB_HOLES):
        x, y = int(fx * w), min(int(fy * h), h - 2)
        alpha[y, x] = a
        if k % 2:                                                   # every other hole is two pixels wide
            alpha[y, x + 1] = a
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 3] = alpha
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def dots_image(seed=12):
    from . import textfx_disc_cases as DC
    alpha = DC.clear(64)
    img = np.random.default_rng(seed).integers(0, 256, alpha.shape + (4,), dtype=np.uint8)
    img[..., 3] = alpha
    img[alpha == 0] = 0
    img.setflags(write=False)
    return img


SLAB_SIZES = [(131, 70), (200, 140)]
DOTS_SIZE = (200, 140)
WHITE = (255, 255, 255, 255)


def _spread(spread, blur):
    return dict(shadow=dict(offset_x=3.0, offset_y=-2.0, blur_radius=blur, spread=spread, color=(20, 20, 20, 180)))


# name -> (image, effects): every one uses the disc, and tests/test_textfx_disc_host.py shows that each would notice a disc with a tap missing
DISC_CASES = {
    **{f"slab-inside-{wd:g}": ("slab", dict(outline=dict(width=wd, position="inside", color=WHITE))) for wd in (3.0, 8.0, 9.0, 30.0, 64.0)},
    "dots-outside-50": ("dots", dict(outline=dict(width=50.0, color=(10, 30, 200, 255)))),
    "dots-outside-64": ("dots", dict(outline=dict(width=64.0, color=(10, 30, 200, 255)))),
    "dots-center-128": ("dots", dict(outline=dict(width=128.0, position="center", color=(200, 30, 10, 200)))),
    "dots-spread-30": ("dots", _spread(30.0, 0.0)),
    "dots-spread-64": ("dots", _spread(64.0, 0.0)),
    "dots-spread-30-blur-2": ("dots", _spread(30.0, 2.0)),
    "dots-spread-64-blur-2": ("dots", _spread(64.0, 2.0)),
}
DISC_RUNS = [(name, size) for name, (image, _) in DISC_CASES.items() for size in (SLAB_SIZES if image == "slab" else [DOTS_SIZE])]


# the outlines of test_the_largest_radius_and_the_two_tile_shapes (tests/test_gpu_textfx.py), which run on the rings and on tile_shape_image(position)
TILE_SHAPE_OUTLINES = [(64.0, "outside"), (128.0, "center"), (64.0, "inside"), (63.2, "outside"), (8.0, "outside"), (8.01, "outside"), (8.0, "inside"), (9.0, "inside"),
                       (16.0, "center"), (16.5, "center")]


def tile_shape_image(position):
    """the slab at the MEASURED size for the erosion, the dots for the dilations"""
    return slab_image(*MEASURED) if position == "inside" else dots_image()


def disc_text(name, size):
    return slab_image(*size) if DISC_CASES[name][0] == "slab" else dots_image()


@functools.lru_cache(maxsize=None)
def expected_disc_case(name, size):
    out, counts = M.apply(disc_text(name, size), DISC_CASES[name][1])
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


# the tight bounds at their extremes, on small canvases: name -> ((w, h), [(x, y)] of the only pixels, each of alpha 1).  One pixel in each corner in turn and
# in all four; the column behind a workgroup's first 256; the row behind the bounds kernel's 2048 workgroups, where its walk over the rows takes a second
# step, and the last row of that canvas; the first and the last pixel of a canvas a little wider than 256
BOUNDS_DOCUMENTS = {
    "top-left": ((300, 200), [(0, 0)]),
    "top-right": ((300, 200), [(299, 0)]),
    "bottom-left": ((300, 200), [(0, 199)]),
    "bottom-right": ((300, 200), [(299, 199)]),
    "four-corners": ((300, 200), [(0, 0), (299, 0), (0, 199), (299, 199)]),
    "column-256": ((300, 8), [(256, 3)]),
    "row-2048": ((5, 2100), [(2, 2048)]),
    "row-2099": ((5, 2100), [(4, 2099)]),
    "first-and-last": ((260, 3), [(0, 0), (259, 2)]),
}
BOUNDS_EFFECTS = dict(outline=dict(width=3.0, color=(10, 30, 200, 255)), shadow=dict(blur_radius=0.0, spread=2.0))


@functools.lru_cache(maxsize=None)
def bounds_document(name):
    (w, h), pixels = BOUNDS_DOCUMENTS[name]
    text = np.zeros((h, w, 4), np.uint8)
    for k, (x, y) in enumerate(pixels):
        text[y, x] = (200 - 40 * k, 100, 50 + 40 * k, 1)
    text.setflags(write=False)
    return text


@functools.lru_cache(maxsize=None)
def expected_bounds_layer(name):
    out, region = M.layer(bounds_document(name), BOUNDS_EFFECTS)
    out.setflags(write=False)
    return out, region


@functools.lru_cache(maxsize=None)
def expected_layer(name):
    text, effects = document(name)
    out, region = M.layer(text, effects)
    out.setflags(write=False)
    return out, region
