"""The inputs of tests/test_gpu_gradient.py and the model's answers for them, computed once and shared; tests/test_gradient_model_host.py asserts that they reach
every branch.  Shapes are the smallest at which the kernels can still go wrong: 67 x 5 and 130 x 70 (w % 4 != 0: the pixel arm and its tail; more than one
workgroup), 64 x 8 (the four-pixel arm), 1 x 1, preview scales 2 and 3 (div_ceil; the last column's selection index; 130 / 3 -> 44 columns, a multiple of 4
while w is not), and one case just past the four-pixel arm's grid-stride bound."""
import functools

import numpy as np

from . import gradient_model as M

SIZES = [(67, 5), (130, 70), (64, 8)]
SHAPE_NAMES = ["linear", "reflected", "radial", "diamond"]
# alpha 0 between 0.30 and 0.35, partial alpha around 0.7, stops out of order
STOPS = [(0.7, (10, 20, 200, 128)), (0.0, (255, 0, 0, 255)), (0.35, (0, 0, 255, 0)), (0.3, (0, 255, 0, 0)), (1.0, (255, 255, 255, 255))]
BIG = (4100, 2049)   # 8 400 900 pixels: past 8192 workgroups x 256 lanes x 4 pixels = 8 388 608


@functools.lru_cache(maxsize=None)
def lut():
    table = M.build_lut(STOPS)
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def selection(w, h, kind):
    """kind: 'binary' (0 / 255) or 'grey' (0, 255 and everything between, 1 and 254 among them)"""
    rng = np.random.default_rng(1000 * w + h + (7 if kind == "grey" else 0))
    sel = rng.choice(np.array([0, 255], np.uint8), size=(h, w), p=[0.3, 0.7])
    if kind == "grey":
        grey = rng.integers(1, 255, size=(h, w), dtype=np.uint8)
        sel = np.where(rng.random((h, w)) < 0.5, grey, sel).astype(np.uint8)
    sel.setflags(write=False)
    return sel


def drag(w, h):
    """a drag inside the canvas, neither axis-aligned nor centred: raw runs below 0 on one side and above 1 (above 2 on the wider canvases) on the other"""
    return (w * 0.31 + 0.3, h * 0.24 + 0.2), (w * 0.52 + 0.7, h * 0.71 + 0.4)


def _cases():
    cases = {}
    k = 0
    for w, h in SIZES:
        for shape in range(4):
            for repeat in (False, True):
                for mode in (M.COLOR, M.TRANSPARENCY):
                    start, end = drag(w, h)
                    name = f"{w}x{h}-{SHAPE_NAMES[shape]}-{'repeat' if repeat else 'clamp'}-{'erase' if mode else 'colour'}"
                    cases[name] = dict(w=w, h=h, g=M.gradient(start, end, shape, repeat, mode), sel=[None, "binary", "grey"][k % 3], premul=k % 2 == 0)
                    k += 1
    for shape in range(4):
        cases[f"67x5-degenerate-{SHAPE_NAMES[shape]}"] = dict(w=67, h=5, g=M.gradient((12.5, 2.0), (12.5, 2.0), shape, shape % 2 == 1), sel=None, premul=False)
    cases["1x1"] = dict(w=1, h=1, g=M.gradient((0.0, 0.0), (3.0, 2.0), M.RADIAL), sel="grey", premul=True)
    cases["67x5-scale2"] = dict(w=67, h=5, g=M.gradient(*drag(67, 5), M.LINEAR, True, preview_scale=2), sel="grey", premul=True)
    cases["67x5-scale3"] = dict(w=67, h=5, g=M.gradient(*drag(67, 5), M.DIAMOND, False, preview_scale=3), sel="binary", premul=False)
    cases["130x70-scale3"] = dict(w=130, h=70, g=M.gradient(*drag(130, 70), M.REFLECTED, True, M.TRANSPARENCY, preview_scale=3), sel="grey", premul=True)
    cases["64x8-scale2"] = dict(w=64, h=8, g=M.gradient(*drag(64, 8), M.RADIAL, True, preview_scale=2), sel="binary", premul=True)   # 32 columns: quads, byte-wise selection
    cases["130x70-off-canvas"] = dict(w=130, h=70, g=M.gradient((-300.5, -40.0), (-120.25, -15.0), M.LINEAR, True), sel=None, premul=True)
    cases["67x5-off-canvas"] = dict(w=67, h=5, g=M.gradient((90.0, 12.0), (200.0, -30.0), M.RADIAL, False), sel="grey", premul=False)
    return cases


CASES = _cases()
NAMES = list(CASES)


def selection_of(name):
    c = CASES[name]
    return None if c["sel"] is None else selection(c["w"], c["h"], c["sel"])


@functools.lru_cache(maxsize=None)
def rendered(name):
    """(preview, premultiplied copy, stats) of a case, by the model"""
    c = CASES[name]
    stats = {}
    out = M.render(c["g"], lut(), c["w"], c["h"], selection_of(name), stats)
    pm = M.premultiply(out)
    out.setflags(write=False)
    pm.setflags(write=False)
    return out, pm, stats


@functools.lru_cache(maxsize=None)
def big():
    """the descriptor and the model's preview of the one large case: linear with repeat, one vectorised expression over 8.4 M pixels"""
    w, h = BIG
    g = M.gradient((1000.25, 300.5), (1700.75, 1100.0), M.LINEAR, True)
    out = M.render(g, lut(), w, h)
    out.setflags(write=False)
    return g, out


# ---- commit and apply: full-resolution previews over a layer whose alpha is 0, partial and 255 ----
# (the case whose preview is committed, is_eraser).  The previews are colour-mode ones in both modes: a baked table's alpha stops at 254 (the luminance of
# white truncates to 254), and commit does not care where its preview came from
COMMITS = [("130x70-linear-clamp-colour", False), ("130x70-diamond-repeat-colour", True), ("67x5-diamond-clamp-colour", False), ("67x5-radial-clamp-colour", True),
           ("64x8-radial-clamp-colour", False), ("64x8-linear-clamp-colour", True)]


@functools.lru_cache(maxsize=None)
def layer(w, h, seed=3):
    rng = np.random.default_rng(seed + 100 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    kind = rng.integers(0, 3, (h, w))
    img[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, img[..., 3]))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def committed(name, is_eraser):
    c = CASES[name]
    out = M.commit(layer(c["w"], c["h"]), rendered(name)[0], is_eraser)
    out.setflags(write=False)
    return out


# ---- perspective crop ----
def quads(w, h):
    """name -> corners [TL, TR, BR, BL]"""
    return {"inside": [(w * 0.08 + 0.3, h * 0.08), (w * 0.9 + 0.2, h * 0.18), (w * 0.87 + 0.1, h * 0.92), (w * 0.11 + 0.7, h * 0.84)],
            "beyond": [(-10.5, -3.25), (w + 13.0, -2.0), (w + 8.5, h + 4.0), (-6.0, h + 3.5)],      # corners left of, above and beyond the canvas
            "flipped": [(w * 0.9, h * 0.85), (w * 0.1, h * 0.9), (w * 0.15, h * 0.1), (w * 0.85, h * 0.2)],
            "identity": [(0.0, 0.0), (float(w), 0.0), (float(w), float(h)), (0.0, float(h))]}


def none_quad(w, h):
    return [(w * 0.5, h * 0.5), (w * 0.5 + 1.2, h * 0.5), (w * 0.5 + 1.2, h * 0.5 + 3.0), (w * 0.5, h * 0.5 + 3.0)]   # 1 x 3 after rounding: None


CROP_SIZES = [(67, 5), (130, 70)]
CROP_NAMES = ["inside", "beyond", "flipped", "identity"]


@functools.lru_cache(maxsize=None)
def cropped(w, h, quad, seed=3):
    stats = {}
    out = M.crop(quads(w, h)[quad], layer(w, h, seed), stats)
    out.setflags(write=False)
    return out, stats
