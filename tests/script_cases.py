"""The script host API's test cases, shared by tests/test_script_model_host.py (no device: the table reaches what it claims) and
tests/test_gpu_script_host_api.py (every program on the device against tests/script_model.py).  No model or oracle code here.

A statement is a tuple.  render() turns it into one line of script text (one statement per line: an error's line number names the statement), and
the model takes the tuple as it is.
  ("print", fn, *args)            print(fn(args));         the console is how a read is observed
  ("closure_map_invert",)         map_channels invert
  ("closure_each_selected",)      for_each_pixel: invert where is_selected(x, y)
  ("closure_region", x, y, w, h)  for_region over the box, returning [b, g, r, a]
  ("fail_div",) ("fail_unknown",) a statement that fails
  (fn, *args)                     fn(args);
edge_rows(w, h) is the hand-written edge table, each row a short fixed program run on every size of SIZES; program(seed) is the seeded generator.
"""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np

# one pixel, single columns and rows, one below / at / one above the 64-column and 4-row tile of permute_kernel, recanvas_kernel and mask_kernel, several
# tiles both ways, a fifth 64-column tile.  No row is impossible at any size: a target below 1 clamps to 1 (so at w = 1 the "shrink" rows keep the width).
SIZES = [(1, 1), (1, 70), (70, 1), (63, 5), (64, 4), (65, 3), (130, 67), (257, 2)]
GEN_SIZES = SIZES + [(97, 61)]
ALPHAS = [0, 0, 1, 128, 200, 255, 255]
MASK_VALUES = [0, 1, 7, 200, 255]
MAX_SIDE = 300    # no generated size-changing statement takes a side above this
SEEDS = range(0, 240)

TRANSFORMS = ["flip_horizontal", "flip_vertical", "rotate_180", "flip_canvas_horizontal", "flip_canvas_vertical", "rotate_canvas_90cw", "rotate_canvas_90ccw",
              "rotate_canvas_180"]
ROT90 = ("rotate_canvas_90cw", "rotate_canvas_90ccw")
ANCHOR_NAMES = ["top-left", "tl", "nw", "top-center", "tc", "n", "top", "top-right", "tr", "ne", "center-left", "cl", "w", "left", "center", "c", "middle",
                "center-right", "cr", "e", "right", "bottom-left", "bl", "sw", "bottom-center", "bc", "s", "bottom", "bottom-right", "br", "se"]
FILTER_NAMES = ["nearest", "bilinear", "bicubic", "lanczos"]
GETTERS = ["get_r", "get_g", "get_b", "get_a"]
SETTERS = ["set_r", "set_g", "set_b", "set_a"]
SCALAR_READS = GETTERS + ["get_pixel"]
SCALAR_WRITES = SETTERS + ["set_pixel"]

# The `_core` effects of the corpus with the test that already holds their entry point to the oracle at tolerance 0, and the parameter draws.  apply_twist and
# apply_noise(_, true) are class LIBM (tests/test_gpu_effects.py) and stay out; apply_motion_blur is not among the issue's candidates.  Nothing was left out
# for want of such a test.
CORE_EFFECTS = {
    "apply_blur": ("tests/test_gpu_parity.py::test_gaussian_identity_and_selection, ::test_exact_gaussian_fused_small_radii (exact mode)", [(0.8,), (2.0,)]),
    "apply_sharpen": ("tests/test_gpu_parity.py::test_sharpen_vs_oracle", [(1.5,), (-0.5,)]),
    "apply_glow": ("tests/test_gpu_parity.py::test_glow_vs_oracle", [(2.0, 0.8), (3.0, 0.5)]),
    "apply_box_blur": ("tests/test_gpu_parity.py::test_box_blur_bitexact", [(r,) for r in range(1, 9)]),
    "apply_median": ("tests/test_gpu_parity.py::test_median_bitexact", [(r,) for r in range(1, 9)]),
    "apply_pixelate": ("tests/test_gpu_parity.py::test_pixelate_bitexact", [(1,), (3,), (8,), (0,)]),
    "apply_reduce_noise": ("tests/test_gpu_effects.py::test_effect_vs_oracle[reduce_noise-*]", [(0.5,), (10.0,)]),
    "apply_vignette": ("tests/test_gpu_effects.py::test_effect_vs_oracle[vignette-*]", [(0.8, 0.5), (2.5, 0.0)]),
    "apply_halftone": ("tests/test_gpu_effects.py::test_effect_vs_oracle[halftone-*]", [(4.0,), (7.5,)]),
    "apply_ink": ("tests/test_gpu_effects.py::test_effect_vs_oracle[ink-*]", [(1.0, 0.5), (35.0, 40.0)]),
    "apply_oil_painting": ("tests/test_gpu_effects.py::test_effect_vs_oracle[oil_painting-*]", [(1,), (3,)]),
    "apply_crystallize": ("tests/test_gpu_effects.py::test_effect_vs_oracle[crystallize-*]", [(5,), (16,)]),
    "apply_bulge": ("tests/test_gpu_effects.py::test_effect_vs_oracle[bulge-*]", [(0.5,), (-1.25,)]),
    "apply_noise": ("tests/test_gpu_effects.py::test_effect_vs_oracle[add_noise-20] (gaussian, colour: the uniform branch)", [(30.0, False)]),
}
INLINE_EFFECTS = [("apply_invert",), ("apply_desaturate",), ("apply_sepia",), ("apply_sepia", 0.25), ("apply_sepia", 7.0), ("apply_brightness_contrast", 20.0, 10.0),
                  ("apply_hsl", 30.0, -20.0, 10.0), ("apply_exposure", 0.5), ("apply_exposure", -0.5), ("apply_levels", 20.0, 230.0, 0.75)]
CHAIN_CAPACITY = 8   # inline effects one chain launch carries


def image(w, h, seed):
    """uniform bytes, then alpha redrawn from ALPHAS (as tests/overlay_cases.py)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = rng.choice(np.array(ALPHAS, np.uint8), (h, w))
    return img


def caller_mask(w, h, seed):
    return np.random.default_rng(7000 + seed).choice(np.array(MASK_VALUES, np.uint8), (h, w))


def _arg(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, str):
        return '"' + v + '"'
    if isinstance(v, float):
        s = repr(v)
        if "e" in s:                      # 1e+200 -> 1.0e200
            m, e = s.split("e")
            return (m if "." in m else m + ".0") + "e" + str(int(e))
        return s
    return str(v)


def render(st):
    k = st[0]
    if k == "print":
        return f"print({st[1]}({', '.join(_arg(v) for v in st[2:])}));"
    if k == "closure_map_invert":
        return "map_channels(|r, g, b, a| [255 - r, 255 - g, 255 - b, a]);"
    if k == "closure_each_selected":
        return "for_each_pixel(|x, y, r, g, b, a| if is_selected(x, y) { [255 - r, 255 - g, 255 - b, a] } else { [r, g, b, a] });"
    if k == "closure_region":
        return f"for_region({', '.join(_arg(v) for v in st[1:])}, |x, y, r, g, b, a| [b, g, r, a]);"
    if k == "fail_div":
        return "let z = 1 / 0;"
    if k == "fail_unknown":
        return "no_such_host_function(1);"
    return f"{k}({', '.join(_arg(v) for v in st[1:])});"


def script(statements):
    return "\n".join(render(st) for st in statements)


def fails_at(statements):
    """the line of the first failing statement, or None"""
    return next((k + 1 for k, st in enumerate(statements) if st[0] in ("fail_div", "fail_unknown")), None)


@dataclass
class Program:
    name: str
    size: tuple          # (w, h)
    image_seed: int
    mask_seed: object    # None: no caller mask
    statements: list

    def inputs(self):
        w, h = self.size
        return image(w, h, self.image_seed), None if self.mask_seed is None else caller_mask(w, h, self.mask_seed)


# ------------------------------------------------------------------------------------------------ the edge table
def corners(w, h):
    return [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]


def probe_mask(w, h):
    """shows the whole selection: has_selection, is_selected on the corners, the centre and just outside, then a fill that paints it into the image"""
    pts = corners(w, h) + [(w // 2, h // 2), (w, 0), (0, h), (-1, 0)]
    return [("print", "has_selection")] + [("print", "is_selected", x, y) for x, y in pts] + [("fill_selected", 9, 8, 7, 6)]


def edge_rows(w, h):
    """(name, statements, caller mask?) for a w x h image"""
    rows = []

    def add(name, sts, mask=False):
        rows.append((name, list(sts), mask))
    size = [("print", "width"), ("print", "height")]
    for t in TRANSFORMS:
        add(t, [(t,)] + size)
        add(t + "-twice", [(t,), (t,)] + size)
    # ---- resize_canvas: every anchor name on a mixed odd change; the centre and the far corner on every kind of change
    for name in ANCHOR_NAMES + ["nowhere", "CENTER", "Bottom-Right", "SE"]:
        add(f"recanvas-{name}", [("resize_canvas", w + 3, h - 3, name)] + size)
    changes = {"grow-even": (4, 6), "grow-odd": (3, 5), "shrink-even": (-2, -4), "shrink-odd": (-3, -1), "mixed-a": (3, -3), "mixed-b": (-3, 3), "mixed-c": (-5, 2),
               "same": (0, 0)}
    for cname, (dw, dh) in changes.items():
        for an in ("center", "br", "top", "left"):
            add(f"recanvas-{cname}-{an}", [("resize_canvas", w + dw, h + dh, an)] + size)
    for an in ("tl", "center", "se"):
        add(f"recanvas-to-1x1-{an}", [("resize_canvas", 0, -3, an)] + size)
        add(f"recanvas-to-32768x1-{an}", [("resize_canvas", 40000, 1, an)] + size)
    # ---- select_rect
    rects = {"negative": (-5, -2, w - 1, h), "beyond": (0, 0, w + 9, h + 70), "inverted": (w, h, 0, 0), "equal": (w // 2, h // 2, w // 2, h // 2),
             "wrap-2^32+5": (0, 0, 4294967296 + 5, 4294967296 + 5), "wrap-2^32+5-low": (4294967296 + 5, 0, w, h), "whole": (0, 0, w, h),
             "inner": (1, 1, w - 1, h - 1), "one-pixel": (w - 1, h - 1, w, h)}
    for rname, r in rects.items():
        add(f"select_rect-{rname}", [("select_rect", *r)] + probe_mask(w, h))
    # ---- select_ellipse
    cx, cy = float(w // 2), float(h // 2)
    ells = {"integer": (cx, cy, 5.0, 3.0), "integer-round": (cx, cy, 5.0, 5.0), "fractional": (w / 2 + 0.25, h / 2 - 0.5, w / 3 + 0.5, h / 3 + 0.5),
            "off-canvas": (-3.0, h + 2.0, 6.0, 6.0), "radius-0-x": (cx, cy, 0.0, 4.0), "radius-0-both": (cx, cy, 0.0, 0.0), "radius-0-fractional": (cx + 0.5, cy, 0.0, 4.0),
            "negative-radius": (cx, cy, -4.0, -2.5), "huge": (cx, cy, 1.0e200, 1.0e200), "huge-x": (cx, cy, 1.0e200, 1.0)}
    for ename, e in ells.items():
        add(f"select_ellipse-{ename}", [("select_ellipse", *e)] + probe_mask(w, h))
    # ---- invert_selection
    add("invert-no-mask", [("invert_selection",)] + probe_mask(w, h))
    add("invert-mask", [("select_rect", 0, 0, w // 2 + 1, h // 2 + 1), ("invert_selection",)] + probe_mask(w, h))
    add("invert-twice", [("select_rect", 0, 0, w // 2 + 1, h // 2 + 1), ("invert_selection",), ("invert_selection",)] + probe_mask(w, h))
    add("invert-no-mask-twice", [("invert_selection",), ("invert_selection",)] + probe_mask(w, h))
    add("invert-caller-mask", [("invert_selection",)] + probe_mask(w, h), mask=True)
    add("invert-caller-mask-twice", [("invert_selection",), ("invert_selection",)] + probe_mask(w, h), mask=True)
    add("invert-after-read", [("print", "is_selected", 0, 0), ("invert_selection",), ("print", "is_selected", 0, 0), ("invert_selection",)] + probe_mask(w, h), mask=True)
    add("caller-mask", probe_mask(w, h), mask=True)
    # ---- fills
    add("fill-clamps", [("fill_selected", 300, -5, 128, 1000)])
    add("fill-clamps-masked", [("fill_selected", 300, -5, 128, 1000)], mask=True)
    add("delete-no-mask", [("delete_selected",)])
    add("delete-caller-mask", [("delete_selected",)], mask=True)
    add("fill-after-clear", [("select_rect", 0, 0, 1, 1), ("clear_selection",), ("print", "has_selection"), ("fill_selected", 1, 2, 3, 4)])
    add("fill-after-clear-caller-mask", [("clear_selection",), ("print", "has_selection"), ("fill_selected", 1, 2, 3, 4)], mask=True)
    # ---- scalar accessors on and just outside each corner
    around = sorted({(x + dx, y + dy) for x, y in corners(w, h) for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))})
    add("accessors", [("print", fn, x, y) for x, y in around for fn in SCALAR_READS + ["is_selected"]], mask=True)
    sts = []
    for k, (x, y) in enumerate(around):
        sts += [(SETTERS[k % 4], x, y, (-7, 256, 1000, -1, 255, 0, 77)[k % 7]), ("print", "get_pixel", x, y)]
    add("setters-out-of-range", sts)
    add("set_pixel-out-of-range", [st for x, y in around for st in (("set_pixel", x, y, 300, -5, 128, 1000), ("print", "get_pixel", x, y))])
    # ---- the mask across a 90 degree rotation: the same bytes read flat at the new width
    for t in ROT90:
        add(f"mask-across-{t}", [("select_rect", 0, 0, w // 2 + 1, h // 2 + 1), (t,)] + probe_mask(w, h)[:-1] + [("apply_box_blur", 1), ("closure_each_selected",),
                                                                                                             ("fill_selected", 9, 8, 7, 6)])
        add(f"caller-mask-across-{t}", [(t,)] + probe_mask(w, h)[:-1] + [("apply_median", 1), ("delete_selected",)], mask=True)
    # ---- the device's rule for a mask of the old size: dropped
    add("stale-mask-resize_canvas", [("select_rect", 0, 0, 1, 1), ("resize_canvas", w + 2, h + 1, "tl"), ("print", "has_selection"), ("fill_selected", 1, 2, 3, 4)])
    add("stale-mask-resize_image", [("select_rect", 0, 0, 1, 1), ("resize_image", w + 2, h + 1, "nearest"), ("print", "has_selection"), ("fill_selected", 1, 2, 3, 4)])
    add("stale-caller-mask-resize_canvas", [("resize_canvas", w + 2, h + 1, "center"), ("print", "has_selection"), ("print", "is_selected", 0, 0),
                                            ("delete_selected",)], mask=True)
    add("kept-mask-same-size-resize", [("select_rect", 0, 0, 1, 1), ("resize_canvas", w, h, "center"), ("resize_image", w, h, "nearest"), ("print", "has_selection"),
                                       ("fill_selected", 1, 2, 3, 4)])
    return rows


def edge_programs():
    out = []
    for k, (w, h) in enumerate(SIZES):
        for j, (name, sts, mask) in enumerate(edge_rows(w, h)):
            out.append(Program(f"{name}@{w}x{h}", (w, h), 100 * k + j, 100 * k + j if mask else None, sts))
    return out


# ------------------------------------------------------------------------------------------------ the generator
class _Gen:
    """draws statements while tracking what a draw needs to know: the size and whether a mask is live"""
    def __init__(self, rng, w, h, mask):
        self.rng, self.w, self.h, self.mask, self.out = rng, w, h, mask, []

    def pick(self, seq):
        return seq[self.rng.randrange(len(seq))]

    def coord(self):
        w, h, r = self.w, self.h, self.rng
        return self.pick([0, w - 1, r.randrange(w), r.randrange(w), r.randrange(w), -1, w]), self.pick([0, h - 1, r.randrange(h), r.randrange(h), r.randrange(h), -1, h])

    def inside(self):
        return self.rng.randrange(self.w), self.rng.randrange(self.h)

    def scalar_write(self):
        x, y = self.inside() if self.rng.random() < 0.8 else self.coord()
        fn = self.pick(SCALAR_WRITES)
        vals = [self.pick([0, 255, 300, -5, self.rng.randrange(256), self.rng.randrange(256)]) for _ in range(4)]
        self.out.append((fn, x, y, *vals) if fn == "set_pixel" else (fn, x, y, vals[0]))

    def scalar_read(self):
        x, y = self.inside() if self.rng.random() < 0.8 else self.coord()
        self.out.append(("print", self.pick(SCALAR_READS), x, y))

    def info_read(self):
        self.out.append(("print", self.pick(["width", "height", "has_selection"])))

    def selected_read(self):
        self.out.append(("print", "is_selected", *(self.inside() if self.rng.random() < 0.8 else self.coord())))

    def transform(self, rot90=False):
        t = self.pick(ROT90) if rot90 else self.pick(TRANSFORMS)
        self.out.append((t,))
        if t in ROT90:
            self.w, self.h = self.h, self.w

    def side(self, old):
        r = self.rng
        return min(max(self.pick([old + r.randrange(-5, 6), old + r.randrange(-5, 6), r.randrange(1, 100), old * 2 + 1, old // 2, old]), 1), MAX_SIDE)

    def resize(self):
        nw, nh = self.side(self.w), self.side(self.h)
        if self.mask and (nw, nh) != (self.w, self.h):
            self.out.append(("clear_selection",))   # a live mask never meets a mask-dependent statement across a size-changing resize
            self.mask = False
        if self.rng.random() < 0.5:
            self.out.append(("resize_canvas", nw, nh, self.pick(ANCHOR_NAMES + ["nowhere", "CENTER"])))
        else:
            self.out.append(("resize_image", nw, nh, self.pick(FILTER_NAMES + ["nn", "Lanczos3", "whatever"])))
        self.w, self.h = nw, nh

    def select(self):
        w, h, r = self.w, self.h, self.rng
        if r.random() < 0.5:
            self.out.append(("select_rect", r.randrange(-3, w + 4), r.randrange(-3, h + 4), r.randrange(-3, w + 4), r.randrange(-3, h + 4)))
        else:
            self.out.append(("select_ellipse", r.randrange(0, 2 * w + 1) / 2.0, r.randrange(0, 2 * h + 1) / 2.0, r.randrange(0, w + 2) / 2.0, r.randrange(0, h + 2) / 2.0))
        self.mask = True

    def selection_change(self):
        k = self.rng.random()
        if k < 0.55:
            self.select()
        elif k < 0.85:
            self.out.append(("invert_selection",))
            self.mask = True
        else:
            self.out.append(("clear_selection",))
            self.mask = False

    def fill(self):
        r = self.rng
        self.out.append(("delete_selected",) if r.random() < 0.3 else ("fill_selected", r.randrange(-20, 300), r.randrange(-20, 300), r.randrange(256), r.randrange(256)))

    def inline(self):
        self.out.append(self.pick(INLINE_EFFECTS))

    def core(self):
        name = self.pick(sorted(CORE_EFFECTS))
        self.out.append((name, *self.pick(CORE_EFFECTS[name][1])))

    def closure(self, selected=False):
        w, h, r = self.w, self.h, self.rng
        k = 1 if selected else r.randrange(6)
        if k == 0:
            self.out.append(("closure_map_invert",))
        elif k == 1:
            self.out.append(("closure_each_selected",))
        elif k == 2:
            self.out.append(("closure_region", 0, 0, w, h))                                                   # the whole image
        elif k == 3:
            self.out.append(("closure_region", w + r.randrange(0, 3), r.randrange(-2, h), 5, 5))              # wholly outside
        elif k == 4:
            self.out.append(("closure_region", r.randrange(-4, 0), r.randrange(-4, h), r.randrange(5, w + 8), r.randrange(1, h + 8)))   # pokes out on the left
        else:
            self.out.append(("closure_region", r.randrange(0, w), r.randrange(0, h), r.randrange(1, w + 4), r.randrange(1, h + 4)))

    def any(self):
        table = [(self.scalar_write, 16), (self.scalar_read, 10), (self.info_read, 3), (self.selected_read, 8), (self.transform, 10), (self.resize, 9),
                 (self.selection_change, 12), (self.fill, 7), (self.inline, 18), (self.core, 8), (self.closure, 9)]
        k = self.rng.randrange(sum(wt for _, wt in table))
        for fn, wt in table:
            if k < wt:
                return fn()
            k -= wt


def program(seed):
    """start size, image seed, optional caller mask and 6 to 14 statements.  seed % 8 picks the flavour: 0 a run of nine or more inline effects, 1 and 5 a mask
    taken across a 90 degree rotation into mask-dependent statements, the others a free draw; seed % 4 == 3 puts a failing statement first, last or in the
    middle, alternately a division by zero and a call of an unknown function."""
    rng = random.Random(seed)
    w, h = GEN_SIZES[rng.randrange(len(GEN_SIZES))]
    has_mask = rng.random() < 0.35
    g = _Gen(rng, w, h, has_mask)
    flavour = seed % 8
    n = 6 + rng.randrange(8)   # 6 .. 13: a failing statement may still join
    if flavour == 0:
        g.scalar_write()
        for _ in range(9 + rng.randrange(3)):
            g.inline()
            if rng.random() < 0.15:
                g.info_read()      # reads that need no image leave the queue alone
        g.pick([g.scalar_read, g.scalar_write, g.transform, g.fill, lambda: None])()
        n = max(n, len(g.out))
    elif flavour in (1, 5):
        if not g.mask or rng.random() < 0.5:
            g.select()
        if rng.random() < 0.5:
            g.selected_read()
        if rng.random() < 0.4:
            g.out.append(("invert_selection",))
        g.transform(rot90=True)
        follow = [g.selected_read, g.core, g.fill, lambda: g.closure(selected=True), lambda: g.out.append(("invert_selection",))]
        for _ in range(3):
            g.pick(follow)()
            if rng.random() < 0.5:
                g.selected_read()
    while len(g.out) < n:
        g.any()
    sts = g.out[:13]
    if seed % 4 == 3:
        k = seed // 4
        pos = (0, len(sts), len(sts) // 2)[k % 3]
        sts.insert(pos, (("fail_div",), ("fail_unknown",))[(k // 3) % 2])
    return Program(f"seed{seed}", (w, h), seed, seed if has_mask else None, sts)


def corpus():
    return [program(s) for s in SEEDS]
