"""The effect bank's edge cases: one table for the host test (tests/test_effect_cases_host.py: the table reaches what it claims, the
oracle stays inside every cap) and the device test (tests/test_gpu_effects_edges.py: every row against the oracle).  No oracle code here.

A row is one effect call (keyword arguments of OracleBackend.effect / GpuBackend.effect) with the sizes and content kinds it runs on and
what is expected of it:
  ORACLE  the device image equals the oracle's (EXACT; LIBM for twist and monochrome gaussian noise);
  STATUS  the call raises PfxError and leaves the destination untouched.  Only for parameters that set a per-pixel loop count or an
          allocation and have a documented bound; `bound` names it and the largest loop count it admits.  Never handed to the oracle.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import inputs as I
from .test_gpu_effects import CASES, SHAPE_CASES

EXACT, LIBM = "exact", "libm"
ORACLE, STATUS = "oracle", "status"

# the smallest sizes that cross every block edge of the bank: 64-wide tiles (w % 64 in {63, 0, 1}), 4-row tiles (h % 4 in {3, 0, 1}), oil painting's 32-row
# walk and crystallize's 64-row tiles (h below, at, above 32 and 64), oil painting's 128 / 256-lane column blocks (w = 129, 257, 300, 513)
SIZES = [(63, 31), (64, 32), (65, 33), (129, 65), (257, 5), (300, 70), (2, 130), (513, 3), (64, 64)]
# alpha_bits_kernel rows are 2 * ceil((w + 32) / 64) + 1 dwords: w + 32 on either side of 64 and of 128
OUTLINE_EXTRA_SIZES = [(31, 40), (32, 40), (33, 40), (96, 6), (97, 6)]
OUTLINE_SIZES = [s for s in SIZES if s[0] <= 129 and s[1] <= 65 and s[0] > 2] + OUTLINE_EXTRA_SIZES
NONFINITE_SIZE = (65, 33)
LIBM_SIZES = sorted(SIZES, key=lambda s: s[0] * s[1])[2:]   # one channel of (2, 130) is 9.6e-4 of the image: the 0.1 % bar needs more pixels

KINDS = ["noise", "white", "clear", "halves", "gradient", "checker1", "checker8", "levels2"]

# levels2: three greys by column, period 3.  An oil window of 2r + 1 columns with r = 1, 4, 7, 10 holds each grey equally often, so with levels = 3 (one bin
# per grey) all bins tie and "first level with the largest count" (artistic.rs:186-195) decides.  Two bins alone cannot tie: a window holds an odd count.
LEVELS2_GREYS = [(10, 20, 30), (130, 110, 120), (200, 100, 240)]   # (r + g + b) / 3 = 20, 120, 180 -> bins 0, 1, 2 of 3


def content(kind: str, w: int, h: int) -> np.ndarray:
    if kind == "noise":
        return I.random_rgba(w, h, 1000 + 7 * w + h)
    img = np.zeros((h, w, 4), np.uint8)
    if kind == "white":
        img[:] = 255
    elif kind == "clear":
        img[..., :3] = 77
    elif kind == "halves":
        img[:, : w // 2] = (255, 0, 128, 255)
        img[:, w // 2:] = (77, 77, 77, 0)
    elif kind == "gradient":
        return I.create_test_gradient(w, h)
    elif kind in ("checker1", "checker8"):
        n = 1 if kind == "checker1" else 8
        yy, xx = np.mgrid[0:h, 0:w]
        img[..., :3] = np.where(((xx // n + yy // n) % 2) == 1, 255, 0)[..., None]
        img[..., 3] = 255
    elif kind == "levels2":
        img[..., :3] = np.array(LEVELS2_GREYS, np.uint8)[np.arange(w) % 3][None, :, :]
        img[..., 3] = 255
    else:
        raise KeyError(kind)
    return img


def selection(w: int, h: int) -> np.ndarray:
    """60 % of the pixels selected, with the values a selection mask can hold; the rule under test is `mask == 0`"""
    rng = np.random.default_rng(500 + 3 * w + h)
    values = rng.choice(np.array([1, 7, 200, 255], np.uint8), size=(h, w))
    return np.where(rng.random((h, w)) < 0.6, values, 0).astype(np.uint8)


@dataclass
class Row:
    effect: str
    kw: dict
    cls: str = EXACT
    expect: str = ORACLE
    sizes: list = field(default_factory=lambda: list(SIZES))
    kinds: list = field(default_factory=lambda: list(KINDS))
    bound: str = ""          # STATUS rows: the documented bound and the largest loop count it admits
    tune: tuple = ()         # (pfx_tune key, value) to run the device under, restored to 1 afterwards

    def cases(self):
        return [(size, kind) for size in self.sizes for kind in self.kinds]


NAN, INF = float("nan"), float("inf")
NONFINITE = [NAN, INF, -INF, 1e30, -1e30, 1e-30]
ALL_MODES = [(m, aa) for m in ("outside", "inside", "center") for aa in (False, True)]
SMALL = [(65, 33), (129, 65)]

# first rows for the four effects of k_effects.hip (no row in CASES)
BASE_EXTRA = {
    "sharpen": dict(amount=1.5, radius=2.0),
    "glow": dict(radius=3.0, intensity=0.8),
    "bokeh_blur": dict(radius=3.0),
    "motion_blur": dict(angle_deg=30.0, distance=8.0),
}

# every float parameter: name, or (name, index) for a component of a tuple
FLOAT_PARAMS = {
    "zoom_blur": ["center_x", "center_y", "strength", "tint_strength", "tint_color"],
    "crystallize": ["cell_size"],
    "dents": ["scale", "amount", "roughness"],
    "bulge": ["amount", ("origin", 0), ("origin", 1)],
    "twist": ["angle_deg", ("origin", 0), ("origin", 1)],
    "add_noise": ["amount", "scale"],
    "reduce_noise": ["strength"],
    "vignette": ["amount", "softness"],
    "halftone": ["dot_size", "angle_deg"],
    "grid": ["opacity"],
    "shadow": ["blur_radius", "opacity"],
    "pixel_drag": ["amount", "direction"],
    "ink": ["edge_strength", "threshold"],
    "color_filter": ["intensity"],
    "contours": ["scale", "frequency", "line_width", "blend"],
    "sharpen": ["amount", "radius"],
    "glow": ["radius", "intensity"],
    "bokeh_blur": ["radius"],
    "motion_blur": ["angle_deg", "distance"],
}

# The float parameters that set a loop count or an allocation, the bound that keeps it finite, and which of the six values it refuses.
# Read from the host code; no other float parameter reaches a kernel as a trip count (octaves, samples, radii and widths are integers with clamps or
# bounds of their own; cell_size only lowers the cell count, ceil(w / max(cs, 2)) * ceil(h / max(cs, 2)), and NaN gives max(NaN, 2) = 2).
GAUSS_BOUND = "gaussian radius ceil(3 sigma) <= 850 (pfx_gauss.cpp:unsupported / pfxk_gauss_max_radius): at most 1701 taps per pass"
STATUS_PARAMS = {
    ("bokeh_blur", "radius"): ({INF, 1e30}, "ceil(radius) <= 1500 (pfx_effects.cpp:pfx_bokeh_blur_dev): at most 3001 spans, ~7.07e6 samples per pixel"),
    ("motion_blur", "distance"): ({INF, 1e30}, "ceil(distance) <= 65536 (pfx_effects.cpp:pfx_motion_blur_dev): at most 131073 samples per pixel"),
    ("sharpen", "radius"): ({INF, 1e30}, GAUSS_BOUND),
    ("glow", "radius"): ({INF, 1e30}, GAUSS_BOUND),
    ("shadow", "blur_radius"): ({INF, 1e30}, GAUSS_BOUND + "; with widen_radius also spread = round(max(blur, 1)) <= 4096 (pfx_shadow_dev), "
                                "a max over at most 2 * 4096 + 1 texels clamped to the image side"),
}


def first_row(effect):
    if effect in BASE_EXTRA:
        return dict(BASE_EXTRA[effect])
    for name, _cls, kw in CASES:
        if name == effect:
            return dict(kw)
    return dict(next(kw for name, kw in SHAPE_CASES if name == effect))


def with_param(kw, param, value):
    kw = dict(kw)
    if isinstance(param, tuple):
        name, idx = param
        t = list(kw.get(name, (0.5, 0.5)))
        t[idx] = value
        kw[name] = tuple(t)
    elif param == "tint_color":
        kw["tint_color"] = (value,) * 4
        kw["tint_strength"] = 0.7
    else:
        kw[param] = value
    return kw


def nonfinite_rows(effect):
    out = []
    for param in FLOAT_PARAMS.get(effect, []):
        refused, bound = STATUS_PARAMS.get((effect, param), (set(), ""))
        for v in NONFINITE:
            kw = with_param(first_row(effect), param, v)
            if effect == "zoom_blur":
                kw.setdefault("tint_color", (0.0, 0.0, 0.0, 0.0))   # spelled out: the C ABI reads a NULL colour as "no tint" whatever the strength
            status = v in refused
            out.append(Row(effect, kw, cls=LIBM if effect == "twist" else EXACT, expect=STATUS if status else ORACLE, sizes=[NONFINITE_SIZE], kinds=["noise"],
                           bound=bound if status else ""))
    return out


def _edge_rows():
    R = Row
    rows = []
    # ---- the rows of test_gpu_effects.py, now on every size and content kind (the heavy ones on fewer)
    for name, cls, kw in CASES:
        heavy = (name == "oil_painting" and kw["radius"] >= 10) or (name == "reduce_noise" and kw["radius"] >= 4) or (name == "zoom_blur" and kw["samples"] >= 32)
        sizes = LIBM_SIZES if cls == LIBM else list(SIZES)
        rows.append(R(name, dict(kw), cls=cls, sizes=sizes, kinds=["noise", "white", "halves"] if heavy else list(KINDS)))
    for name, kw in SHAPE_CASES:
        rows.append(R(name, dict(kw), sizes=OUTLINE_SIZES if name == "outline" else list(SIZES), kinds=["noise", "halves", "clear", "white"]))

    # ---- zoom blur: sample counts with n % 4 in {1, 3} (the gather works in groups of four), the cap, centres on a pixel and off the canvas on each side
    for n in (3, 5, 7):
        rows.append(R("zoom_blur", dict(center_x=0.5, center_y=0.5, strength=0.5, samples=n)))
        rows.append(R("zoom_blur", dict(center_x=0.3, center_y=0.6, strength=0.9, samples=n, tint_color=(0.2, 1.0, 0.4, 0.9), tint_strength=0.5),
                      kinds=["noise", "halves"]))
    rows.append(R("zoom_blur", dict(center_x=0.5, center_y=0.5, strength=0.7, samples=4096), sizes=SMALL, kinds=["noise"]))
    for ts in NONFINITE:                                            # a tint that is on, with a colour
        rows.append(R("zoom_blur", dict(center_x=0.4, center_y=0.6, strength=0.3, samples=8, tint_color=(1.0, 0.5, 0.25, 1.0), tint_strength=ts),
                      sizes=[NONFINITE_SIZE], kinds=["noise", "gradient"]))
    rows.append(R("zoom_blur", dict(center_x=0.25, center_y=0.25, strength=0.6, samples=6), kinds=["noise", "gradient"]))   # cx = w / 4: on a pixel where 4 | w
    for cx, cy in ((-0.5, 0.5), (1.5, 0.5), (0.5, -0.5), (0.5, 1.5)):
        rows.append(R("zoom_blur", dict(center_x=cx, center_y=cy, strength=0.6, samples=5), kinds=["noise", "gradient"]))

    # ---- crystallize: both sides of the 64x4 | 64x64 tile switch at 8.0, the smallest cell, cells larger than a tile, one cell
    for cs in (7.99, 8.0, 8.01, 2.0, 63.9, 1e4):
        rows.append(R("crystallize", dict(cell_size=cs, seed=11), kinds=["noise", "white", "halves", "gradient", "checker1"]))

    # ---- oil painting: the 256 | 128-lane switch at levels 32 | 33, more than one column block, the packed word at saturation (white), exact ties
    for radius, levels in ((10, 64), (10, 33), (10, 32), (10, 2)):
        rows.append(R("oil_painting", dict(radius=radius, levels=levels), kinds=["noise", "white"]))
        rows.append(R("oil_painting", dict(radius=radius, levels=levels), sizes=[(65, 33), (300, 70)], kinds=["halves", "checker1", "checker8", "levels2"]))
    rows.append(R("oil_painting", dict(radius=1, levels=64)))
    rows.append(R("oil_painting", dict(radius=1, levels=3), kinds=["levels2", "checker1"]))     # the tie rows: levels = 3, see LEVELS2_GREYS
    rows.append(R("oil_painting", dict(radius=10, levels=3), kinds=["levels2"]))
    rows.append(R("oil_painting", dict(radius=1, levels=2), kinds=["levels2", "checker1"]))

    # ---- outline: the bit plane | scan switch at search radius width + 1 = 15 | 16, every mode; 64 and the ABI bound 256 in one mode
    for width in (14, 15, 16):
        for mode, aa in ALL_MODES:
            kw = dict(width=width, color=(20, 200, 250, 200), mode=mode, anti_alias=aa)
            rows.append(R("outline", kw, sizes=OUTLINE_SIZES, kinds=["noise", "halves"]))
            rows.append(R("outline", kw, sizes=[(65, 33)], kinds=["clear", "white"]))
            if width < 16:
                rows.append(R("outline", kw, sizes=OUTLINE_SIZES, kinds=["noise", "halves"], tune=("outline_bits", 0)))
    rows.append(R("outline", dict(width=64, color=(250, 20, 20, 255), mode="center", anti_alias=True), sizes=[(65, 33), (33, 40)], kinds=["noise", "halves"]))
    rows.append(R("outline", dict(width=256, color=(250, 20, 20, 255), mode="outside", anti_alias=False), sizes=[(65, 33)], kinds=["halves"]))

    # ---- grid: a line wider than the cell, opacity at both ends
    rows.append(R("grid", dict(cell_w=2, cell_h=2, line_width=5, color=(200, 30, 90, 128), style="lines", opacity=0.5)))
    for op in (0.0, 1.0):
        rows.append(R("grid", dict(cell_w=7, cell_h=13, line_width=3, color=(200, 30, 90, 128), style="lines", opacity=op)))
        rows.append(R("grid", dict(cell_w=5, cell_h=3, line_width=1, color=(10, 250, 60, 255), style="checkerboard", opacity=op), kinds=["noise", "halves"]))

    # ---- canvas border: min(w, h) / 2 and one more (the two bands meet / overlap)
    for (w, h) in SIZES:
        for width in (min(w, h) // 2, min(w, h) // 2 + 1):
            rows.append(R("canvas_border", dict(width=width, color=(255, 0, 0, 255)), sizes=[(w, h)], kinds=["noise", "clear"]))

    # ---- pixel drag: distance 0 | 1 | 4e9 (the drag saturates `as i32`), every row dragged (amount 100) and beyond
    for distance in (0, 1, 4_000_000_000):
        for amount in (100.0, 250.0):
            rows.append(R("pixel_drag", dict(seed=9, amount=amount, distance=distance, direction=37.0), kinds=["noise", "gradient", "halves"]))

    # ---- rgb displace / drop shadow: offsets up to +-2^20 (beyond that the reference's own i32 sums overflow)
    big = 1 << 20
    for r_off, g_off, b_off in (((big, 0), (0, -big), (-big, big)), ((-big, -big), (big, big), (1, -1)), ((63, 0), (-64, 3), (0, -4))):
        rows.append(R("rgb_displace", dict(r_off=r_off, g_off=g_off, b_off=b_off), kinds=["noise", "gradient", "halves"]))
    for ox, oy in ((big, 0), (0, -big), (-big, big), (-63, 3)):
        rows.append(R("shadow", dict(offset_x=ox, offset_y=oy, blur_radius=2.0, widen_radius=True, color=(30, 60, 200, 180), opacity=0.9),
                      kinds=["noise", "halves", "clear"]))
    for blur in (5.33, 5.34):                                       # ceil(3 sigma) = 16 | 17: the fused Gaussian's limit, as plane and as RGBA
        rows.append(R("shadow", dict(offset_x=3, offset_y=-2, blur_radius=blur, widen_radius=False, color=(0, 0, 0, 255), opacity=0.8),
                      kinds=["noise", "halves"]))

    # ---- bokeh: the identity threshold 0.5, the smallest discs, a disc larger than every image
    for radius in (0.49, 0.5, 1.0):
        rows.append(R("bokeh_blur", dict(radius=radius)))
    rows.append(R("bokeh_blur", dict(radius=3.0)))
    rows.append(R("bokeh_blur", dict(radius=100.0), sizes=[(65, 33), (97, 61)], kinds=["noise", "halves"]))

    # ---- motion: the identity threshold 1.0, the bound 65536
    for distance in (0.99, 1.0, 8.0):
        rows.append(R("motion_blur", dict(angle_deg=30.0, distance=distance)))
    rows.append(R("motion_blur", dict(angle_deg=-100.0, distance=40.5), kinds=["noise", "gradient", "halves"]))
    rows.append(R("motion_blur", dict(angle_deg=30.0, distance=65536.0), sizes=[(16, 16)], kinds=["noise", "gradient"]))

    # ---- sharpen / glow: Gaussian radii ceil(3 sigma) = 16 | 17 around the fused kernel's limit, amount / intensity 0 and negative
    for sigma in (2.0, 5.33, 5.34):
        for p in (1.5, 0.0, -0.75):
            kinds = list(KINDS) if sigma == 2.0 else ["noise", "halves", "checker1"]
            rows.append(R("sharpen", dict(amount=p, radius=sigma), kinds=kinds))
            rows.append(R("glow", dict(radius=sigma, intensity=p), kinds=kinds))

    # ---- integer parameters past their documented bounds: a status
    first = {e: first_row(e) for e in ("zoom_blur", "reduce_noise", "outline", "shadow")}
    rows.append(R("zoom_blur", dict(first["zoom_blur"], samples=4097), expect=STATUS, sizes=[NONFINITE_SIZE], kinds=["noise"],
                  bound="samples <= 4096 (pfx_zoom_blur_dev): at most 4096 gathers per pixel"))
    rows.append(R("reduce_noise", dict(first["reduce_noise"], radius=65), expect=STATUS, sizes=[NONFINITE_SIZE], kinds=["noise"],
                  bound="radius <= 64 (pfx_reduce_noise_dev): at most 129 * 129 = 16641 taps per pixel"))
    rows.append(R("outline", dict(first["outline"], width=257), expect=STATUS, sizes=[NONFINITE_SIZE], kinds=["noise"],
                  bound="width <= 256 (pfx_outline_dev): search radius 257, a window of at most 515 * 515 texels clamped to the image"))
    rows.append(R("shadow", dict(first["shadow"], blur_radius=4097.0, widen_radius=True), expect=STATUS, sizes=[NONFINITE_SIZE], kinds=["noise"],
                  bound="spread = round(max(blur, 1)) <= 4096 (pfx_shadow_dev): a max over at most 8193 texels clamped to the image side"))
    return rows


EFFECTS = ["zoom_blur", "crystallize", "dents", "bulge", "twist", "add_noise", "reduce_noise", "vignette", "halftone", "grid", "canvas_border", "shadow",
           "outline", "pixel_drag", "rgb_displace", "ink", "oil_painting", "color_filter", "contours", "sharpen", "glow", "bokeh_blur", "motion_blur"]

_ROWS = None


def all_rows():
    global _ROWS
    if _ROWS is None:
        _ROWS = _edge_rows() + [r for e in EFFECTS for r in nonfinite_rows(e)]
    return _ROWS


def rows(effect):
    return [r for r in all_rows() if r.effect == effect]
