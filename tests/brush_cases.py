"""The brush engine's edge cases: one table for the host test (tests/test_brush_cases_host.py: each row reaches the state it was written for, from the
table and the oracle alone) and the device test (tests/test_gpu_brush_edges.py: every row against the oracle at tolerance 0).  No oracle code here.

A row is one stroke: a canvas size, a target kind, the brush (keyword arguments of make_brush), the stamp centres (or the two ends of a brush_line),
optionally a selection kind and the dynamics (image tip, jitter), the `brush_binning` settings to run the device under, and what the host test asserts
of it (`expect`).  Families, by what they were written for:
  size       radius^2 on both sides of the 0.001 skip, radii below a pixel, around the 64 x 64 chunk and beyond the canvas; hardness 0, 0.37, 1
  gain       colour alpha x flow just above, at and just below the 0.01 cut-off (which the image-tip paint path does not have)
  count      1 .. 193 stamps: both sides of the 64 / 65 switch between the bounding-box and the binned kernel, and every 64-stamp cull group
  order      the 0 .. 255 alpha lattice under stamps of one computed a8 (paint `>=`) and an erase strength that equals a lattice value (eraser `>`)
  tone       Dodge / Burn / Sponge over a colour lattice that takes every branch of the HSL round trip
  tip        image tips of 1 .. 65 and 300 texels, rotations around the 0.01 degree test, degenerate masks
  nonfinite  NaN, +-inf and +-3e9 centres first, in the middle and last in strokes of <= 64 and > 64 stamps
  selection  a mask that is 0 on the chunk borders and on every stamp's box edge
  line       brush_line at the size and hardness extremes, ends on and off the canvas
  radius     one anti-aliased stamp per radius of a sweep over [0.0316, 4096]: the prepared reciprocal of brush_alpha_dev against `/`
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import inputs as I

W, H = 200, 136
COLOR = (0.9, 0.3, 0.1, 0.85)
SIZES = [0.06, 0.0632, 0.0633, 0.07, 0.5, 1.0, 1.5, 2.0, 3.0, 63.0, 64.0, 127.5, 128.0, 129.0, 400.0, 5000.0]
HARDNESS = [0.0, 0.37, 1.0]
KINDS = ["paint", "eraser", "tone"]
GAINS = [  # (colour alpha, flow, on the painted side of `alpha * flow < 0.01` in f32)
    (0.02, 0.6, True), (0.011, 1.0, True), (1.0, 0.0101, True), (0.1, 0.1, True), (0.01, 1.0, True),
    (0.0999, 0.1, False), (0.00999, 1.0, False), (1.0, 0.0099, False)]
COUNTS = [1, 63, 64, 65, 127, 128, 129, 193]
TIP_SIZES = [1, 2, 3, 63, 64, 65]
TIP_ROTATIONS = [0.0, 0.0099, 0.0101, 90.0, 180.0, 270.0, 360.0, -45.0]
NONFINITE = [(np.nan, 10.0), (10.0, np.nan), (np.nan, np.nan), (np.inf, 10.0), (-np.inf, 10.0), (10.0, np.inf), (10.0, -np.inf), (np.inf, -np.inf),
             (3e9, 10.0), (-3e9, 10.0), (10.0, 3e9), (10.0, -3e9)]
FAMILIES = ["size", "gain", "count", "order", "tone", "tip", "nonfinite", "selection", "line", "radius"]


@dataclass
class Row:
    family: str
    name: str
    size: tuple                       # canvas (w, h)
    target: str                       # target(kind, w, h)
    brush: dict
    points: np.ndarray = None         # (n, 2) float32 stamp centres, or
    line: tuple = None                # ((x0, y0), (x1, y1)) for brush_line
    selection: str = None             # selection(kind, row)
    dyn: dict = None
    binning: tuple = (1,)             # `brush_binning` values the device runs under; the results must all be the oracle's
    expect: dict = field(default_factory=dict)

    def __str__(self):
        return f"{self.family}/{self.name}"


# ---------------------------------------------------------------------------------------------------------------------------------- content
def alpha_lattice(w, h):
    """every alpha 0 .. 255 in each 16 x 16 tile, colours random"""
    img = I.random_rgba(w, h, 4000 + w + 3 * h)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 3] = ((xx % 16) + 16 * (yy % 16)).astype(np.uint8)
    return img


def lattice_colors():
    """the colours a tone mode has to get right: greys of every level, the six primaries and secondaries, 0 / 255 in every channel, near-greys whose
    channels differ by 1 (|max - min| = 1/255, far above the 1e-6 test, next to the greys below it), every hue sextant at l below and above 0.5"""
    c = [(v, v, v) for v in range(256)]
    c += [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)]
    for v in (0, 1, 63, 127, 128, 200, 254):
        c += [(v + 1, v, v), (v, v + 1, v), (v, v, v + 1), (v, v + 1, v + 1), (v + 1, v, v + 1), (v + 1, v + 1, v)]
    for lo, hi in ((10, 90), (30, 200), (140, 250), (0, 254), (1, 255), (120, 135)):   # l = (lo + hi) / 510: 0.098, 0.45, 0.76, 0.498, 0.502, 0.5
        mid = (lo + hi) // 2
        c += [(hi, mid, lo), (hi, lo, mid), (mid, hi, lo), (lo, hi, mid), (lo, mid, hi), (mid, lo, hi), (hi, hi - 1, lo), (hi, lo, hi - 1), (hi - 1, hi, lo)]
    return np.array(c, np.uint8)


def color_lattice(w, h):
    """lattice_colors() as a 19 x 19 tile (any 37 x 37 window holds a whole one), every third tile seeded random colours instead; alpha random (tone modes
    leave it alone)"""
    img = I.random_rgba(w, h, 4100 + w + 3 * h)
    c = lattice_colors()
    assert len(c) <= 19 * 19
    yy, xx = np.mgrid[0:h, 0:w]
    tiled = c[((yy % 19) * 19 + (xx % 19)) % len(c)]
    keep = ((xx // 19 + yy // 19) % 3) != 2
    img[..., :3] = np.where(keep[..., None], tiled, img[..., :3])
    return img


def target(kind, w, h):
    if kind == "zeros":
        return np.zeros((h, w, 4), np.uint8)
    if kind == "alpha_lattice":
        return alpha_lattice(w, h)
    if kind == "color_lattice":
        return color_lattice(w, h)
    if kind == "half_mask":   # an eraser preview that already holds a weaker mask on its left half
        img = np.zeros((h, w, 4), np.uint8)
        img[:, : w // 2, 3] = 60
        return img
    raise KeyError(kind)


def stamp_box(row, cx, cy):
    """the reference's pixel box of a round stamp (brush_render.rs:208-215) for finite centres, unclamped"""
    r = np.float32(row.brush["size"]) / np.float32(2)
    dr = r + np.float32(0.5) if row.brush["anti_aliased"] else r
    return (int(np.floor(np.float32(cx) - dr)), int(np.ceil(np.float32(cx) + dr)), int(np.floor(np.float32(cy) - dr)), int(np.ceil(np.float32(cy) + dr)))


def selection(kind, row):
    """"borders": 0 exactly on the chunk borders (x or y = 63, 64 mod 64 and the canvas edge) and on the box edges of every finite stamp, other pixels
    1 or 255 or (one in eight) 0"""
    assert kind == "borders"
    w, h = row.size
    rng = np.random.default_rng(4200 + w + h)
    sel = rng.choice(np.array([1, 255, 255, 255, 7, 200, 255, 0], np.uint8), size=(h, w))
    for edge in (63, 64, 127, 128, 191, 192):
        if edge < w:
            sel[:, edge] = 0
        if edge < h:
            sel[edge, :] = 0
    sel[0, :] = sel[h - 1, :] = 0
    sel[:, 0] = sel[:, w - 1] = 0
    if row.points is not None and row.dyn is None:
        for cx, cy in row.points:
            if not (np.isfinite(cx) and np.isfinite(cy)):
                continue
            x0, x1, y0, y1 = stamp_box(row, cx, cy)
            ys = slice(max(y0, 0), max(min(y1, h - 1) + 1, 0))
            xs = slice(max(x0, 0), max(min(x1, w - 1) + 1, 0))
            for x in (x0, x1):
                if 0 <= x < w:
                    sel[ys, x] = 0
            for y in (y0, y1):
                if 0 <= y < h:
                    sel[y, xs] = 0
    return sel


def tip_mask(kind, n):
    if kind == "zeros":
        return np.zeros((n, n), np.uint8)
    if kind == "full":
        return np.full((n, n), 255, np.uint8)
    if kind == "texel":
        m = np.zeros((n, n), np.uint8)
        m[n // 3, (2 * n) // 3] = 255
        return m
    assert kind == "random"
    m = np.random.default_rng(4300 + n).integers(0, 256, size=(n, n)).astype(np.uint8)
    m[n - 1, n - 1] = 1   # the corners count
    m[0, 0] = 255
    return m


def _pts(p):
    return np.array(p, np.float32).reshape(-1, 2)


def _brush(size, hardness, aa, kind, color=COLOR, flow=0.8, mode=1):
    return dict(size=size, hardness=hardness, anti_aliased=aa, color=color, flow=flow, is_eraser=kind == "eraser", mode=mode if kind == "tone" else 0)


def _target_for(kind):
    return "color_lattice" if kind == "tone" else "alpha_lattice"


# ---------------------------------------------------------------------------------------------------------------------------------- families
def size_points(size, w=W, h=H):
    """17 centres: integer, half-integer and quarter positions, the corner shared by four chunks, the canvas corners, half a pixel off the left edge, and
    points off the canvas by less and by more than the radius"""
    r = size / 2.0
    return _pts([(100.0, 68.0), (100.5, 40.5), (30.25, 90.75), (63.5, 63.5), (64.0, 64.0), (128.0, 128.0), (0.0, 0.0), (w - 1.0, h - 1.0), (-0.5, 50.0),
                 (127.75, 64.25), (192.0, 0.5), (64.0, 135.0), (10.5, 10.0),
                 (-0.5 * r, 20.0), (-(2.0 * r + 2.0), 100.0), (w - 1.0 + 0.5 * r, 110.0), (150.0, h + 2.0 * r + 3.0)])


def size_rows():
    rows = []
    for size in SIZES:
        for aa in (True, False):
            for hi, hardness in enumerate(HARDNESS):
                for kind in KINDS:
                    mode = 1 + (SIZES.index(size) + hi) % 3
                    rows.append(Row("size", f"{size}-aa{int(aa)}-h{hardness}-{kind}", (W, H), _target_for(kind), _brush(size, hardness, aa, kind, mode=mode),
                                    size_points(size), expect=dict(noop=size < 0.0633, min_painted=0 if size < 0.0633 else 3)))
    # the stated small canvases: one chunk exactly, one column more and one row fewer, and a single pixel
    for (w, h) in ((64, 64), (65, 63), (1, 1)):
        for size in (0.07, 3.0, 64.0, 5000.0):
            for kind in KINDS:
                pts = _pts([(0.0, 0.0), (w - 1.0, h - 1.0), (w / 2.0, h / 2.0), (63.5, 62.5), (-1.0, -1.0), (w + 0.25 * size, 3.0)])
                rows.append(Row("size", f"{w}x{h}-{size}-{kind}", (w, h), _target_for(kind), _brush(size, 0.37, True, kind, mode=2), pts, expect=dict(min_painted=1)))
    return rows


def gain_rows():
    rows = []
    pts = _pts([(50.0, 40.0), (60.5, 44.25), (120.0, 70.0)])
    for (a, flow, painted) in GAINS:
        for kind in KINDS:
            for aa in (True, False):
                rows.append(Row("gain", f"{a}x{flow}-{kind}-aa{int(aa)}", (160, 100), "color_lattice" if kind == "tone" else "zeros",
                                _brush(40.0, 0.2, aa, kind, color=(0.9, 0.3, 0.1, a), flow=flow, mode=1), pts, expect=dict(painted=painted)))
        for kind in ("eraser", "paint"):   # an image tip: the eraser has the cut-off, the paint path has none (a8 >= 0 writes the colour under any gain)
            rows.append(Row("gain", f"{a}x{flow}-tip-{kind}", (160, 100), "zeros", _brush(9.0, 1.0, True, kind, color=(0.9, 0.3, 0.1, a), flow=flow), pts,
                            dyn=dict(tip_mask=tip_mask("full", 9)), expect=dict(painted=painted or kind == "paint")))
    return rows


def stroke(n, w=W, h=H, seed=0):
    """n centres along a curve that crosses itself, the chunk borders and the canvas edge, with jumps"""
    t = np.linspace(0, 5 * np.pi, 193)[:n]
    pts = np.stack([w * (0.5 + 0.55 * np.cos(t * 0.7) * np.sin(t * 0.31 + 0.4)), h * (0.5 + 0.55 * np.sin(t * 0.9))], axis=1).astype(np.float32)
    rng = np.random.default_rng(4400 + seed)
    pts[::29] += rng.uniform(-30, 30, size=pts[::29].shape).astype(np.float32)
    return pts


COUNT_KINDS = {   # name: (brush kind, anti-aliased, size, dynamics)
    "paint_jitter": ("paint", True, 23.0, dict(stamp_counter=7, hue_jitter=0.8, brightness_jitter=0.4)),   # a colour per stamp: every tie shows the order
    "paint_noaa_small": ("paint", False, 3.0, dict(stamp_counter=9, hue_jitter=0.9)),
    "eraser": ("eraser", False, 23.0, None),
    "sponge": ("tone", True, 23.0, None),
    "tip": ("paint", True, 17.0, dict(stamp_counter=5, hue_jitter=0.7, tip_mask=tip_mask("random", 17), tip_random_rotation=True, tip_rotation_range=(-90.0, 250.0))),
}


def count_rows():
    rows = []
    for n in COUNTS:
        for name, (kind, aa, size, dyn) in COUNT_KINDS.items():
            rows.append(Row("count", f"{n}-{name}", (W, H), _target_for(kind), _brush(size, 0.6, aa, kind, mode=3), stroke(n), dyn=dyn,
                            binning=(1, 0) if n > 64 else (1,), expect=dict(painted=True)))
    return rows


ORDER_GAIN = (1.0, np.float32(128.0) / np.float32(255.0))   # colour alpha, flow: the eraser's strength at full coverage is the lattice's 128 / 255 exactly


def order_rows():
    """hardness 1 without anti-aliasing: every covered pixel has geometry 255, so every stamp of a stroke computes one a8 (paint) or one strength (eraser)"""
    pts = _pts([(40.0, 40.0), (52.0, 44.0), (46.5, 52.5), (64.0, 64.0), (70.25, 58.5), (58.0, 70.0), (40.0, 40.0)])
    rows = []
    for n_extra in (0, 70):   # the same ties through the binned kernel
        p = np.concatenate([pts, stroke(n_extra, 130, 100, seed=3)]) if n_extra else pts
        binning = (1, 0) if len(p) > 64 else (1,)
        rows.append(Row("order", f"paint-{len(p)}", (130, 100), "alpha_lattice", _brush(30.0, 1.0, False, "paint", color=(0.2, 0.7, 0.4, 0.8), flow=0.75), p,
                        dyn=dict(stamp_counter=11, hue_jitter=0.9, brightness_jitter=0.3), binning=binning, expect=dict(ties="paint")))
        rows.append(Row("order", f"eraser-{len(p)}", (130, 100), "alpha_lattice",
                        _brush(30.0, 1.0, False, "eraser", color=(0.0, 0.0, 0.0, ORDER_GAIN[0]), flow=float(ORDER_GAIN[1])), p, binning=binning,
                        expect=dict(ties="eraser")))
    return rows


TONE_GAIN = (0.6, 0.5)   # strength 0.15 a stamp inside the disc: several stamps on one pixel run l into 0 and 1 and s into 0


def tone_points():
    p = [(48.0, 32.0), (52.5, 30.25), (44.0, 36.0), (50.0, 34.0), (47.0, 31.0), (49.5, 33.5), (46.0, 30.0), (51.0, 35.0)]
    return _pts(p + [(16.0, 16.0), (80.0, 48.0), (64.0, 64.0), (0.0, 0.0)])


def tone_rows():
    rows = []
    for mode in (1, 2, 3):
        for aa in (True, False):
            for hardness in (1.0, 0.37):
                rows.append(Row("tone", f"mode{mode}-aa{int(aa)}-h{hardness}", (96, 64), "color_lattice",
                                _brush(40.0, hardness, aa, "tone", color=(0.0, 0.0, 0.0, TONE_GAIN[0]), flow=TONE_GAIN[1], mode=mode), tone_points(),
                                expect=dict(branches=hardness == 1.0)))
    return rows


def tip_points(w=W, h=H):
    return _pts([(100.0, 68.0), (100.5, 40.5), (30.25, 90.75), (63.5, 63.5), (64.0, 64.0), (0.0, 0.0), (w - 1.0, h - 1.0), (-0.5, 50.0), (-20.0, 20.0),
                 (w + 10.0, 110.0), (150.0, h + 400.0)])


def tip_rows():
    rows = []

    def add(name, n, mask, kind="paint", **dyn):
        d = dict(stamp_counter=3, hue_jitter=0.6, tip_mask=tip_mask(mask, n), **dyn)
        rows.append(Row("tip", name, (W, H), "half_mask" if kind == "eraser" else "alpha_lattice", _brush(float(n), 0.6, True, kind), tip_points(), dyn=d,
                        expect=dict(painted=mask != "zeros")))
    for n in TIP_SIZES + [300]:   # 300: larger than the canvas
        for rot in (0.0, -45.0):
            add(f"{n}-rot{rot}", n, "random", tip_rotation=rot)
        add(f"{n}-eraser", n, "random", kind="eraser", tip_rotation=33.0)
    for n in (64, 65, 3):
        for rot in TIP_ROTATIONS:
            add(f"{n}-rotation{rot}", n, "random", tip_rotation=rot)
            add(f"{n}-rotation{rot}-eraser", n, "random", kind="eraser", tip_rotation=rot)
    add("random-rotation-no-range", 63, "random", tip_random_rotation=True, tip_rotation_range=(30.0, 30.005))   # |range| < 0.01: the lower end itself
    add("random-rotation", 63, "random", tip_random_rotation=True, tip_rotation_range=(-90.0, 250.0))
    for mask in ("zeros", "full", "texel"):
        for kind in ("paint", "eraser"):
            for rot in (0.0, 17.0):
                add(f"{mask}-{kind}-rot{rot}", 33, mask, kind=kind, tip_rotation=rot)
    return rows


NONFINITE_KINDS = {   # name: (brush kind, anti-aliased, dynamics)
    "paint": ("paint", True, None), "paint_noaa": ("paint", False, None), "eraser": ("eraser", True, None), "dodge": ("tone", True, None),
    "tip": ("paint", True, dict(stamp_counter=2, tip_mask=tip_mask("random", 17))),
    "tip_rotated": ("paint", True, dict(stamp_counter=2, tip_mask=tip_mask("random", 17), tip_rotation=30.0)),
    "tip_eraser": ("eraser", True, dict(stamp_counter=2, tip_mask=tip_mask("random", 17), tip_rotation=30.0)),
}
NONFINITE_FINITE = {3: _pts([(50.0, 50.0), (90.0, 60.0)]), 70: stroke(69, 120, 90, seed=5)}


def nonfinite_points(n, bad, place):
    fin = NONFINITE_FINITE[n]
    at = {"first": 0, "middle": len(fin) // 2, "last": len(fin)}[place]
    return np.concatenate([fin[:at], _pts([bad]), fin[at:]])


def nonfinite_rows():
    rows = []
    for n in (3, 70):
        for bad in NONFINITE:
            for place in ("first", "middle", "last"):
                for name, (kind, aa, dyn) in NONFINITE_KINDS.items():
                    rows.append(Row("nonfinite", f"{n}-{bad[0]},{bad[1]}-{place}-{name}", (120, 90), "half_mask" if kind == "eraser" else _target_for(kind),
                                    _brush(17.5, 0.6, aa, kind), nonfinite_points(n, bad, place), dyn=dyn, binning=(1, 0) if n > 64 else (1,),
                                    expect=dict(nan=bool(np.isnan(bad[0]) or np.isnan(bad[1])), n=n, bad=bad, place=place)))
    return rows


def selection_rows():
    rows = []
    for size in (3.0, 9.5, 64.0, 400.0):   # from 3 up a stamp's box has an inside
        for kind in KINDS:
            for aa in (True, False):
                rows.append(Row("selection", f"{size}-{kind}-aa{int(aa)}", (W, H), _target_for(kind), _brush(size, 0.37, aa, kind, mode=3), size_points(size),
                                selection="borders", expect=dict(painted=True)))
    for n in (64, 65, 129):
        for name in ("paint_jitter", "eraser", "sponge", "tip"):
            kind, aa, size, dyn = COUNT_KINDS[name]
            rows.append(Row("selection", f"{n}-{name}", (W, H), _target_for(kind), _brush(size, 0.6, aa, kind, mode=3), stroke(n), selection="borders", dyn=dyn,
                            binning=(1, 0) if n > 64 else (1,), expect=dict(painted=True)))
    return rows


LINES = [   # on a 120 x 80 canvas: (p0, p1, some stamp lands on the canvas)
    ((10.0, 10.0), (100.5, 60.25), True), ((-30.0, 40.0), (60.0, 40.0), True), ((-20.0, -10.0), (140.0, 95.0), True), ((-20.0, 10.0), (-5.0, 70.0), False),
    ((50.0, 50.0), (50.05, 50.0), True), ((-3.0, 5.0), (-3.0, 5.0), False), ((119.0, 79.0), (0.0, 0.0), True), ((119.25, 0.0), (119.99, 79.0), True)]


def line_rows():
    rows = []
    for size in (0.0633, 1.0, 64.0, 400.0):
        for hardness in (0.0, 1.0):
            for aa in (True, False):
                for kind in KINDS:
                    for k, (p0, p1, on) in enumerate(LINES):
                        if size == 400.0 and k not in (0, 3, 4):   # the oracle's cost is stamps x area
                            continue
                        rows.append(Row("line", f"{size}-h{hardness}-aa{int(aa)}-{kind}-{k}", (120, 80), _target_for(kind),
                                        _brush(size, hardness, aa, kind, mode=2), line=(p0, p1), binning=(1, 0), expect=dict(painted=on)))
    return rows


def sweep_radii():
    """64 seeded radii log-uniform over [0.0316, 4096], then the powers of two 2^-4 .. 2^12 with their f32 neighbours (2^-5 = 0.03125 is below the skip)"""
    rng = np.random.default_rng(4500)
    r = list(np.exp(rng.uniform(np.log(0.0316), np.log(4096.0), 64)).astype(np.float32))
    for e in range(-4, 13):
        p = np.float32(2.0) ** np.float32(e)
        r += [np.nextafter(p, np.float32(0)), p, np.nextafter(p, np.float32(1e9))]
    return [np.float32(x) for x in r]


def radius_rows():
    """one anti-aliased stamp on 96 x 96; a radius beyond the canvas has its centre moved away along (0.6, 0.8) so that the edge band crosses the middle"""
    rows = []
    for r in sweep_radii():
        size = float(np.float32(2) * r)
        assert np.float32(size) / np.float32(2) == r
        c = (48.25, 47.9) if r < 40 else (48.25 - float(r) * 0.6, 47.9 - float(r) * 0.8)
        rows.append(Row("radius", repr(float(r)), (96, 96), "zeros", _brush(size, 0.37, True, "paint", color=(0.5, 0.25, 0.75, 1.0), flow=1.0), _pts([c]),
                        expect=dict(radius=float(r), min_painted=1)))
    return rows


def run(backend, row, tgt=None):
    """the row on an OracleBackend or a GpuBackend (tests/backends.py): the stroke's result"""
    w, h = row.size
    t = target(row.target, w, h) if tgt is None else tgt
    sel = selection(row.selection, row) if row.selection else None
    if row.line is not None:
        return backend.brush_line(t, row.brush, row.line[0], row.line[1], sel)
    return backend.brush_stamps(t, row.brush, row.points, sel, row.dyn)


_BUILDERS = dict(size=size_rows, gain=gain_rows, count=count_rows, order=order_rows, tone=tone_rows, tip=tip_rows, nonfinite=nonfinite_rows,
                 selection=selection_rows, line=line_rows, radius=radius_rows)
_cache = {}


def rows(family):
    if family not in _cache:
        _cache[family] = _BUILDERS[family]()
    return _cache[family]
