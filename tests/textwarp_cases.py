"""The cases of the text warps, shared by tests/test_textwarp_model_host.py (which shows that each draws what it is named after) and
tests/test_gpu_textwarp.py (which holds the device to the model on them).  Expected images are computed once per (case, flavour) and handed out read-only."""
import functools

import numpy as np

from . import textwarp_model as M
from .shape_model import PI, F, Libm

MEASURED, POW2, DOT = (131, 37), (64, 32), (1, 1)   # sources: ragged against every tile; the hand-derived envelope's; the smallest
EIGHT_PI = float(F(8) * PI)
BEYOND_EIGHT_PI = float(np.nextafter(F(8) * PI, F(np.inf)))


@functools.lru_cache(maxsize=None)
def source(size, seed=7):
    """a block raster of size = (w, h): random colours, an alpha that is 0 on a lattice of holes, 255 on stripes and random between"""
    w, h = size
    rng = np.random.default_rng(seed + 1000 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 3] = np.where((xx // 3 + yy // 2) % 5 == 0, 0, np.where((xx + yy) % 7 < 2, 255, img[..., 3]))
    if size == DOT:
        img[0, 0] = (200, 100, 50, 255)
    img.setflags(write=False)
    return img


CROSSING_TOP = [(0.0, -30.0), (100.0, -30.0), (200.0, 30.0), (300.0, 30.0)]
CROSSING_BOTTOM = [(0.0, 30.0), (100.0, 30.0), (200.0, -30.0), (300.0, -30.0)]
# name: (source size, warp, the least number of output pixels the case must sample; 0 with an identity plan: the source itself comes back)
WARPS = {
    # arc: the default bend and its mirror, the half circle, both sides of the identity gate, the flat-radius branch (|angle| <= 0.01), distortions
    "arc_0.5": (MEASURED, dict(kind="arc", bend=0.5), 3000),
    "arc_-0.5": (MEASURED, dict(kind="arc", bend=-0.5), 0),          # see PAINT_NOTHING
    "arc_1.0": (MEASURED, dict(kind="arc", bend=1.0), 3000),
    "arc_0.0009_identity": (MEASURED, dict(kind="arc", bend=0.0009), 0),
    "arc_0.0011": (MEASURED, dict(kind="arc", bend=0.0011), 1500),   # the flat radius' forward map shrinks the bounds to the middle 46 columns
    "arc_0.002_flat_radius": (MEASURED, dict(kind="arc", bend=0.002), 3000),
    "arc_distorted": (MEASURED, dict(kind="arc", bend=0.5, horizontal_distortion=0.3, vertical_distortion=-0.2), 3000),
    "arc_-0.8_distorted": (MEASURED, dict(kind="arc", bend=-0.8, horizontal_distortion=-0.25, vertical_distortion=0.4), 0),
    "arc_hdist_-1": (MEASURED, dict(kind="arc", bend=0.5, horizontal_distortion=-1.0), 0),      # divides by zero: the comparisons reject what it gives
    "arc_bounds_over_8192_identity": (MEASURED, dict(kind="arc", bend=0.5, horizontal_distortion=100.0), 0),
    "arc_pow2": (POW2, dict(kind="arc", bend=0.5), 1000),
    "arc_dot": (DOT, dict(kind="arc", bend=0.5), 0),
    # circular: both directions, a radius below the floor of 10, start angles that run the first loop, the second loop, and each of them several times
    "circle_cw": (MEASURED, dict(kind="circular", radius=40.0), 3000),
    "circle_ccw": (MEASURED, dict(kind="circular", radius=25.0, clockwise=False), 3000),
    "circle_radius_5": (MEASURED, dict(kind="circular", radius=5.0), 1000),
    "circle_start_2": (MEASURED, dict(kind="circular", radius=40.0, start_angle=2.0), 3000),
    "circle_start_-4": (MEASURED, dict(kind="circular", radius=40.0, start_angle=-4.0), 3000),
    "circle_start_8pi": (MEASURED, dict(kind="circular", radius=40.0, start_angle=EIGHT_PI), 3000),
    "circle_start_-8pi": (MEASURED, dict(kind="circular", radius=40.0, start_angle=-EIGHT_PI, clockwise=False), 3000),
    "circle_pow2": (POW2, dict(kind="circular", radius=30.0), 1500),
    "circle_dot": (DOT, dict(kind="circular", radius=12.0), 1),
    # path: the default points, a curve that crosses itself, four coincident points (paints nothing), three points (identity), and a straight path long
    # enough that out_w clamps at 4096, under a source 8 px tall so that the frame stays small
    "path_default": (MEASURED, dict(kind="path"), 3000),
    "path_crossing": (MEASURED, dict(kind="path", control_points=[(0.0, 0.0), (150.0, 100.0), (-50.0, 100.0), (100.0, 0.0)]), 3000),
    "path_coincident": (MEASURED, dict(kind="path", control_points=[(50.0, 50.0)] * 4), 0),
    "path_3_points_identity": (MEASURED, dict(kind="path", control_points=[(0.0, 0.0), (100.0, -50.0), (200.0, -50.0)]), 0),
    "path_clamped_4096": ((131, 8), dict(kind="path", control_points=[(0.0, 0.0), (1500.0, 0.0), (3000.0, 0.0), (4500.0, 0.0)]), 800),
    "path_pow2": (POW2, dict(kind="path"), 1500),
    "path_dot": (DOT, dict(kind="path"), 0),
    # envelope: the defaults, the hand-derived rectangle, curves that cross (|span| < 0.001 at the crossing, a negative span behind it)
    "envelope_default": (MEASURED, dict(kind="envelope"), 3000),
    "envelope_rectangle": (POW2, dict(kind="envelope", top_curve=[(0.0, 0.0), (0.0, 0.0), (64.0, 0.0), (64.0, 0.0)],
                                      bottom_curve=[(0.0, 32.0), (0.0, 32.0), (64.0, 32.0), (64.0, 32.0)]), 2048),
    "envelope_crossing": (MEASURED, dict(kind="envelope", top_curve=CROSSING_TOP, bottom_curve=CROSSING_BOTTOM), 3000),
    # curves so far apart that out_h clamps at 4096 (and beyond +-2^18, where the kernel divides with `/`): every sampled pixel reads the source's first row
    "envelope_steep": (MEASURED, dict(kind="envelope", top_curve=[(0.0, -300000.0), (100.0, -300000.0), (200.0, -300000.0), (300.0, -300000.0)],
                                      bottom_curve=[(0.0, 300000.0), (100.0, 300000.0), (200.0, 300000.0), (300.0, 300000.0)]), 100000),
    # a numerator below the range the kernel's shared-reciprocal division is proved for (py - top_y = 1e-30 on the row py = 0): the plain divide's branch
    "envelope_tiny_numerator": (POW2, dict(kind="envelope", top_curve=[(0.0, -1e-30), (0.0, -1e-30), (64.0, -1e-30), (64.0, -1e-30)],
                                           bottom_curve=[(0.0, 32.0), (0.0, 32.0), (64.0, 32.0), (64.0, 32.0)]), 2048),
    "envelope_3_points_identity": (MEASURED, dict(kind="envelope", top_curve=CROSSING_TOP[:3]), 0),
    "envelope_dot": (DOT, dict(kind="envelope"), 1),
    "none": (MEASURED, dict(kind="none"), 0),
}
LIBM_WARPS = [n for n, (_, warp, _) in WARPS.items() if warp["kind"] in ("arc", "circular")]
EXACT_WARPS = [n for n in WARPS if n not in LIBM_WARPS]
IDENTITIES = [n for n in WARPS if n.endswith("identity") or n == "none"]
# what the reference leaves empty: a division by zero; a negative bend, whose arc_inverse_map is not the inverse of arc_map_point (rel_y = r_abs - dy * r_sign
# lands near 3 r_abs where the forward map put dy near 2 r_abs, so sy_norm is far below 0: restated, not repaired); a path of zero length (no tangent);
# a source one pixel tall under an arc or a path, whose band of valid sy misses every pixel centre
PAINT_NOTHING = ["arc_hdist_-1", "arc_-0.5", "arc_-0.8_distorted", "path_coincident", "arc_dot", "path_dot"]

# name: (source size, angle, pivot in buffer coordinates or None)
ROTATIONS = {
    "rotate_0.3": (MEASURED, 0.3, None),
    "rotate_-0.3": (MEASURED, -0.3, None),
    "rotate_pivot": (MEASURED, 0.3, (10.5, 40.25)),
    "rotate_-0.3_pivot": (POW2, -0.3, (-7.0, 3.5)),
    "rotate_dot": (DOT, 0.3, None),
    "rotate_0.001_skipped": (MEASURED, 0.001, None),
    "rotate_quarter_turn": (POW2, float(F(np.pi / 2)), None),
}

CANVAS = (300, 200)
# name: [(source size, warp, offset on the canvas, rotation, pivot in canvas coordinates or None), ...] placed in order; prior: the canvas starts with content
PLACEMENTS = {
    "off_the_left": (False, [(MEASURED, dict(kind="none"), (-60, 40), 0.0, None)]),
    "off_the_top": (False, [(MEASURED, dict(kind="arc", bend=0.5), (50, -30), 0.0, None)]),
    "off_the_right": (False, [(MEASURED, dict(kind="none"), (230, 90), 0.3, None)]),
    "off_the_bottom": (False, [(MEASURED, dict(kind="envelope"), (20, 150), 0.0, None)]),
    "outside": (True, [(MEASURED, dict(kind="none"), (400, 40), 0.0, None)]),
    "prior_content": (True, [(MEASURED, dict(kind="none"), (80, 70), -0.3, (100.0, 100.0))]),
    "two_blocks": (True, [(MEASURED, dict(kind="none"), (60, 60), 0.0, None), (POW2, dict(kind="circular", radius=30.0), (120, 70), 0.3, None)]),
    "warped_and_rotated": (False, [(MEASURED, dict(kind="path"), (90, 140), 0.3, (150.0, 100.0))]),
}


@functools.lru_cache(maxsize=None)
def prior_canvas():
    rng = np.random.default_rng(99)
    c = rng.integers(0, 256, (CANVAS[1], CANVAS[0], 4), dtype=np.uint8)
    c.setflags(write=False)
    return c


def start_canvas(name):
    return prior_canvas() if PLACEMENTS[name][0] else np.zeros((CANVAS[1], CANVAS[0], 4), np.uint8)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_warp(name, flavour="glibc", perturb=None):
    """(image, plan, sampled pixels, ambiguous libm calls) of a warp case, read-only"""
    size, warp, _ = WARPS[name]
    libm = Libm(flavour)
    out, plan, painted = M.apply_warp(source(size), warp, libm, perturb)
    return frozen(out), plan, painted, libm.ambiguous


@functools.lru_cache(maxsize=None)
def expected_rotation(name):
    size, angle, pivot = ROTATIONS[name]
    out, plan = M.rotate(source(size), angle, pivot)
    return frozen(out), plan


@functools.lru_cache(maxsize=None)
def expected_placement(name, flavour="glibc"):
    """(canvas, ambiguous libm calls)"""
    libm = Libm(flavour)
    canvas = start_canvas(name)
    for size, warp, offset, rotation, pivot in PLACEMENTS[name][1]:
        canvas = M.place(canvas, source(size), warp, offset, rotation, pivot, libm)
    return frozen(canvas), libm.ambiguous
