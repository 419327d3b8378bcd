"""Paths and shapes the custom-shape tests share (tests/test_customshape_model_host.py, tests/test_gpu_customshape.py).  Every path is written by hand or
generated from a seed here; a shape is a tests/shape_model.py dict (its `kind` only shapes the bounding box)."""
import math

import numpy as np

from . import customshape_model as CM
from . import shape_model as M

F = np.float32
CANVAS_W, CANVAS_H = 240, 200


def square(x0, y0, x1, y1):
    return np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)], F)


def square_path(size=8.0):
    return CM.path([square(0, 0, size, size)])


def holed_path():
    """a 16 x 16 square with a 6 x 6 square hole at (5, 5): even-odd"""
    return CM.path([square(0, 0, 16, 16), square(5, 5, 11, 11)])


def reversed_path(p):
    """the same segments, listed in reverse order (and each one reversed)"""
    return dict(polylines=[q[::-1].copy() for q in p["polylines"][::-1]], bounds=p["bounds"])


def ring(n, seed, cx=50.0, cy=50.0, r=40.0, jitter=0.35):
    """a closed polygon of exactly n segments (n >= 3) around (cx, cy), radii jittered from a seed"""
    rng = np.random.default_rng(seed)
    ang = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * (2 * math.pi / n)
    rad = r * (1 + rng.uniform(-jitter, jitter, n))
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).astype(F)
    return np.concatenate([pts, pts[:1]])


def counted_path(n, seed=1):
    """a path of exactly n segments in bounds (0, 0, 100, 100)"""
    if n == 0:
        polys = [np.zeros((0, 2), F), np.array([(3, 4)], F)]          # a polyline of 0 and one of 1 point: no segment
    elif n < 3:
        polys = [np.array([(20, 15), (80, 35), (30, 90)][:n + 1], F)]  # open
    else:
        polys = [ring(n, seed)]
    return CM.path(polys, (0, 0, 100, 100))


def blob_path(n_outer=96, n_hole=40, seed=3):
    """a wobbly ring with a hole: the realistic case"""
    return CM.path([ring(n_outer, seed, 60, 50, 44, 0.2), ring(n_hole, seed + 1, 62, 48, 14, 0.25)], (0, 0, 120, 100))


def far_and_near_path(n_far=1000, seed=9):
    """many short segments far from where the shape is looked at and a few near it: the worst case for a wrong drop.  Bounds (0, 0, 4000, 4000); the near
    square sits at (1990 .. 2010)"""
    rng = np.random.default_rng(seed)
    polys = [square(1990, 1990, 2010, 2010)]
    left = n_far
    while left > 0:
        k = min(left, 25)
        cx, cy = rng.uniform(0, 4000, 2)
        if abs(cx - 2000) < 300 and abs(cy - 2000) < 300:
            continue
        polys.append(ring(k, int(rng.integers(1 << 30)), cx, cy, 30.0) if k >= 3 else np.array([(cx, cy), (cx + 5, cy + 7), (cx - 3, cy + 2)][:k + 1], F))
        left -= k
    return CM.path(polys, (0, 0, 4000, 4000))


def predicate_edge_path():
    """integer coordinates in bounds (0, 0, 16, 16): horizontal segments, zero-length and near-zero-length segments (len2 on both sides of 1e-6), a 45-degree
    edge through integer points, and a segment whose |dy| straddles 1e-6"""
    return CM.path([
        np.array([(2, 2), (14, 2), (14, 14), (8, 8), (2, 14), (2, 2)], F),       # horizontals, verticals, two diagonals through lattice points
        np.array([(4, 10), (4, 10)], F),                                         # zero length
        np.array([(10, 4), (10.0009, 4)], F),                                    # len2 = 8.1e-7 <= 1e-6: distance to the start point
        np.array([(11, 5), (11.0011, 5)], F),                                    # len2 = 1.21e-6 > 1e-6: projected
        np.array([(5, 12), (9, 12.0000005)], F),                                 # |dy| <= 1e-6: no crossing
        np.array([(5, 13), (9, 13.000002)], F),                                  # |dy| > 1e-6: a crossing for py in between
    ], (0, 0, 16, 16))


def shape(fill="filled", **kw):
    kw.setdefault("primary", (30, 200, 90, 255))
    return M.shape(kw.pop("kind", "rectangle"), fill, **kw)


def on_grid_shape(fill, cx, cy, half=8.0, **kw):
    """half extents that make sx = sy = 1 for a 16 x 16 path: with cx, cy on a quarter the samples land on the path's lattice"""
    return shape(fill, cx=cx, cy=cy, hw=half, hh=half, **kw)
