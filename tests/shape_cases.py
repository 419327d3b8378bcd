"""Parameter sets of the shape tests: the reference's 20 golden shapes (tests/visual_shapes.rs:44-171) and the seeded cases of the device parity sweep."""
import math

import numpy as np

from tests import shape_model as M

GOLDEN_W = GOLDEN_H = 128


def to_api(s):
    """the model's shape dict as the package's Shape"""
    from paintfe_amd import Shape
    return Shape(kind=s["kind"], fill=s["fill"], cx=float(s["cx"]), cy=float(s["cy"]), hw=float(s["hw"]), hh=float(s["hh"]), rotation=float(s["rotation"]),
                 outline_width=float(s["outline_width"]), corner_radius=float(s["corner_radius"]), primary=s["primary"], secondary=s["secondary"],
                 anti_alias=s["anti_alias"])


def load_goldens():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes.npz"))


def _golden():
    g = {}
    for k in ("ellipse", "rectangle", "triangle", "pentagon", "hexagon", "octagon", "cross", "heart", "star5"):   # :86-94
        g[f"{k}_outline"] = M.shape(k, "outline")
    for k in ("ellipse", "rectangle", "triangle", "pentagon", "hexagon", "heart"):                                # :111-116
        g[f"{k}_filled"] = M.shape(k, "both")
    g["rounded_rect_outline"] = M.shape("rounded_rect", "outline", corner_radius=12.0)                            # :122-136
    g["rounded_rect_filled"] = M.shape("rounded_rect", "both", corner_radius=12.0)
    g["rectangle_rotated_45"] = M.shape("rectangle", "both", rotation=np.float32(0.78539816339744830962))         # FRAC_PI_4, :143
    g["ellipse_fill_only"] = M.shape("ellipse", "filled")                                                         # :155
    g["rectangle_no_aa"] = M.shape("rectangle", "both", anti_alias=False)                                         # :166
    return g


GOLDEN = _golden()
GOLDEN_LIBM = sorted(n for n, s in GOLDEN.items() if s["kind"] in M.LIBM_KINDS)
GOLDEN_EXACT = sorted(n for n, s in GOLDEN.items() if s["kind"] not in M.LIBM_KINDS)
assert len(GOLDEN) == 20 and len(GOLDEN_LIBM) == 6 and len(GOLDEN_EXACT) == 14

# ---- the device parity sweep: canvas 131 x 77 (ragged 64 x 4 tiles, a width that is no multiple of 4 or 64) ----
SWEEP_W, SWEEP_H = 131, 77


def sweep_geometries(kind):
    """six geometries per kind, each named after what it is there for; together they hold, for every kind: hw != hh, a non-zero rotation, a box that starts at an
    odd x and is clipped by a canvas edge, outline_width 0 and one above min(hw, hh), a corner_radius above min(hw, hh), hw = 0.3 and semi-transparent colours"""
    rng = np.random.default_rng(1000 + M.KINDS.index(kind))
    jit = lambda: float(np.float32(rng.uniform(-0.45, 0.45)))
    semi_p, semi_s = (250, 70, 30, 140), (20, 160, 240, 90)
    return {
        "stretched_rotated": dict(cx=60.0 + jit(), cy=36.0 + jit(), hw=34.0 + jit(), hh=17.0 + jit(), rotation=0.3 + jit(), outline_width=2.5, corner_radius=6.0,
                                  primary=semi_p, secondary=semi_s),
        "odd_x0_clipped_right": dict(cx=111.25, cy=40.5 + jit(), hw=30.0, hh=22.0 + jit(), rotation=0.0, outline_width=4.0, corner_radius=40.0),   # x0 = floor(111.25 - 30 - 2) = 79
        "clipped_top_left_rotated": dict(cx=9.0 + jit(), cy=5.0 + jit(), hw=21.0, hh=26.0, rotation=-2.1, outline_width=0.0, corner_radius=3.0, primary=semi_p),
        "fat_outline": dict(cx=65.0 + jit(), cy=38.0 + jit(), hw=19.0, hh=12.0, rotation=float(np.float32(math.pi / 4)), outline_width=15.0, corner_radius=30.0,
                            secondary=semi_s),
        "sliver": dict(cx=40.0 + jit(), cy=39.0 + jit(), hw=0.3, hh=9.0, rotation=0.0, outline_width=1.0, corner_radius=0.0),
        "tiny": dict(cx=70.5, cy=30.5, hw=1.25, hh=0.75, rotation=1.0 + jit(), outline_width=0.5, corner_radius=0.25, primary=semi_p, secondary=semi_s),
    }


def sweep_cases():
    """(id, shape) for 17 kinds x 6 geometries x 3 fill modes x anti-alias on / off"""
    out = []
    for kind in M.KINDS:
        for gname, g in sweep_geometries(kind).items():
            for fill in M.FILLS:
                for aa in (True, False):
                    out.append((f"{kind}-{gname}-{fill}-{'aa' if aa else 'noaa'}", M.shape(kind, fill, anti_alias=aa, **g)))
    return out


def width_cases():
    """rectangle and heart whose clipped boxes are 1, 63, 64, 65 and 130 pixels wide on the 131-wide canvas: (id, shape, expected box width)"""
    out = []
    for kind in ("rectangle", "heart"):
        # a box hanging off the left edge: x0 = 0, x1 = ceil(cx + hw + 2) = bw
        for bw in (1, 63, 64, 65, 130):
            out.append((f"{kind}-bw{bw}", M.shape(kind, "both", cx=bw - 2.0 - 70.0 - 0.5, cy=38.0, hw=70.0, hh=20.0, outline_width=3.0), bw))
    return out
