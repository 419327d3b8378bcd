"""Case tables of the warp kernels at their edges (k_warp.hip): the fused mesh warp and the mesh field, the displacement warp, the Liquify dab lists.
tests/test_warp_cases_host.py shows on the CPU, with the oracle alone, that each table reaches what it is here for; tests/test_gpu_warp_edges.py runs them.
Every size comes from the kernels' compile-time shape (pfx_int_warp_info), so a retuned build moves the cases instead of passing them by."""
import collections
import functools

import numpy as np

from . import inputs as I

f32 = np.float32
IN_LDS, PAIR, BUF32, XCD = 1, 2, 4, 8      # pfx_int_warp_last(ctx, 0)
DAB_NONE, DAB_PLAIN, DAB_CHUNKED = 0, 1, 2  # pfx_int_warp_last(ctx, 3)
MAX_CELLS = 4096                            # the host's cap on a grid's columns and rows (pfx_api.cpp:upload_points)

Consts = collections.namedtuple("Consts", "walk wx lds_pts warp_yr xcd_rows dab_cull")


@functools.lru_cache(maxsize=None)
def consts():
    from paintfe_amd import _lib
    f = _lib.load().pfx_int_warp_info
    c = Consts(*[int(f(k)) for k in range(6)])
    assert min(c) > 0 and f(6) == -1
    return c


def tile_rows():
    """pixel rows of one tile row of the fused mesh warp (a workgroup's 4 / WX waves below each other, MESH_WALK rows each)"""
    c = consts()
    return c.walk * (4 // c.wx)


def tile_cols():
    return 64 * consts().wx


def tile_grid(w, h):
    """pfxk_warp_mesh's grid: tile columns, tile rows"""
    return -(-w // tile_cols()), -(-h // tile_rows())


def xcd_parts(gy):
    """mesh_roll_kernel's split of gy tile rows over the eight XCDs: [r0, r1) of every part"""
    return [(gy * k // 8, gy * (k + 1) // 8) for k in range(8)]


def takes_xcd_order(h):
    return tile_grid(1, h)[1] >= consts().xcd_rows


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------------------------------
def sizes():
    """(w, h); with MESH_WALK 48, MESH_WX 4 and the XCD order from 16 tile rows: (70, 721) (130, 769) (257, 1105) (300, 1009) (1, 800) (2, 730) (65, 47)"""
    t, x, cw = tile_rows(), consts().xcd_rows, tile_cols()
    return [(70, (x - 1) * t + 1),          # exactly the threshold's tile rows, the last one 1 row high
            (130, x * t + 1),               # one more: a ragged split over 8 parts, with blocks that return at once
            (cw + 1, (x + 7) * t + 1),      # 2 tile columns, the second 1 pixel wide
            (300, (x + 5) * t + 1),
            (1, x * t + 32),                # the non-PAIR path
            (2, (x - 1) * t + 10),          # the PAIR path at its least width
            (65, t - 1)]                    # below every threshold


def small_size():
    return sizes()[-1]


@functools.lru_cache(maxsize=None)
def source(w, h):
    """random RGBA, alpha >= 1: an all-zero result pixel was sampled outside"""
    img = I.random_rgba(w, h, 0xED6E + 131 * w + h)
    img[..., 3] = np.maximum(img[..., 3], 1)
    img.setflags(write=False)
    return img


def transparent_share(out):
    return float((out == 0).all(-1).mean())


# ---- grids and deformations --------------------------------------------------------------------------------------------------------------------------------------------
def grids():
    p = consts().lds_pts
    assert p == 2048, "pick new grids around MESH_LDS_PTS: (cols + 1) * (rows + 1) == MESH_LDS_PTS and == MESH_LDS_PTS + 1"
    return [(1, 1), (6, 6), (9, 4),
            (31, 63),       # 32 x 64 = 2048 points: the last grid staged in LDS (32 KiB)
            (2, 682),       # 3 x 683 = 2049 points: the first that is not
            (3, 200)]       # cell rows narrower than a walk at every size


CAP_GRIDS = [(MAX_CELLS, 1), (1, MAX_CELLS)]
FORMS = ("nonuniform", "uniform", "omitted")          # the original grid: given and jittered by +-1.5 px, given and uniform, not given (the _fast field)
NONFINITE = ("nan", "+inf", "-inf", "3e9", "1e30")
DEFORMS = ("jitter", "fold", "coincident", "shift_int", "shift_half") + NONFINITE
MeshRow = collections.namedtuple("MeshRow", "size grid form deform")


def n_points(grid):
    return (grid[0] + 1) * (grid[1] + 1)


def lattice(grid, w, h):
    cols, rows = grid
    x = np.arange(cols + 1, dtype=f32) / f32(cols) * f32(w)
    y = np.arange(rows + 1, dtype=f32) / f32(rows) * f32(h)
    return np.stack(np.broadcast_arrays(x[None, :], y[:, None]), -1).astype(f32)      # (rows + 1, cols + 1, 2), inputs.uniform_grid's values


SALT = 42      # the first draw at which every jitter and fold row meets the non-vacuity condition of test_warp_cases_host.py (a 1 x 1 grid has four points)


def _seed(row):
    return [row.size[0], row.size[1], row.grid[0], row.grid[1], DEFORMS.index(row.deform), SALT]


def mesh_points(row):
    """(original points or None, deformed points), each (rows + 1) * (cols + 1) x 2 f32"""
    (w, h), (cols, rows) = row.size, row.grid
    rng = np.random.default_rng(_seed(row))
    base = lattice(row.grid, w, h)
    orig = base + (rng.random(base.shape).astype(f32) - f32(0.5)) * f32(3.0) if row.form == "nonuniform" else base
    jitter = f32(0.6) * (rng.random(base.shape).astype(f32) - f32(0.5)) * np.array([w, h], f32)   # +-0.3 of the size on every point, borders included
    if row.deform == "shift_int":
        deformed = orig + np.array([3.0, -2.0], f32)
    elif row.deform == "shift_half":
        deformed = orig + np.array([-0.5, 1.5], f32)
    elif row.deform in NONFINITE:
        deformed = base + f32(0.1) * jitter                 # mild: what turns transparent is what the one point below reaches
    else:
        deformed = base + jitter
    if row.deform == "fold":                            # two interior rows of points change places
        assert rows >= 3
        a = rows // 2
        deformed[[a, a + 1]] = deformed[[a + 1, a]]
    if row.deform == "coincident":                      # a 2 x 2 block of points on one spot
        r0, c0 = rows // 2, cols // 2
        deformed[r0:r0 + 2, c0:c0 + 2] = deformed[r0, c0]
    if row.deform in NONFINITE:
        v = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "3e9": 3e9, "1e30": 1e30}[row.deform]
        deformed[rows // 2, (cols + 1) // 2, NONFINITE.index(row.deform) % 2] = v
    o = None if row.form == "omitted" else np.ascontiguousarray(orig.reshape(-1, 2), f32)
    return o, np.ascontiguousarray(deformed.reshape(-1, 2), f32)


@functools.lru_cache(maxsize=None)
def mesh_rows():
    """Not the full product (1700 rows): jitter on every size x grid with the form rotating, so that every grid meets every form and every size meets every
    form; the other deformations on the 6 x 6 grid at every size and on both sides of the LDS boundary at the ragged XCD size; the capped grids at the small size"""
    out = []
    for si, size in enumerate(sizes()):
        for gi, grid in enumerate(grids()):
            out.append(MeshRow(size, grid, FORMS[(si + gi) % 3], "jitter"))
        for di, deform in enumerate(DEFORMS[1:]):
            out.append(MeshRow(size, (6, 6), FORMS[(si + di) % 3], deform))
    ragged = sizes()[1]
    for grid in ((31, 63), (2, 682), (3, 200)):
        for di, deform in enumerate(("fold", "coincident", "nan", "shift_half")):
            out.append(MeshRow(ragged, grid, FORMS[di % 3], deform))
    for grid in CAP_GRIDS:
        for form in FORMS:
            out.append(MeshRow(small_size(), grid, form, "jitter"))
    return tuple(out)


def mesh_flags(row, xcd, buf32):
    """pfx_int_warp_last(ctx, 0) after the fused warp of this row under pfx_tune mesh_xcd = xcd, warp_buf32 = buf32"""
    w, h = row.size
    return ((IN_LDS if n_points(row.grid) <= consts().lds_pts else 0) | (PAIR if w >= 2 else 0) | (BUF32 if buf32 and w >= 2 else 0) |
            (XCD if xcd and takes_xcd_order(h) else 0))


def cell_row_of(h_full, rows, y):
    """catmull_rom_surface's cell row of pixel rows y (transform.rs:1688, :1597-1603), in f32 like the reference"""
    v = (np.asarray(y).astype(f32) + f32(0.5)) / f32(h_full) * f32(rows)
    return np.minimum(np.clip(v, f32(0.0), f32(rows) - f32(0.0001)).astype(np.int64), rows - 1)


def walk_kinds(h, rows, first_row=0, h_full=None):
    """(walks whose rows lie in one row of mesh cells, walks that straddle two or more) of an h-row launch: mesh_roll_kernel's two walk forms"""
    walk = consts().walk
    one = two = 0
    for y0 in range(0, h, walk):
        ri = cell_row_of(h_full or h, rows, np.array([y0, min(y0 + walk, h) - 1]) + first_row)
        one, two = one + (ri[0] == ri[1]), two + (ri[0] != ri[1])
    return int(one), int(two)


# ---- band form -----------------------------------------------------------------------------------------------------------------------------------------------------------
def band_cases():
    """(w, h_full, [(first_row, band_rows)]): with today's shape 130, 1500, (0, 721) (37, 800) (699, 801) (1499, 1)"""
    t, x = tile_rows(), consts().xcd_rows
    h_full = (2 * x - 1) * t + 12
    return 130, h_full, [(0, (x - 1) * t + 1), (37, x * t + 32), (h_full - (x * t + 33), x * t + 33), (h_full - 1, 1)]


BAND_MESHES = [MeshRow(None, (6, 6), "nonuniform", "jitter"), MeshRow(None, (3, 200), "omitted", "jitter"), MeshRow(None, (2, 682), "uniform", "fold")]


# ---- displacement fields -----------------------------------------------------------------------------------------------------------------------------------------------
FIELD_KINDS = ("random", "border_px", "border_wave_x", "border_wave_y", "src_larger", "src_smaller", "nonfinite")
BORDER_OFFSETS = (-2, -1, 0)       # floor(sx) on each of these, and on size + each of these


def border_targets(n):
    """sample coordinates whose floor is -2, -1, 0, n - 2, n - 1, n, and fractional neighbours"""
    return np.array([-2.0, -1.5, -1.0, -0.75, -0.5, 0.0, 0.25, n - 2.0, n - 1.5, n - 1.0, n - 0.5, n - 0.001, n, n + 0.5, -2.5, n + 7.0], f32)


def field_case(kind, size):
    """(source image, field): the field has the size's shape, the source too unless the kind says otherwise"""
    w, h = size
    rng = np.random.default_rng([w, h, FIELD_KINDS.index(kind)])
    sw, sh = {"src_larger": (w + 3, h + 2), "src_smaller": (max(w - 3, 1), max(h - 2, 1))}.get(kind, (w, h))
    img = source(sw, sh)
    gx, gy = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    if kind in ("random", "src_larger", "src_smaller"):
        disp = (rng.random((h, w, 2)).astype(f32) - f32(0.5)) * f32(1.2) * np.array([w, h], f32)          # +-0.6 of the size
    elif kind == "border_px":                                                                                  # every pixel its own target: waves that mix
        xs, ys = border_targets(sw), border_targets(sh)
        tx, ty = xs[rng.integers(0, len(xs), (h, w))], ys[rng.integers(0, len(ys), (h, w))]
        disp = np.stack([gx - tx, gy - ty], -1)
    elif kind in ("border_wave_x", "border_wave_y"):                                                           # one target per wave (64 columns of a row)
        ts = border_targets(sw if kind[-1] == "x" else sh)
        pick = ts[(np.arange(h)[:, None] + 5 * (np.arange(w)[None, :] // 64)) % len(ts)]
        inside = f32(0.25) + (gx if kind[-1] == "y" else gy) * f32(0.5)                                        # the other axis stays inside (and off the grid)
        tx, ty = (pick, inside) if kind[-1] == "x" else (inside, pick)
        disp = np.stack([gx - tx, gy - ty], -1)
    else:                                                                                                      # NaN / inf inside waves that are otherwise interior
        disp = np.full((h, w, 2), 0.25, f32)
        disp[:, 0, 0] = -0.5
        disp[0, :, 1] = -0.5
        specials = [(np.nan, 0.25), (0.25, np.nan), (np.nan, np.nan), (np.inf, 0.25), (0.25, -np.inf), (-np.inf, np.inf), (3.0e9, 0.25), (-3.0e9, -3.0e9)]
        for k, v in enumerate(specials * 3):
            disp[(7 + 37 * k) % h, (5 + 29 * k) % w] = v
    return img, np.ascontiguousarray(disp, f32)


def sample_floor(disp):
    """floor of the sample coordinates of a field, as f64 (no conversion edge in the way)"""
    h, w = disp.shape[:2]
    gx, gy = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    return np.floor((gx - disp[..., 0]).astype(np.float64)), np.floor((gy - disp[..., 1]).astype(np.float64))


def displacement_flags(sw, buf32):
    return (PAIR if sw >= 2 else 0) | (BUF32 if buf32 and sw >= 2 else 0)


# ---- dab lists -----------------------------------------------------------------------------------------------------------------------------------------------------------
# a dab: (mode, cx, cy, delta_x, delta_y, radius, strength)
DabList = collections.namedtuple("DabList", "name size dabs launch")
STROKE_SIZE = (200, 150)


def start_field(w, h):
    """0.0, a lattice of -0.0 and a patch of 3.25"""
    d = np.zeros((h, w, 2), f32)
    d[::7, ::5] = -0.0
    d[h // 3:h // 3 + 10, w // 4:w // 4 + 20] = 3.25
    return d


def stroke(n=200):
    """modes cycling 0..4, 0.5 px apart, radius 20: every pixel near the path is reached by far more than one group of 64"""
    return [(k % 5, 50.0 + 0.5 * k, 60.0 + 0.125 * k, 3.0 - 0.01 * k, -2.0 + 0.02 * k, 20.0, 0.3 + 0.001 * k) for k in range(n)]


def dab_box(d, w, h):
    """the reference's loop bounds x0, y0, x1, y1 (transform.rs:1056-1069: `as i32` saturates, NaN -> 0)"""
    def i32(v):
        v = np.float64(v)
        return 0 if v != v else int(min(max(v, -2147483648.0), 2147483647.0))
    with np.errstate(all="ignore"):
        cx, cy = f32(d[1]), f32(d[2])
        r = f32(d[5]) if f32(d[5]) > f32(1.0) else f32(1.0)       # f32::max: NaN -> 1
        return (max(i32(np.floor(cx - r)), 0), max(i32(np.floor(cy - r)), 0), min(i32(np.ceil(cx + r)), w), min(i32(np.ceil(cy + r)), h))


def reaches_canvas(dabs, w, h):
    return any(b[2] > b[0] and b[3] > b[1] for b in (dab_box(d, w, h) for d in dabs))


EDGE_SIZE = (40, 30)
EDGE_DABS = {   # name: (cx, cy, radius, strength); each runs in every mode
    "radius 0": (20.5, 14.25, 0.0, 0.7), "radius -5": (20.5, 14.25, -5.0, 0.7), "radius +inf": (20.5, 14.25, np.inf, 0.7), "radius NaN": (20.5, 14.25, np.nan, 0.7),
    "radius 1e9": (20.5, 14.25, 1e9, 0.7),
    "centre NaN": (np.nan, 14.25, 9.0, 0.7), "centre NaN y": (20.5, np.nan, 9.0, 0.7), "centre +inf": (np.inf, 14.25, 9.0, 0.7),
    "centre 3e9": (3e9, 14.0, 4e9, 0.7), "centre -3e9": (-3e9, 14.0, 4e9, 0.7), "centre y -3e9": (20.0, -3e9, 4e9, 0.7),
    "strength 0": (20.5, 14.25, 9.0, 0.0), "strength -0.0": (20.5, 14.25, 9.0, -0.0), "strength NaN": (20.5, 14.25, 9.0, np.nan),
    "centre on a pixel": (20.0, 14.0, 9.5, 0.7),
    "centre (-0.5, -0.5)": (-0.5, -0.5, 9.0, 0.7), "centre (w - 0.5, h - 0.5)": (EDGE_SIZE[0] - 0.5, EDGE_SIZE[1] - 0.5, 9.0, 0.7),
    "box one past the left": (4.0, 14.0, 5.0, 0.7), "box one past the top": (20.0, 4.0, 5.0, 0.7),
    "box one past the right": (EDGE_SIZE[0] - 4.0, 14.0, 5.0, 0.7), "box one past the bottom": (20.0, EDGE_SIZE[1] - 4.0, 5.0, 0.7),
    "dist_sq == r * r": (20.0, 14.0, 5.0, 0.7),      # 3-4-5: the test is `>`, so (23, 18) is inside
}


def edge_dab(name, mode):
    cx, cy, radius, strength = EDGE_DABS[name]
    return (mode, cx, cy, 3.0, -2.0, radius, strength)


def spread_list():
    """dabs far apart on a large field: the launch over the chunks their boxes touch.  The common box starts at x = 57, y = 47; the second dab's box ends at
    x = 128 and y = 128 exactly"""
    w, h = 1180, 1100
    rng = np.random.default_rng(21)
    dabs = [(0, 70.0, 60.0, 3.0, -2.0, 13.0, 0.8), (1, 100.0, 100.0, 0.0, 0.0, 28.0, 0.9)]
    centres = [(1100.0, 1040.0), (600.0, 540.0), (1100.0, 150.0), (163.5, 1030.0)]
    for k in range(28):
        cx, cy = centres[k % len(centres)]
        dabs.append((k % 5, cx + float(rng.uniform(-30, 30)), cy + float(rng.uniform(-30, 30)), float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8)),
                     float(rng.uniform(5, 40)), float(rng.uniform(0.1, 1.0))))
    return DabList("spread", (w, h), dabs, DAB_CHUNKED)


def late_list():
    """300 dabs of which only indices >= DAB_CULL reach the canvas: the first trip of the cull loop sees nothing"""
    n0 = consts().dab_cull
    off = [(k % 5, -500.0 - k, 70.0, 1.0, 1.0, 20.0, 0.5) for k in range(n0)]
    return off + [(k % 5, 30.0 + 0.45 * k, 40.0 + 0.2 * k, -2.0 + 0.01 * k, 1.5, 12.0 + (k % 7), 0.4) for k in range(300 - n0)]


@functools.lru_cache(maxsize=None)
def dab_lists():
    n0 = consts().dab_cull
    s = stroke()
    return (DabList("stroke", STROKE_SIZE, s, DAB_PLAIN), DabList("stroke reversed", STROKE_SIZE, s[::-1], DAB_PLAIN),
            DabList("exactly one trip", STROKE_SIZE, stroke(n0), DAB_PLAIN), DabList("one dab into the second trip", STROKE_SIZE, stroke(n0 + 1), DAB_PLAIN),
            DabList("late", STROKE_SIZE, late_list(), DAB_PLAIN), spread_list())


def apply_dabs(field, dabs):
    """the oracle, dab by dab, in place"""
    from . import oracle_lib as O
    for d in dabs:
        O.displacement_brush(field, *d)
    return field


def same_field(got, want):
    """fields as bits; where the oracle has a NaN the device must have one (x86 and the GPU make different default NaNs), everywhere else the same bits"""
    g, w_ = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(w_)
    return g.shape == w_.shape and bool(np.isnan(g[nan]).all()) and np.array_equal(g.view(np.uint32)[~nan], w_.view(np.uint32)[~nan])
