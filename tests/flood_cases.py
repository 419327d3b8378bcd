"""Seeded inputs of the flood tests (tests/test_flood_model_host.py, tests/test_gpu_flood.py).  No golden of the reference covers the bucket fill or the magic
wand, so every expectation comes from tests/flood_model.py.  Model results are cached: the host test and the GPU test of one session share them."""
import functools

import numpy as np

from . import flood_model as M

TILE = 64   # the tile edge the sizes below are chosen around (the GPU test checks that the library reports the same)


# ---- images --------------------------------------------------------------------------------------------------------------------------------------------------
def gradient(w, h):
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = (x * 3 + y) % 256
    img[..., 1] = (x + y * 2) // 2 % 256
    img[..., 2] = 255 - (x * 255 // max(w - 1, 1))
    img[..., 3] = 255
    return img


def noise(w, h, seed=11):
    """threshold-scale contrast (steps of a few units around a base colour) with partial alpha"""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 4), np.uint8)
    img[..., :3] = 120 + rng.integers(-40, 41, (h, w, 3))
    img[..., 3] = rng.choice(np.array([255, 255, 200, 128], np.uint8), (h, w))
    return img


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    on = ((x // 8 + y // 8) % 2).astype(bool)
    img = np.empty((h, w, 4), np.uint8)
    img[on] = (200, 180, 40, 255)
    img[~on] = (30, 60, 90, 255)
    img[..., 0] += (x % 5).astype(np.uint8)    # a little texture inside the squares
    return img


def clear_regions(w, h, seed=5):
    """fully transparent stripes (with stale colour bytes) between opaque noise"""
    rng = np.random.default_rng(seed)
    img = noise(w, h, seed)
    img[..., 3] = 255
    y, x = np.mgrid[0:h, 0:w]
    clear = ((x + 2 * y) // 11) % 3 == 0
    img[clear, 3] = 0
    img[clear, :3] = rng.integers(0, 256, (int(clear.sum()), 3))
    return img


def hline(w, h):
    """a one-pixel black line along y = 20 on white: around a seed on the line every other pixel of its tile is at distance 255"""
    img = np.full((h, w, 4), 255, np.uint8)
    img[20, :, :3] = 0
    return img


def cross(w, h):
    """one-pixel black lines along x = 64 and y = 64 on white: the crossing is the corner pixel of a tile"""
    img = np.full((h, w, 4), 255, np.uint8)
    img[64, :, :3] = 0
    img[:, 64, :3] = 0
    return img


IMAGES = {"gradient": gradient, "noise": noise, "checker": checker, "clear": clear_regions, "hline": hline, "cross": cross}

# (name, w, h, image, seed, target or None = the seed's pixel): 1 x 1, single rows / columns, one tile, one tile plus a pixel, 3 x 2 ragged tiles; seeds at a
# corner, on a tile border and inside; every image kind on a multi-tile size
DISTANCE_CASES = [
    ("1x1", 1, 1, "noise", (0, 0), None),
    ("row200", 200, 1, "gradient", (0, 0), None),
    ("col200", 1, 200, "noise", (0, 100), None),
    ("64-checker", 64, 64, "checker", (31, 20), None),
    ("64-clear-corner", 64, 64, "clear", (63, 63), None),
    ("65-noise-border", 65, 65, "noise", (64, 10), None),
    ("65-gradient-border", 65, 65, "gradient", (63, 64), None),
    ("130x70-gradient-corner", 130, 70, "gradient", (0, 0), None),
    ("130x70-noise-border", 130, 70, "noise", (64, 63), None),
    ("130x70-checker-inside", 130, 70, "checker", (100, 40), None),
    ("130x70-clear-inside", 130, 70, "clear", (70, 30), None),
    ("130x70-clear-seed-clear", 130, 70, "clear", (0, 0), (9, 9, 9, 0)),          # a transparent target: every transparent pixel is at distance 0
    ("130x70-noise-target", 130, 70, "noise", (129, 69), (140, 100, 90, 230)),    # a target that is not the seed's pixel
    # a seed that is the only pixel of its tile, or whose in-tile neighbours are all at distance 255: the flood leaves the seed's tile through the seed alone
    ("65x1-seed-alone", 65, 1, "noise", (64, 0), None),
    ("1x65-seed-alone", 1, 65, "gradient", (0, 64), None),
    ("130x70-line-seed-on-border", 130, 70, "hline", (64, 20), None),
    ("130x70-line-seed-right-border", 130, 70, "hline", (63, 20), None),
    ("130x70-cross-seed-on-corner", 130, 70, "cross", (64, 64), None),
    ("130x70-cross-seed-before-corner", 130, 70, "cross", (63, 64), None),
]


def case_image(case):
    name, w, h, kind, seed, target = case
    img = IMAGES[kind](w, h)
    return img, seed, tuple(int(v) for v in (img[seed[1], seed[0]] if target is None else target))


@functools.lru_cache(maxsize=None)
def distance_expected(case_name, mode, connectivity, global_scope, check):
    case = next(c for c in DISTANCE_CASES if c[0] == case_name)
    img, seed, target = case_image(case)
    d = M.distance_map(img, seed, target, mode, connectivity, global_scope, check)
    d.setflags(write=False)
    return d


# ---- corridors: c = 0 .. 40 rising along a one-pixel corridor, walls of 100 .. 250 one pixel thick ---------------------------------------------------------------
def _corridor_image(order, n, seed):
    """order: the corridor's pixels (x, y) from the seed on; everything else is wall.  Encoded so that the legacy distance to (0, 0, 0, 255) is the value."""
    rng = np.random.default_rng(seed)
    v = rng.integers(100, 251, (n, n)).astype(np.uint8)
    for k, (x, y) in enumerate(order):
        v[y, x] = k * 40 // (len(order) - 1)
    img = np.zeros((n, n, 4), np.uint8)
    img[..., 0] = v
    img[..., 3] = 255
    return img


def snake(n=129):
    """even rows are corridor; odd rows are wall but for one connecting pixel, alternately at the right and the left end"""
    order = []
    for y in range(0, n, 2):
        xs = range(n) if (y // 2) % 2 == 0 else range(n - 1, -1, -1)
        order += [(x, y) for x in xs]
        if y + 2 < n:
            order.append((order[-1][0], y + 1))
    return _corridor_image(order, n, 3), order


def spiral(n=129):
    carved = np.zeros((n, n), bool)
    x, y, (dx, dy) = 0, 0, (1, 0)
    order = [(0, 0)]
    carved[0, 0] = True

    def free(px, py):
        return 0 <= px < n and 0 <= py < n and not carved[py, px]

    while True:
        for _ in range(2):
            ahead_ok = free(x + dx, y + dy) and (not (0 <= x + 2 * dx < n and 0 <= y + 2 * dy < n) or not carved[y + 2 * dy, x + 2 * dx])
            if ahead_ok:
                break
            dx, dy = -dy, dx     # turn right (y grows downwards)
        else:
            break
        x, y = x + dx, y + dy
        carved[y, x] = True
        order.append((x, y))
    return _corridor_image(order, n, 4), order


def long_snake():
    """the snake over 4 x 4 tiles: every corridor row crosses three tile borders and comes back through the tiles it left two rows later, so a tile is listed
    in hundreds of passes and its stamp changes as often"""
    return snake(LONG_SNAKE_N)


LONG_SNAKE_N = 3 * TILE + 1
CORRIDORS = {"snake": snake, "spiral": spiral, "long_snake": long_snake}
CORRIDOR_TARGET = (0, 0, 0, 255)


@functools.lru_cache(maxsize=None)
def corridor_expected(name, connectivity, check):
    img, order = CORRIDORS[name]()
    d = M.distance_map(img, order[0], CORRIDOR_TARGET, M.LEGACY, connectivity, False, check)
    d.setflags(write=False)
    return d


# ---- pass-count images ---------------------------------------------------------------------------------------------------------------------------------------
def uniform(tiles_x=3, tiles_y=2, tile=TILE):
    img = np.empty((tiles_y * tile, tiles_x * tile, 4), np.uint8)
    img[...] = (90, 120, 150, 255)
    return img


def walled(tiles_x=3, tiles_y=2, tile=TILE):
    """a uniform black image with the seed (5, 5) closed in, inside the first tile, by a wall at distance 255: nothing beyond it can drop below its initial 255"""
    img = uniform(tiles_x, tiles_y, tile)
    img[...] = (0, 0, 0, 255)
    img[40, :41] = (255, 255, 255, 255)
    img[:41, 40] = (255, 255, 255, 255)
    return img


# ---- many tiles in flight ------------------------------------------------------------------------------------------------------------------------------------------
# 9 x 7 whole tiles and one ragged pixel in each direction: 10 x 8 = 80 tiles, so a pass's tile list holds many tiles and the lists, the stamps and the
# "visit only listed tiles" schedule work with more than a handful
MANY_TILES_X, MANY_TILES_Y = 10, 8
MANY_W, MANY_H = 9 * TILE + 1, 7 * TILE + 1
MANY_SEEDS = {"corner": (0, 0), "centre": (MANY_W // 2, MANY_H // 2)}


def uniform_many():
    img = np.empty((MANY_H, MANY_W, 4), np.uint8)
    img[...] = (90, 120, 150, 255)
    return img


# a half-transparent target: the opaque noise and the transparent stripes of `clear` are both about 127 from it, so the flood crosses the stripes and
# reaches every tile (from the seed's own pixel the stripes are walls at 255 and the flood stays in one band).  In the perceptual mode the alpha term
# decides and the map has two values, 127 in the seed's band and 128 beyond it: little to compare, but every tile is still listed and lowered
HALF_CLEAR = (120, 120, 120, 128)

# (name, w, h, image, seed, target or None) like DISTANCE_CASES; the seed of the two 80-tile images is a tile corner, the strips are 40 tiles one pixel short
MANY_TILE_CASES = [
    ("many-noise-tile-corner", MANY_W, MANY_H, "noise", (4 * TILE, 3 * TILE), None),
    ("many-clear-tile-corner", MANY_W, MANY_H, "clear", (3 * TILE, 4 * TILE), HALF_CLEAR),
    ("wide-40x1-tiles", 40 * TILE - 1, TILE - 1, "clear", (0, 30), HALF_CLEAR),
    ("tall-1x40-tiles", TILE - 1, 40 * TILE - 1, "noise", (31, 40 * TILE - 2), (120, 120, 120, 255)),
]
# (mode, connectivity) pairs the many-tile cases run in, each in both scopes: both modes and both connectivities without the full cross product (a Dijkstra of
# the model over 260 000 pixels takes a second or two)
MANY_TILE_RUNS = [(M.LEGACY, 4), (M.PERCEPTUAL, 8)]


@functools.lru_cache(maxsize=None)
def many_tile_expected(case_name, mode, connectivity, global_scope):
    """Dijkstra alone: test_flood_model_host.py holds it to the relaxation where that is quick enough"""
    case = next(c for c in MANY_TILE_CASES if c[0] == case_name)
    img, seed, target = case_image(case)
    d = M.distance_map(img, seed, target, mode, connectivity, global_scope, False)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def uniform_many_expected(where, connectivity):
    img = uniform_many()
    seed = MANY_SEEDS[where]
    d = M.distance_map(img, seed, img[seed[1], seed[0]], M.LEGACY, connectivity, False, False)
    d.setflags(write=False)
    return d


def tile_count(w, h, tile=TILE):
    return ((w + tile - 1) // tile) * ((h + tile - 1) // tile)


# ---- threshold-stage inputs ------------------------------------------------------------------------------------------------------------------------------------
THRESHOLDS = [0, 1, 37, 254, 255]


def ramp_distance(w=130, h=70):
    """a distance map that holds every byte value, 0 .. 255: what the mask, box and preview kernels are swept over"""
    y, x = np.mgrid[0:h, 0:w]
    d = ((x * 2 + y * 3) % 256).astype(np.uint8)
    d[:4, :8] = 255
    return d


def base_mask(w=130, h=70, seed=21):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0, 255, 255, 128, 7, 200], np.uint8), (h, w))


def selection(w=130, h=70):
    y, x = np.mgrid[0:h, 0:w]
    sel = np.zeros((h, w), np.uint8)
    sel[(x - 60) ** 2 + (y - 30) ** 2 < 45 ** 2] = 255
    sel[10:20, 5:50] = 1      # > 0 counts as selected
    return sel


def layer(w=130, h=70, seed=31):
    """a layer for the fill: flat regions the bucket can flood, with partial alpha"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 4), np.uint8)
    region = (x // 33 + 2 * (y // 29)) % 4
    palette = np.array([(200, 60, 40, 255), (40, 200, 90, 255), (60, 80, 220, 180), (0, 0, 0, 0)], np.uint8)
    img[...] = palette[region]
    img[..., :3] = np.clip(img[..., :3].astype(np.int16) + rng.integers(-6, 7, (h, w, 3)) * (region[..., None] != 3), 0, 255)
    return img
