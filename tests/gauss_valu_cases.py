"""The case tables of the two-pass VALU Gaussian (k_gauss.hip: gauss_h_kernel / gauss_v_kernel), shared by the host tests
(tests/test_gauss_valu_cases_host.py) and the GPU tests (tests/test_gpu_gauss_valu_edges.py).

TEST INFRASTRUCTURE ONLY (like oracle_lib.py and gauss_model.py): no product code imports it.

Radii: both sides of every switch point of the path choice (16|17 fused exact, 48|49 and 80|81 matrix-core) and of the vertical tile
choice (110|111, 160|161, 240|241, 340|341, 380|381), one deep inside the 4-column tile's range and the largest radius there is.

Shapes (w, h) per radius r, each the smallest that reaches its edge:
  (13, 2r + 140)                     taller than the window (interior rows exist), crosses a vertical tile of every height, and 13 columns
                                     leave a partial last tile for 4, 8 and 16 columns;
  (2r + 1040, 5)                     wider than the window and past the first 1024-pixel horizontal tile;
  (1023, 3), (1024, 3), (1025, 3)    both sides of the horizontal tile's edge;
  (3, rows - 1), (4, rows), (5, rows + 1)   both sides of the chosen vertical tile's row count, and (with the 13-column shape) of its columns;
  (1, 1), (1, 70), (70, 1)           degenerate sizes.

Images: seeded noise whose lower half (tall shapes) or right half (wide shapes) is divided by 4, so that the blurred bytes range over many
values instead of sitting at 127.

``restate`` is a numpy float32 restatement of the reference's arithmetic, with the mutants the host tests use to show that the rows can see a
dropped tap or a wrong clamp."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np

from . import gauss_model as G
from . import oracle_lib as O

LDS_LIMIT = 160 * 1024
MAX_RADIUS = 850   # pfxk_gauss_max_radius(); the host test asserts it
H_TILE = 1024      # k_gauss.hip: pixels per block of the horizontal pass

RADII = (17, 48, 49, 80, 81, 110, 111, 160, 161, 240, 241, 340, 341, 380, 381, 600, 850)

# the vertical tile shapes by config index: (columns, output rows, LDS row stride in float4); k_gauss.hip V_TILES
V_TILES = ((8, 128, 10), (16, 256, 16), (4, 256, 5), (8, 256, 10), (8, 512, 10))
V_SLACK = 4

# radius -> the "gauss_v_cfg" values to force; 0 is the shipped choice that the others must reproduce
FORCED = {49: (0, 1, 2, 3, 4), 110: (0, 1, 2, 3, 4), 190: (0, 1, 2, 3, 4), 254: (0, 2, 3, 4)}
REFUSED = (300, 1)   # (260 + 600) rows x 16 float4 x 16 B = 220160 B > 160 KiB


@lru_cache(maxsize=None)
def _lib():
    from paintfe_amd import _lib as L
    lib = L.load()
    lib.pfxk_gauss_v_tile.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    lib.pfxk_gauss_v_tile.restype = C.c_int
    lib.pfxk_gauss_h_lds_bytes.argtypes = [C.c_int]
    lib.pfxk_gauss_h_lds_bytes.restype = C.c_size_t
    lib.pfxk_gauss_max_radius.argtypes = []
    lib.pfxk_gauss_max_radius.restype = C.c_int
    return lib


def v_tile(radius: int, knob: int = 0):
    """(config index, columns, output rows, LDS bytes) from the library's own decision (pfxk_gauss_v_tile); needs no device"""
    tx, rows, lds = C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    cfg = _lib().pfxk_gauss_v_tile(radius, knob, C.byref(tx), C.byref(rows), C.byref(lds))
    return cfg, tx.value, rows.value, lds.value


def h_lds_bytes(radius: int) -> int:
    return int(_lib().pfxk_gauss_h_lds_bytes(radius))


def max_radius() -> int:
    return int(_lib().pfxk_gauss_max_radius())


def tall_shape(r: int):
    return (13, 2 * r + 140)


def wide_shape(r: int):
    return (2 * r + 1040, 5)


def tile_edge_shapes(rows: int):
    return [(3, rows - 1), (4, rows), (5, rows + 1)]


def shapes(r: int, knob: int = 0):
    """the (w, h) rows of radius r; the tile-edge shapes follow the tile that the library chooses under `knob`"""
    rows = v_tile(r, knob)[2]
    return [tall_shape(r), wide_shape(r), (H_TILE - 1, 3), (H_TILE, 3), (H_TILE + 1, 3)] + tile_edge_shapes(rows) + [(1, 1), (1, 70), (70, 1)]


def forced_shapes(r: int, knob: int):
    """rows for a forced tile: the tall shape, the forced tile's own edges, and 17 columns (a full 16-column tile and a 1-column one)"""
    rows = v_tile(r, knob)[2]
    return [tall_shape(r)] + tile_edge_shapes(rows) + [(17, 131)]


def image(w: int, h: int, r: int) -> np.ndarray:
    """seeded noise; the lower half (h >= w) or the right half (w > h) divided by 4"""
    rng = np.random.default_rng([0x6A55, w, h, r])
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if h >= w:
        img[h // 2:] //= 4
    else:
        img[:, w // 2:] //= 4
    return img


@lru_cache(maxsize=None)
def _oracle(w: int, h: int, r: int) -> np.ndarray:
    out = O.gaussian_blur(image(w, h, r), G.sigma_for_radius(r))
    out.setflags(write=False)
    return out


def oracle(w: int, h: int, r: int) -> np.ndarray:
    """the reference's blur of image(w, h, r) at sigma_for_radius(r): computed once per row, shared, read-only"""
    return _oracle(w, h, r)


# ------------------------------------------------------------------ the reference restated, and its mutants

def one_pass(a: np.ndarray, taps: np.ndarray, axis: int, drop=None, clamp_hi=None, descending=False) -> np.ndarray:
    """one clamp-to-edge pass along `axis` in float32: acc = acc + sample * tap (two roundings), taps ascending.
    drop: index of a tap to leave out; clamp_hi: the index the far edge clamps to (n - 1 in the reference); descending: mutant tap order"""
    a = np.moveaxis(np.asarray(a, np.float32), axis, 0)
    n = a.shape[0]
    klen = len(taps)
    r = (klen - 1) // 2
    hi = n - 1 if clamp_hi is None else max(clamp_hi, 0)
    padded = a[np.clip(np.arange(-r, n + r), 0, hi)]   # padded[i + t] = a[clamp(i + t - r)]
    acc = np.zeros_like(a)
    order = range(klen - 1, -1, -1) if descending else range(klen)
    for t in order:
        if t == drop:
            continue
        acc = acc + padded[t:t + n] * taps[t]
    return np.moveaxis(acc, 0, axis)


def round_half_away(v: np.ndarray) -> np.ndarray:
    """f32::round() then the saturating cast to u8, without forming v + 0.5 (which rounds)"""
    f = np.floor(v)
    return np.clip(f + ((v - f) >= np.float32(0.5)), 0, 255).astype(np.uint8)


def restate(img: np.ndarray, sigma: float, h_kw=None, v_kw=None) -> np.ndarray:
    """the reference's Gaussian: u8 -> f32 horizontal pass, f32 -> u8 vertical pass, round half away from zero.
    h_kw / v_kw: mutant arguments of one_pass for the horizontal / vertical pass"""
    taps = O.gaussian_kernel(sigma)
    assert taps.dtype == np.float32 and len(taps) == 2 * G.radius_of(sigma) + 1
    hx = one_pass(img, taps, 1, **(h_kw or {}))
    return round_half_away(one_pass(hx, taps, 0, **(v_kw or {})))


def mutants(r: int, n_long: int):
    """name -> one_pass arguments, for the pass that runs along the long axis (n_long samples)"""
    return {"first tap dropped": dict(drop=0), "last tap dropped": dict(drop=2 * r), "centre tap dropped": dict(drop=r),
            "clamp at n - 2": dict(clamp_hi=n_long - 2)}
