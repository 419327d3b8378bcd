"""An exact float64 model of the default-mode Gaussian's arithmetic, and a checker that holds device output to it.

TEST INFRASTRUCTURE ONLY (like oracle_lib.py): no product code imports it.

What the device computes
------------------------
Matrix-core kernel (k_gauss.hip: gauss_strip_kernel / gauss_strip64_kernel, radius 1 .. 80, out of place).  With the
library's own tap table w'_t (pfx_gaussian_f16_tables, third part at offset 48: ONE f16 per tap, ~ RN(256 w_t), nudged so
that the table keeps the exact taps' sum) and clamp-to-edge sampling, the shipped build ("gauss_parts" = 12) computes

    H[y, x] = sum_t p[y, clamp(x + t - r)] * w'_t             ("scaled units": 256 x an LSB; H < 255 * 256)
    V[y, x] = sum_s H[clamp(y + s - r), x] * w'_s             (2^16 x an LSB)
    out     = RNE_sat_u8(V * 2^-16)                           (v_cvt_pk_u8_f32: nearest, ties to even, saturating)

and ``model_mfma`` returns m = V * 2^-16 evaluated exactly in float64 (as BLAS products over banded matrices; float64's own
error is below 2^-30 LSB and is part of eps).  "gauss_parts" = 22 weights with two f16 pieces w1 + w2 (parts 0 and 1 of
the table) and its vertical pass multiplies h1*w1 + h1*w2 + h2*w1: the model evaluates the same with the dropped h2*w2
computed from the model's own split of H.  ("gauss_parts" = 11 rounds H to ONE f16 before the vertical pass; not modelled —
its own +-1 LSB test covers it.)

The VALU kernels (k_gauss.hip: gauss_h_kernel / gauss_v_kernel, EXACT = false) take radius 81 .. 850 and every in-place
call: fmaf in ascending tap order over the reference's f32 taps, f32 intermediate, round half away.  ``model_valu`` is the
float64 convolution with those f32 taps (O.gaussian_kernel).

The bound eps (LSB) — derived from k_gauss.hip:225-256 (operands, encoding) and :436-452 (the split), not tuned
-----------------------------------------------------------------------------------------------------------------------
Every MFMA product is exact in f32: a sample is 1024 + b (0x6400 | b, exact in f16), a tap and a piece of H are f16, so a
product has at most 22 significant bits.  What rounds is each f32 accumulation; the MFMA's internal summation order is
unspecified, so every product is bounded as its own rounding of at most half an ulp of the largest magnitude its chain can
reach, in any order.  NKB = ((32 + R8 + r + 15) / 16 + 1) & ~1 K blocks of 16 products per chain, R8 = r rounded up to 16
(nkb(); 4, 6, 8, 10, 12).

H pass, parts 12 (one chain).  It starts at -bias_single = -f32(1024 * sum w') ~ -2^18 and adds (1024 + p) w' >= 0, ending at
H < 2^16; every partial sum, and every partial sum of products alone (<= 1279 * 256 < 2^19), is below 2^19 in magnitude, where
half an ulp is 2^-6.  16 NKB roundings + the f32 rounding of bias_single itself:

    e_H <= (16 NKB + 1) * 2^-6 scaled units.

Parts 22: a second chain of (1024 + p) * w2 (|w2| <= 2^-11 w1, so |chain| <= 1279 * 256 * 2^-11 < 2^8: 16 NKB roundings of
2^-16) and one more rounding where the two chains are added (result < 2^16: 2^-8).

Split (:444-448).  hi = RTZ_f16(H), and H - hi is exact in f32; lo = RTZ_f16(H - hi) loses less than one f16 ulp
of a number below one f16 ulp of H: < 2^-21 relative (2^-24 absolute where lo is subnormal), always toward zero.  Through the
vertical weights (sum 256): e_split <= (2^-21 * 2^16 + 2^-24) * 256 ~ 2^3 V units.

V pass, parts 12.  accA = sum h1 w' stays below 255 * 2^16 < 2^24 (half ulp 2^-1); accX = sum h2 w' is far smaller (|h2| < 2^5);
both are bounded by 2^-1 per product: 2 * 16 NKB roundings, + 1 for accA + accX.  The final * 2^-16 is exact.

    e_V <= (2 * 16 NKB + 1) * 2^-1 V units.

Parts 22 adds a third product per tap (accX = h1 w2 + h2 w1): 3 * 16 NKB + 1 roundings, and the model's dropped h2 w2 can
differ from the kernel's where the two split H at different f16 boundaries: |h2 w2| <= 2^5 * sum|w2| <= 2^5 * 2^-3 per side,
2^3 V units.

An error of e scaled units in H moves V by at most e * sum w' = 256 e V units, so in LSB

    eps_mfma = (256 e_H + e_split + e_V) * 2^-16 + 2^-30
             = 0.0051 (4 K blocks) .. 0.0148 (12 K blocks) LSB for parts 12.

VALU path: each fmaf rounds an accumulator of magnitude <= 255 by at most 255 * 2^-24, 2r + 1 of them per pass, two passes
(the horizontal error passes through vertical taps summing to ~1); the model uses the f32 taps themselves, so the tap term of
the issue's formula is zero:  eps_valu = 2 (2r + 1) * 255 * 2^-24 + 2^-30.

The checker
-----------
``check(m, eps, dev)``: where |m - (k + 1/2)| > eps for every integer k the device byte must equal clamp(round(m)); inside that
band either neighbour is accepted; everywhere |dev - clamp(m)| <= 1/2 + eps.  The share of channels inside the band is
returned and must stay below 8 eps + 1 % (so a large eps cannot make a test vacuous).

``true_gaussian_bound(sigma, eps)``: |dev - G64(img)| <= 1/2 + 2 sum|delta| * 255 / 256 + eps, G64 = float64 convolution with
the reference's f32 taps, delta_t = w'_t - 256 w_t (DESIGN §4.2's per-pass bound on the table, turned into an assertion).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from . import oracle_lib as O

MFMA_MAXR = 80   # k_gauss.hip GM_MAXR
WLEN, WOFF = 256, 48


def radius_of(sigma: float) -> int:
    """ceil(3 sigma) in f32, as the reference and the library compute it"""
    return int(np.ceil(np.float32(sigma) * np.float32(3.0)))


def sigma_for_radius(r: int) -> float:
    s = (r - 0.4) / 3.0
    assert radius_of(s) == r, (r, s)
    return s


def nkb(r: int) -> int:
    """K blocks per MFMA chain (k_gauss.hip launch_gauss_mfma)"""
    r8 = (r + 15) & ~15
    return ((32 + r8 + r + 15) // 16 + 1) & ~1


@lru_cache(maxsize=None)
def f16_tables(sigma: float):
    """(w1, w2, ws) as float64 arrays of the 2r + 1 taps, straight from the library's table builder (pfx_gaussian_f16_tables)"""
    from paintfe_amd import _lib
    lib = _lib.load()
    lib.pfx_gaussian_f16_tables.restype = C.c_int
    tab = (C.c_uint16 * 768)()
    b2, b1 = C.c_float(), C.c_float()
    n = lib.pfx_gaussian_f16_tables(C.c_float(sigma), tab, C.byref(b2), C.byref(b1))
    assert n == 2 * radius_of(sigma) + 1, (sigma, n)
    t = np.frombuffer(tab, dtype=np.uint16).copy()
    parts = [t[p * WLEN + WOFF:p * WLEN + WOFF + n].view(np.float16).astype(np.float64) for p in range(3)]
    return tuple(parts)


@lru_cache(maxsize=None)
def f32_taps(sigma: float) -> np.ndarray:
    """the reference's taps (f32, filters.rs:214-234) as float64 values"""
    return O.gaussian_kernel(sigma).astype(np.float64)


def conv_matrix(n: int, taps, clamp_hi: int | None = None) -> np.ndarray:
    """T[src, dst] = sum of the taps t with clamp(dst + t - r) == src: out = in @ T is the clamp-to-edge correlation.
    clamp_hi: the index the right / bottom edge clamps to (n - 1 unless a test builds a deliberately wrong model)."""
    taps = np.asarray(taps, np.float64)
    r = (len(taps) - 1) // 2
    hi = n - 1 if clamp_hi is None else clamp_hi
    T = np.zeros((n, n), np.float64)
    dst = np.arange(n)
    for t in range(len(taps)):
        np.add.at(T, (np.clip(dst + t - r, 0, hi), dst), taps[t])
    return T


def sep_conv(img, taps_h, taps_v=None, clamp_hi_x=None, clamp_hi_y=None):
    """float64 separable clamp-to-edge convolution of an (h, w, 4) array: horizontal with taps_h, then vertical with taps_v"""
    a = np.asarray(img, np.float64)
    h, w = a.shape[:2]
    taps_v = taps_h if taps_v is None else taps_v
    Th = conv_matrix(w, taps_h, clamp_hi_x)
    Hx = np.einsum("ywc,wx->yxc", a, Th, optimize=True)
    return vert(Hx, taps_v, clamp_hi_y)


def vert(Hx, taps_v, clamp_hi_y=None):
    Tv = conv_matrix(Hx.shape[0], taps_v, clamp_hi_y)
    return np.einsum("syc,sx->xyc", Hx, Tv, optimize=True)


def horiz(img, taps_h, clamp_hi_x=None):
    a = np.asarray(img, np.float64)
    return np.einsum("ywc,wx->yxc", a, conv_matrix(a.shape[1], taps_h, clamp_hi_x), optimize=True)


def rtz_f16(x):
    """round toward zero to binary16 (v_cvt_pkrtz_f16_f32), for |x| < 65504"""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    ulp = np.ldexp(1.0, np.maximum(e - 11, -24))
    return np.trunc(x / ulp) * ulp


def model_mfma(img, sigma: float, parts: int = 12) -> np.ndarray:
    """m (LSB, before the final rounding) of the matrix-core Gaussian at "gauss_parts" = parts (12 shipped, 22)"""
    r = radius_of(sigma)
    assert 1 <= r <= MFMA_MAXR, r
    w1, w2, ws = f16_tables(sigma)
    if parts == 12:
        return sep_conv(img, ws) * 2.0 ** -16
    assert parts == 22, parts
    W = w1 + w2
    H = horiz(img, W)
    h1 = rtz_f16(H)
    h2 = rtz_f16(H - h1)
    return (vert(H, W) - vert(h2, w2)) * 2.0 ** -16


def model_valu(img, sigma: float) -> np.ndarray:
    """m (LSB) of the VALU two-pass Gaussian in the default mode (fmaf, f32 taps)"""
    return sep_conv(img, f32_taps(sigma))


def model_rounded(m) -> np.ndarray:
    return np.clip(np.rint(m), 0, 255).astype(np.uint8)


def eps_mfma(r: int, parts: int = 12) -> float:
    k = 16 * nkb(r)
    if parts == 12:
        e_h = (k + 1) * 2.0 ** -6
        e_v = (2 * k + 1) * 2.0 ** -1
    else:
        e_h = (k + 2) * 2.0 ** -6 + k * 2.0 ** -16
        e_v = (3 * k + 1) * 2.0 ** -1 + 2.0 ** 3
    e_split = (2.0 ** -21 * 2.0 ** 16 + 2.0 ** -24) * 256.0
    return (256.0 * e_h + e_split + e_v) * 2.0 ** -16 + 2.0 ** -30


def eps_valu(r: int) -> float:
    return 2.0 * (2 * r + 1) * 255.0 * 2.0 ** -24 + 2.0 ** -30


def table_delta(sigma: float) -> np.ndarray:
    """delta_t = w'_t - 256 w_t in scaled units (the one-piece table's deviation from the reference's f32 taps)"""
    return f16_tables(sigma)[2] - 256.0 * f32_taps(sigma)


def true_gaussian_bound(sigma: float, eps: float) -> float:
    return 0.5 + 2.0 * np.abs(table_delta(sigma)).sum() * 255.0 / 256.0 + eps


@dataclass
class CheckResult:
    n: int
    ambiguous: float      # share of channels inside the band
    differ: float         # share of channels where the device is not round(m) (inside the band only, or the check fails)
    worst: float          # max |dev - clamp(m)|


def check(m, eps: float, dev, what: str = "", max_ambiguous: float | None = None) -> CheckResult:
    m = np.asarray(m, np.float64)
    d = np.asarray(dev).astype(np.float64)
    assert m.shape == d.shape, (what, m.shape, d.shape)
    dist = np.abs(m - np.floor(m) - 0.5)
    amb = dist <= eps
    want = np.clip(np.rint(m), 0, 255)
    differ = d != want
    bad = differ & ~amb
    far = np.abs(d - np.clip(m, 0, 255)) > 0.5 + eps
    if bad.any() or far.any():
        idx = np.argwhere(bad | far)
        ex = [(tuple(int(v) for v in i), float(m[tuple(i)]), int(d[tuple(i)])) for i in idx[:6]]
        need = float(dist[bad].max()) if bad.any() else float("nan")
        raise AssertionError(f"{what}: {int(bad.sum())} channels differ from the model outside its +-{eps:.4f} LSB band, {int(far.sum())} further "
                             f"than 1/2 + eps; the device would need eps >= {need:.4f}; (index, model, device): {ex}")
    res = CheckResult(int(m.size), float(amb.mean()), float(differ.mean()), float(np.abs(d - np.clip(m, 0, 255)).max()))
    cap = 8.0 * eps + 0.01 if max_ambiguous is None else max_ambiguous
    assert res.ambiguous < cap, f"{what}: {res.ambiguous:.2e} of the channels are inside the band (cap {cap:.2e}): the check would be vacuous"
    return res


def check_true_gaussian(img, sigma: float, eps: float, dev, what: str = "") -> float:
    """|dev - G64(img)| <= true_gaussian_bound(sigma, eps); returns the largest distance seen"""
    g = np.clip(sep_conv(img, f32_taps(sigma)), 0, 255)
    worst = float(np.abs(np.asarray(dev, np.float64) - g).max())
    bound = true_gaussian_bound(sigma, eps)
    assert worst <= bound, f"{what}: {worst:.4f} LSB from the true Gaussian, bound {bound:.4f}"
    return worst


# ------------------------------------------------------------------ inputs

def impulse_image(r: int, sigma: float, variant: int = 0, min_w: int = 200, min_h: int = 200) -> np.ndarray:
    """The test image of radius r (one channel per kind of content):

    R  impulses, 255 on 0 (variant 0) or 0 on 255 (variant 1), on a grid of odd pitch > 2r + 1 whose rows are shifted by one
       column and columns by one row (the grid's column phases mod 64 and row phases mod 32 differ from impulse to impulse and
       between variants), and impulses at distances 0, 1, 2, r/2, r - 1, r, r + 1 from each of the four borders;
    G  hard edges on K-block boundaries (a column and a row that are multiples of 16) and a diagonal edge across every row;
    B  the adversarial sign pattern of the tap errors: 255 - k where delta_{x mod n} > 0, else k (k a different level per row) in the
       top half, the same along columns in the bottom half;
    A  a slow diagonal ramp (slopes 0.37 and 0.61 per pixel, mod 256) whose blur crosses x.5 boundaries everywhere.
    """
    S = (2 * r + 2) | 1
    K = 4
    off = r + 2 + (30 - (r + 2)) % 32 + 5 * variant   # variant 0: the first impulse row is 30 mod 32 (a ring step's second-last row)
    w = max(min_w, off + r + 2 + K * (S + 1) + 3)
    h = max(min_h, off + r + 2 + K * (S + 1) + 3)
    img = np.zeros((h, w, 4), np.uint8)
    fg, bg = (255, 0) if variant == 0 else (0, 255)
    R = np.full((h, w), bg, np.uint8)
    for j in range(K):
        for i in range(K):
            x, y = off + i * S + j, off + j * S + i
            if x < w and y < h:
                R[y, x] = fg
    dists = sorted({0, 1, 2, r // 2, r - 1, r, r + 1})
    for k, dd in enumerate(dists):
        pos = min(off + k * S // 2 + 3, h - 1), min(off + k * S // 2 + 3, w - 1)
        if dd < w: R[pos[0], dd] = fg; R[pos[0], w - 1 - dd] = fg
        if dd < h: R[dd, pos[1]] = fg; R[h - 1 - dd, pos[1]] = fg
    img[..., 0] = R
    xe, ye = 16 * max(1, (w // 2) // 16), 16 * max(1, (h // 2) // 16)
    G = np.zeros((h, w), np.uint8)
    G[:, xe:] = 255
    G[ye:, :] = 255 - G[ye:, :]
    yy, xx = np.mgrid[0:h, 0:w]
    G[xx + 2 * yy > w + h // 3] ^= 255   # and a diagonal one that crosses every row and column
    img[..., 1] = G
    delta = table_delta(sigma) if r <= MFMA_MAXR else np.zeros(2 * r + 1)
    n = len(delta)
    pos = delta > 0
    k = (np.arange(h) * 7 % 97)[:, None]   # a base level per row / column, so that the shifted sums land on every fraction
    top = np.where(pos[np.arange(w) % n][None, :], 255 - k, k)
    bottom = np.where(pos[np.arange(h) % n][:, None], 255 - (np.arange(w) * 7 % 97)[None, :], (np.arange(w) * 7 % 97)[None, :])
    img[..., 2] = np.where(np.arange(h)[:, None] < h // 2, top, bottom).astype(np.uint8)
    img[..., 3] = (np.floor(0.37 * xx + 0.61 * yy + 17 * variant) % 256).astype(np.uint8)
    return img


def crop_mask_model(img, mask, sigma, model):
    """blur_with_selection (filters.rs:141-207) around a model: the bounding box of mask > 0, padded by ceil(3 sigma), is blurred as its
    own image; selected pixels take the blurred value, the others keep the source.  Returns (m, selected) with m = NaN where unselected."""
    sel = mask > 0
    ys, xs = np.nonzero(sel)
    h, w = mask.shape
    pad = radius_of(sigma)
    x0, y0 = max(xs.min() - pad, 0), max(ys.min() - pad, 0)
    x1, y1 = min(xs.max() + 1 + pad, w), min(ys.max() + 1 + pad, h)
    m = np.full(img.shape, np.nan)
    m[y0:y1, x0:x1] = model(img[y0:y1, x0:x1], sigma)
    return m, sel
