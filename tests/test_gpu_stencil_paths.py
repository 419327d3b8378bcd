"""Every median and box-blur kernel family a knob can reach, once each: the result against the oracle at tolerance 0, and the path the call took —
read back from the context (pfx_int_stencil_last_path) — against the family the case names and against what the pure decision (pfx_int_median_path,
pfx_int_box_plan; tests/test_stencil_dispatch_host.py holds it to the rules) gives for the same knobs.  A knob that pfx_tune dropped on the way to the
launcher would leave the pixels right and show here.  131 x 37 takes the unaligned instantiations, 132 x 37 (w % 4 == 0) the aligned ones."""
import ctypes as C

import numpy as np
import pytest

from . import inputs as I
from . import oracle_lib as O
from .test_stencil_dispatch_host import (B_DEFAULTS, M_DEFAULTS, MEDIAN, PREFIX, SLIDING, STRIP, TILE, TWO_PASS, BoxCase, BoxPlan, MedianCase)

pytestmark = pytest.mark.gpu

SIZES = ((131, 37), (132, 37))
M_KEYS = {"bits_min": "median_bits_min", "xlane": "median_xlane", "single": "median_single", "search1": "median_search1", "pair": "median_pair"}
B_KEYS = {"strip": "box_strip", "two_pass": "box_two_pass", "prefix_from": "box_prefix_from", "px_force": "box_px", "py_force": "box_py",
          "px_switch": "box_px_switch", "py_switch": "box_py_switch"}

# (path, radius, knobs)
MEDIAN_CASES = [("N", 1, {}), ("X", 2, {}), ("R", 2, dict(xlane=2)), ("7", 3, dict(xlane=5))] + \
               [("H", r, dict(xlane=0, bits_min=9)) for r in (2, 3, 4)] + [("G", r, dict(single=1, bits_min=9)) for r in (2, 3)] + \
               [("P", 3, {}), ("P", 7, {}), ("b", 3, dict(pair=0)), ("b", 8, {}), ("4", 5, dict(bits_min=9)), ("1", 5, dict(bits_min=9, search1=1)), ("I", 25, {})]
# (kind, h_kind or None, radius, knobs)
BOX_CASES = [(TILE, None, 2, dict(strip=1)), (STRIP, None, 2, {}), (STRIP, None, 9, {}), (TWO_PASS, SLIDING, 9, dict(strip=0)),
             (TWO_PASS, PREFIX, 9, dict(strip=0, prefix_from=1))]


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    g = GpuBackend(0)
    L = g.r._lib
    L.pfx_int_stencil_last_path.argtypes = [C.c_void_p, C.c_int]
    L.pfx_int_stencil_last_path.restype = C.c_int
    L.pfx_int_median_path.argtypes = [C.POINTER(MedianCase)]
    L.pfx_int_median_path.restype = C.c_int
    L.pfx_int_box_plan.argtypes = [C.POINTER(BoxCase), C.POINTER(BoxPlan)]
    L.pfx_int_box_plan.restype = C.c_int
    return g


@pytest.fixture(scope="module")
def images():
    out = {}
    for w, h in SIZES:
        img = I.random_rgba(w, h, 5000 + w)
        img[: h // 2] = (img[: h // 2] // 86) * 86   # ties
        out[(w, h)] = (img, (np.random.default_rng(w).random((h, w)) < 0.5).astype(np.uint8) * 255)
    return out


@pytest.fixture(scope="module")
def refs(images):
    """oracle results, computed once per (op, radius, size, masked)"""
    cache = {}

    def get(op, radius, size, masked):
        key = (op, radius, size, masked)
        if key not in cache:
            img, mask = images[size]
            cache[key] = (O.median if op == "median" else O.box_blur)(img, radius, mask if masked else None)
        return cache[key]
    return get


def last_path(gpu, which):
    return gpu.r._lib.pfx_int_stencil_last_path(gpu.r._h, which)


def tuned(gpu, keys, defaults, knobs):
    """context manager: the knobs set through pfx_tune, the defaults back in the end"""
    class scope:
        def __enter__(self):
            for k, v in knobs.items():
                gpu.r.tune(keys[k], v)

        def __exit__(self, *exc):
            for k in knobs:
                gpu.r.tune(keys[k], defaults[k])
    return scope()


def packed(p):
    return p.kind | p.h_kind << 4 | p.px << 8 | p.py << 16


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("case", MEDIAN_CASES, ids=lambda c: f"{c[0]}-r{c[1]}")
def test_median_path(gpu, images, refs, case, size):
    letter, radius, knobs = case
    img, mask = images[size]
    k = dict(M_DEFAULTS, **knobs)
    pure = gpu.r._lib.pfx_int_median_path(C.byref(MedianCase(radius, k["bits_min"], k["xlane"], k["single"], k["search1"], k["pair"])))
    with tuned(gpu, M_KEYS, M_DEFAULTS, knobs):
        for masked in (False, True):
            got = gpu.median(img, radius, mask if masked else None)
            assert last_path(gpu, 0) == MEDIAN[letter], (case, size, masked)
            assert last_path(gpu, 0) == pure, (case, size, masked)
            assert np.array_equal(got, refs("median", radius, size, masked)), (case, size, masked)


def test_median_bits_min_below_two_leaves_radius_one_on_the_3x3_network(gpu, images, refs):
    """pfx_tune "median_bits_min" = 1 used to send radius 1 to the bit-plane select, which has no such build: PFX_ERR_HIP"""
    size = SIZES[0]
    img, mask = images[size]
    with tuned(gpu, M_KEYS, M_DEFAULTS, dict(bits_min=1)):
        assert np.array_equal(gpu.median(img, 1), refs("median", 1, size, False))
        assert last_path(gpu, 0) == MEDIAN["N"]
        assert np.array_equal(gpu.median(img, 1, mask), refs("median", 1, size, True))


def box_pure(gpu, radius, in_place, size, knobs):
    k = dict(B_DEFAULTS, **knobs)
    p = BoxPlan()
    c = BoxCase(radius, in_place, size[0], size[1], k["strip"], k["two_pass"], k["prefix_from"], k["px_force"], k["py_force"], k["px_switch"], k["py_switch"])
    gpu.r._lib.pfx_int_box_plan(C.byref(c), C.byref(p))
    return p


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("case", BOX_CASES, ids=lambda c: f"{c[0]}-{c[1]}-r{c[2]}")
def test_box_plan(gpu, images, refs, case, size):
    kind, h_kind, radius, knobs = case
    img, mask = images[size]
    pure = box_pure(gpu, radius, 0, size, knobs)
    with tuned(gpu, B_KEYS, B_DEFAULTS, knobs):
        for masked in (False, True):
            got = gpu.box_blur(img, float(radius), mask if masked else None)
            lp = last_path(gpu, 1)
            assert lp & 15 == kind and (h_kind is None or (lp >> 4) & 15 == h_kind), (case, size, masked, hex(lp))
            assert lp == packed(pure), (case, size, masked, hex(lp))
            assert np.array_equal(got, refs("box", float(radius), size, masked)), (case, size, masked)


@pytest.mark.parametrize("size", SIZES)
def test_box_in_place_takes_the_two_passes(gpu, images, refs, size):
    """src == dst through pfx_box_blur_dev: the fused kernels would read what their neighbours have written"""
    r = gpu.r
    w, h = size
    img, mask = images[size]
    pure = box_pure(gpu, 3, 1, size, {})
    a, m = r.dev_alloc(img.nbytes), r.dev_alloc(mask.nbytes)
    try:
        r.dev_upload(m, mask)
        for masked in (False, True):
            r.dev_upload(a, img)
            r.box_blur_dev(a, a, w, h, 3.0, mask_ptr=m if masked else 0)
            r.synchronize()
            lp = last_path(gpu, 1)
            assert lp & 15 == TWO_PASS and lp == packed(pure), (size, masked, hex(lp))
            assert np.array_equal(r.dev_download(a, img.shape), refs("box", 3.0, size, masked)), (size, masked)
    finally:
        r.dev_free(a)
        r.dev_free(m)
