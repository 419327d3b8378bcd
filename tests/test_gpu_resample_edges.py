"""Parity (GPU): resize_image and the layer affine at their kernels' own edges, against the CPU oracle at tolerance 0.  The shapes come from
tests/resize_model.py; tests/test_resize_model_host.py shows on the host what each reaches.

resize: every case asserts the path the library reports (pfx_int_resize_last: the device copy, the fused kernel, the two passes) and its span_max
against the model's, so a case written for one kernel cannot silently run on the other; every case also runs with `resize_two_pass` forced and must
give the same bytes.

affine: pure translations whose samples land on, and a quarter either side of, x0 / y0 = -2, -1, 0, n - 2, n - 1, n (and the nearest-neighbour .5 ties) for
sources from 1 x 1 and canvases on the 64 x 4 block edges; scales on both sides of |scale| > 1e-6; right angles about x and y with the offsets that put a
row / column of pixels on |w| < 1e-8; saturating offsets; NaN and +-inf in every parameter.  The |det| < 1e-12 identity branch of invert_3x3 is reachable —
rotation_x = rotation_y = 90 on the 1 x 1 canvas (focal^3 * 1.9e-15) — and is one of the rows; on the larger canvases the same angles invert.
"""
import ctypes as C
import time

import numpy as np
import pytest

from . import inputs as I
from . import oracle_lib as O
from . import resize_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    g = GpuBackend(0)
    g.r._lib.pfx_int_resize_last.argtypes = [C.c_void_p, C.c_int]
    g.r._lib.pfx_int_resize_last.restype = C.c_int
    return g


def resize_last(gpu):
    return gpu.r._lib.pfx_int_resize_last(gpu.r._h, 0), gpu.r._lib.pfx_int_resize_last(gpu.r._h, 1)


def same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = (got != ref).any(-1)
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} pixels differ, first at x={x} y={y}: device {got[y, x].tolist()} oracle {ref[y, x].tolist()}")


def source(w, h):
    img = I.random_rgba(w, h, 7000 + 3 * w + h)
    img[::3, ::5] = 255   # saturated neighbours: the negative lobes of bicubic / lanczos3 overshoot and clamp
    img[1::4, 2::7] = 0
    return img


@pytest.mark.parametrize("name,src,dst,filters", M.resize_cases(), ids=[c[0] for c in M.resize_cases()])
def test_resize_edges_vs_oracle(gpu, name, src, dst, filters):
    (w, h), (nw, nh) = src, dst
    img = source(w, h)
    for f in filters:
        ref = O.resize(img, nw, nh, f)
        span = 0 if (nw, nh) == (w, h) else M.span_max(w, nw, f)
        for two_pass in (0, 1):
            gpu.r.tune("resize_two_pass", two_pass)
            try:
                got = gpu.r.resize_image(img, nw, nh, f)
                ran = resize_last(gpu)
            finally:
                gpu.r.tune("resize_two_pass", 0)
            what = f"{name} {f} {w}x{h}->{nw}x{nh} two_pass={two_pass}"
            assert ran == (M.path(w, h, nw, nh, f, bool(two_pass)), span), f"{what}: ran (path, span_max) = {ran}"
            same(got, ref, what)


def test_resize_getter_says_fused_fused_two_pass_across_the_lds_limit(gpu):
    img = {}
    for f in M.FILTERS:
        paths = []
        for span in (511, 512, 513):
            w = M._span_width(span, f)
            img.setdefault(w, source(w, 12))
            gpu.r.resize_image(img[w], 64, 5, f)
            paths.append(resize_last(gpu))
        assert paths == [(M.FUSED, 511), (M.FUSED, 512), (M.TWO_PASS, 513)], (f, paths)


# ---------------------------------------------------------------------------------------------------------------------------------- affine
def affine_both(gpu, img, cw, ch, what, **kw):
    for interp in ("bilinear", "nearest"):
        same(gpu.r.affine_transform(img, cw, ch, interpolation=interp, **kw), O.affine(img, cw, ch, interpolation=interp, **kw), f"{what} {interp}")


@pytest.mark.parametrize("src", M.AFFINE_SOURCES, ids=[f"{w}x{h}" for w, h in M.AFFINE_SOURCES])
def test_affine_translations_on_and_around_every_border(gpu, src):
    sw, sh = src
    img = source(sw, sh)
    img[..., 3] = np.maximum(img[..., 3], 1)
    t0, n = time.perf_counter(), 0
    for (cw, ch) in M.AFFINE_CANVASES:
        for off in M.border_offsets(sw, sh):
            affine_both(gpu, img, cw, ch, f"source {sw}x{sh} canvas {cw}x{ch} offset {off}", offset=off)
            n += 2
    print(f"{sw}x{sh}: {n} device runs, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("src", [(2, 2), (64, 4), (65, 5), (1, 9)], ids=["2x2", "64x4", "65x5", "1x9"])
def test_affine_parameter_edges(gpu, src):
    sw, sh = src
    img = source(sw, sh)
    for (cw, ch) in M.AFFINE_CANVASES:
        for kw in M.affine_param_cases():
            affine_both(gpu, img, cw, ch, f"source {sw}x{sh} canvas {cw}x{ch} {kw}", **kw)


def test_affine_w_zero_rows_are_left_transparent(gpu):
    """M.W_ZERO_CASES on their canvas against a large opaque source: the row / column whose |w| < 1e-8 stays 0 (the plane is edge-on: the other pixels map
    far outside or, about y, onto the source)"""
    cw, ch = M.W_ZERO_CANVAS
    img = np.full((40, 200, 4), 255, np.uint8)
    for kw in M.W_ZERO_CASES:
        ref = O.affine(img, cw, ch, interpolation="nearest", **kw)
        same(gpu.r.affine_transform(img, cw, ch, interpolation="nearest", **kw), ref, f"{kw}")
        if "rotation_x" in kw:
            assert (ref[ch // 2] == 0).all(), kw
        else:
            assert (ref[:, cw // 2] == 0).all(), kw
