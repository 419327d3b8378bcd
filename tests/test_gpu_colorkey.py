"""Removal by colour on the device (k_colorkey.hip) against the CPU model (tests/colorkey_model.py).  Everything is in the EXACT class: every comparison is
np.array_equal — device against model, host-buffer form against `_dev` form against in place.  tests/test_colorkey_model_host.py asserts that the cases hold
what they are meant to hold (unchanged, zeroed and partial pixels; geodesic rings; the small-removal skip), so nothing here passes vacuously.  The launch counts
follow from the structure (one ring launch per 32 levels), not from a clock."""
import ctypes as C

import numpy as np
import pytest

from . import colorkey_cases as CC
from . import colorkey_model as M
from .dev_buffers import SENTINEL, DevBuffers, sentinel_like

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -5


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def status_of(fn):
    from paintfe_amd import PfxError
    try:
        fn()
    except PfxError as e:
        return e.status
    return OK


# ---- colour to alpha -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("name", sorted(CC.CTA_SETTINGS))
def test_colour_to_alpha_equals_the_model(gpu, name, masked):
    for w, h in CC.CTA_SIZES:
        img, mask, want, _ = CC.cta_expected(name, w, h, masked)
        got = gpu.color_to_alpha(img, mask=mask, out=sentinel_like(img), **CC.CTA_SETTINGS[name])
        assert np.array_equal(got, want), (w, h, int((got != want).any(axis=2).sum()))


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_colour_to_alpha_forms_agree(gpu, masked):
    for name, (w, h) in [("default", (130, 70)), ("target-no-zero-channel", (257, 3))]:
        img, mask, want, _ = CC.cta_expected(name, w, h, masked)
        s = CC.CTA_SETTINGS[name]
        m = np.zeros((h, w), np.uint8) if mask is None else mask
        with DevBuffers(gpu, img, sentinel_like(img), m) as (d_src, d_dst, d_mask):
            gpu.color_to_alpha_dev(d_src, d_dst, w, h, mask_ptr=d_mask if masked else 0, **s)
            assert np.array_equal(gpu.dev_download(d_dst, img.shape), want)
            assert np.array_equal(gpu.dev_download(d_src, img.shape), img) and np.array_equal(gpu.dev_download(d_mask, m.shape), m)     # only read
            gpu.color_to_alpha_dev(d_src, d_src, w, h, mask_ptr=d_mask if masked else 0, **s)                                          # in place
            assert np.array_equal(gpu.dev_download(d_src, img.shape), want)
        inplace = img.copy()
        assert gpu.color_to_alpha(inplace, mask=mask, out=inplace, **s) is inplace and np.array_equal(inplace, want)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_colour_to_alpha_byte_path_at_a_pointer_offset(gpu, masked):
    """RGBA8 pointers 4 bytes into their allocations and a pixel count that is no multiple of 4: neither the 16-byte loads nor a whole number of groups"""
    w, h = 257, 3
    assert (w * h) % 4 != 0
    img, mask, want, _ = CC.cta_expected("default", w, h, masked)
    m = np.zeros((h, w), np.uint8) if mask is None else mask
    pad = lambda a, n: np.concatenate([np.full(n, SENTINEL, np.uint8), a.ravel(), np.full(16, SENTINEL, np.uint8)])
    with DevBuffers(gpu, pad(img, 4), pad(sentinel_like(img), 4), pad(m, 1)) as (d_src, d_dst, d_mask):
        gpu.color_to_alpha_dev(d_src + 4, d_dst + 4, w, h, mask_ptr=d_mask + 1 if masked else 0, **CC.CTA_SETTINGS["default"])
        got = gpu.dev_download(d_dst, (img.size + 20,))
        assert np.array_equal(got[4:-16].reshape(img.shape), want)
        assert (got[:4] == SENTINEL).all() and (got[-16:] == SENTINEL).all()       # nothing beside the image is written


# ---- the Color Remover ---------------------------------------------------------------------------------------------------------------------------------------------
def check_structure(gpu, w, h, smoothness, contiguous):
    assert gpu.colorkey_last(1) == CC.ring_launches(smoothness)
    if contiguous:
        assert 1 <= gpu.colorkey_last(0) < w * h + 2          # the flood's own bound (tests/test_gpu_flood.py)
        assert gpu.colorkey_last(4) == 1 + 1 + gpu.colorkey_last(0) + max(CC.ring_launches(smoothness), 1)     # map, seed, passes, then the rings or step 3 alone
    else:
        assert gpu.colorkey_last(0) == 0
        assert gpu.colorkey_last(4) == 1 + max(CC.ring_launches(smoothness), 1)


def test_kernel_shape_is_what_the_cases_assume(gpu):
    assert gpu.colorkey_last(2) == CC.TILE and gpu.colorkey_last(3) == CC.CHUNK
    assert gpu.colorkey_last(5) == -1


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "global"])
@pytest.mark.parametrize("smoothness", CC.SMOOTHNESS)
def test_remover_equals_the_model(gpu, smoothness, contiguous):
    for case in CC.REMOVER_CASES:
        for tol in CC.TOLERANCES:
            for with_sel in ((False, True) if (case[1], case[2]) == (130, 70) and tol == 15.0 else (False,)):
                img, seed, sel, want, _ = CC.remover_expected(case[0], tol, smoothness, contiguous, with_sel)
                got = gpu.color_removal(img, seed, tol, smoothness, contiguous, sel, out=sentinel_like(img))
                assert np.array_equal(got, want), (case[0], tol, with_sel, int((got != want).any(axis=2).sum()))
                if not M.is_noop(img, seed, sel):
                    check_structure(gpu, case[1], case[2], smoothness, contiguous)


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "global"])
@pytest.mark.parametrize("smoothness", CC.WALL_SMOOTHNESS)
def test_walled_case_equals_the_model(gpu, smoothness, contiguous):
    img, sel, want, _ = CC.walled_expected(smoothness, contiguous)
    got = gpu.color_removal(img, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, sel, out=sentinel_like(img))
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())
    check_structure(gpu, CC.WALL_W, CC.WALL_H, smoothness, contiguous)


def test_negative_tolerance_acts_like_its_magnitude(gpu):
    img, sel, want, _ = CC.walled_expected(20, True)
    assert np.array_equal(gpu.color_removal(img, CC.WALL_SEED, -CC.WALL_TOLERANCE, 20, True, sel), want)


def test_the_references_noops_copy_src(gpu):
    img, sel = CC.walled_image().copy(), CC.walled_selection().copy()
    clear_seed = (12, 31)                                  # inside the alpha-0 pocket
    assert img[clear_seed[1], clear_seed[0], 3] == 0
    got = gpu.color_removal(img, clear_seed, 10.0, 5, True, sel, out=sentinel_like(img))
    assert np.array_equal(got, img)
    unselected_seed = (42, 10)                             # on the wall
    assert sel[unselected_seed[1], unselected_seed[0]] == 0 and img[unselected_seed[1], unselected_seed[0], 3] != 0
    for contiguous in (True, False):
        got = gpu.color_removal(img, unselected_seed, 10.0, 5, contiguous, sel, out=sentinel_like(img))
        assert np.array_equal(got, img)
    with DevBuffers(gpu, img, sentinel_like(img), sel) as (d_src, d_dst, d_sel):
        gpu.color_removal_dev(d_src, d_dst, CC.WALL_W, CC.WALL_H, unselected_seed, 10.0, 5, True, d_sel)
        assert np.array_equal(gpu.dev_download(d_dst, img.shape), img)
        gpu.color_removal_dev(d_src, d_src, CC.WALL_W, CC.WALL_H, clear_seed, 10.0, 5, True, d_sel)       # in place: nothing to copy
        assert np.array_equal(gpu.dev_download(d_src, img.shape), img)


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "global"])
@pytest.mark.parametrize("smoothness", [0, 20, 33])
def test_remover_forms_agree(gpu, smoothness, contiguous):
    img, sel, want, _ = CC.walled_expected(smoothness, contiguous)
    w, h = CC.WALL_W, CC.WALL_H
    with DevBuffers(gpu, img, sentinel_like(img), sel) as (d_src, d_dst, d_sel):
        gpu.color_removal_dev(d_src, d_dst, w, h, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, d_sel)
        assert np.array_equal(gpu.dev_download(d_dst, img.shape), want)                                   # the sentinel is gone: every pixel is written
        assert np.array_equal(gpu.dev_download(d_src, img.shape), img) and np.array_equal(gpu.dev_download(d_sel, sel.shape), sel)     # only read
        check_structure(gpu, w, h, smoothness, contiguous)
        gpu.color_removal_dev(d_src, d_src, w, h, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, d_sel)      # in place
        assert np.array_equal(gpu.dev_download(d_src, img.shape), want)
    inplace = img.copy()
    assert gpu.color_removal(inplace, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, sel, out=inplace) is inplace and np.array_equal(inplace, want)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def raw_call(gpu, name, src_ptr, dst_ptr, w, h, params, mask_ptr):
    fn = getattr(gpu._lib, name)
    return fn(gpu.handle, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), None if params is None else C.byref(params), C.c_void_p(mask_ptr or None))


def test_refusals_leave_the_outputs_alone(gpu):
    from paintfe_amd import _lib
    from paintfe_amd.renderer import _color_removal, _color_to_alpha
    img, sel, want, _ = CC.walled_expected(20, True)
    w, h, px = CC.WALL_W, CC.WALL_H, CC.WALL_W * CC.WALL_H
    # host-buffer form through the wrappers
    for kwargs, status in [(dict(seed=(w, 0)), ERR_INVALID), (dict(seed=(0, h)), ERR_INVALID), (dict(tolerance=float("nan")), ERR_INVALID),
                           (dict(tolerance=float("inf")), ERR_INVALID), (dict(contiguous=2), ERR_INVALID), (dict(smoothness=1025), ERR_UNSUPPORTED)]:
        a = dict(seed=CC.WALL_SEED, tolerance=CC.WALL_TOLERANCE, smoothness=20, contiguous=True)
        a.update(kwargs)
        out = sentinel_like(img)
        assert status_of(lambda: gpu.color_removal(img, selection=sel, out=out, **a)) == status, kwargs
        assert (out == SENTINEL).all(), kwargs
    for bad in (float("nan"), float("-inf")):
        for key in ("tolerance", "softness", "strength", "spill_suppression", "alpha_floor", "alpha_ceiling", "protect_luminance"):
            out = sentinel_like(img)
            assert status_of(lambda: gpu.color_to_alpha(img, (255, 0, 0), out=out, **{key: bad})) == ERR_INVALID, key
            assert (out == SENTINEL).all()
    # a host dst that overlaps src other than in place
    both = np.full(px * 4 + 64, SENTINEL, np.uint8)
    src_view, dst_view = both[:px * 4].reshape(h, w, 4), both[64:].reshape(h, w, 4)
    src_view[...] = img
    before = both.copy()
    assert status_of(lambda: gpu.color_removal(src_view, CC.WALL_SEED, CC.WALL_TOLERANCE, 20, True, sel, out=dst_view)) == ERR_INVALID
    assert status_of(lambda: gpu.color_to_alpha(src_view, (250, 10, 10), out=dst_view)) == ERR_INVALID
    assert np.array_equal(both, before)
    # device form: one allocation holds src | dst | selection so that overlaps and odd addresses can be made from it
    req, cta = _color_removal(CC.WALL_SEED, CC.WALL_TOLERANCE, 20, True), _color_to_alpha((250, 10, 10), 18.0, 35.0, 1.0, 0.35, 0.0, 1.0, 0.15)
    block = np.concatenate([img.ravel(), sentinel_like(img).ravel(), sel.ravel(), np.full(64, SENTINEL, np.uint8)])
    with DevBuffers(gpu, block) as (base,):
        d_src, d_dst, d_sel = base, base + px * 4, base + px * 8
        for name, params in (("pfx_color_removal_dev", req), ("pfx_color_to_alpha_dev", cta)):
            assert raw_call(gpu, name, d_src, d_dst, w, h, None, d_sel) == ERR_INVALID                   # NULL struct
            assert raw_call(gpu, name, d_src, d_src + 8, w, h, params, d_sel) == ERR_INVALID              # dst overlaps src, not in place
            assert raw_call(gpu, name, d_src, d_sel - 4 * px + 16, w, h, params, d_sel) == ERR_INVALID    # dst ends inside the selection
            assert raw_call(gpu, name, d_src, d_dst, w, h, params, d_dst + 4) == ERR_INVALID              # the selection inside dst
            assert raw_call(gpu, name, d_src + 2, d_dst, w - 1, h, params, d_sel) == ERR_INVALID          # a misaligned RGBA8 pointer
            assert raw_call(gpu, name, d_src, d_dst + 1, w - 1, h, params, d_sel) == ERR_INVALID
        host_out = sentinel_like(img)
        assert raw_call(gpu, "pfx_color_removal", img.ctypes.data, host_out.ctypes.data, w, h, None, 0) == ERR_INVALID
        assert (host_out == SENTINEL).all()
        gpu.synchronize()
        assert np.array_equal(gpu.dev_download(base, block.shape), block)
        # afterwards the context still works
        assert raw_call(gpu, "pfx_color_removal_dev", d_src, d_dst, w, h, req, d_sel) == OK
        assert np.array_equal(gpu.dev_download(d_dst, img.shape), want)
    assert np.array_equal(gpu.color_removal(img, CC.WALL_SEED, CC.WALL_TOLERANCE, 20, True, sel), want)
