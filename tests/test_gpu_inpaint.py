"""Content-aware fill on the device (k_inpaint.hip) against the reference's goldens and the CPU model (GPU).  Everything is in the EXACT class: every
comparison is np.array_equal — device against golden, device against model, host-buffer form against `_dev` form."""
import ctypes as C

import numpy as np
import pytest

from . import inpaint_cases as IC
from . import inpaint_model as M
from .dev_buffers import DevBuffers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


@pytest.fixture(scope="module")
def goldens():
    return IC.load_goldens()


def instant_dev(gpu, src, mask, out, dabs):
    h, w = mask.shape
    with DevBuffers(gpu, src, mask, out) as (d_src, d_mask, d_out):
        gpu.inpaint_instant_dev(d_src, d_mask, d_out, w, h, dabs)
        return gpu.dev_download(d_out, out.shape)


def patchmatch_dev(gpu, src, mask, ps, iters, in_place):
    h, w = mask.shape
    with DevBuffers(gpu, src, mask, np.full_like(src, 0xA5)) as (d_src, d_mask, d_dst):
        gpu.inpaint_patchmatch_dev(d_src, d_mask, d_src if in_place else d_dst, w, h, ps, iters)
        if not in_place:
            assert np.array_equal(gpu.dev_download(d_src, src.shape), src)      # src is only read
        return gpu.dev_download(d_src if in_place else d_dst, src.shape)


def test_instant_golden(gpu, goldens):
    src, mask, out, dabs = IC.golden_instant()
    want = goldens["inpaint/instant_brush_center"]
    assert np.array_equal(gpu.inpaint_instant(src, mask, out, dabs), want)
    assert np.array_equal(instant_dev(gpu, src, mask, out, dabs), want)


def test_patchmatch_golden(gpu, goldens):
    src, mask, ps, iters = IC.golden_patchmatch()
    want = goldens["inpaint/patchmatch_checkerboard"]
    assert np.array_equal(gpu.inpaint_patchmatch(src, mask, ps, iters), want)
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, False), want)
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, True), want)


@pytest.mark.parametrize("case", IC.instant_cases(), ids=lambda c: c[0])
def test_instant_sweep_matches_the_model(gpu, case):
    name, src, mask, out, dabs, expect = case
    want, changed = M.instant_list(src, mask, out, dabs)
    assert changed == 0 if expect == "nothing" else changed >= 20
    got = gpu.inpaint_instant(src, mask, out, dabs)
    assert np.array_equal(got, want), f"{name}: {int((got != want).any(-1).sum())} px differ from the model"
    assert np.array_equal(instant_dev(gpu, src, mask, out, dabs), got)


def test_a_dab_list_equals_single_dab_calls_in_order(gpu):
    name, src, mask, out, dabs, _ = next(c for c in IC.instant_cases() if c[0] == "five_overlapping_dabs")
    one_call = gpu.inpaint_instant(src, mask, out, dabs)
    cur = out
    for d in dabs:
        cur = gpu.inpaint_instant(src, mask, cur, [d])
    assert np.array_equal(one_call, cur)
    assert not np.array_equal(one_call, gpu.inpaint_instant(src, mask, out, dabs[::-1]))      # the order matters on this input
    assert np.array_equal(gpu.inpaint_instant(src, mask, out, []), out)


@pytest.mark.parametrize("spec", IC.PATCHMATCH_SWEEP, ids=IC.patchmatch_id)
def test_patchmatch_sweep_matches_the_model(gpu, spec):
    src, mask, ps, iters = IC.patchmatch_case(spec)
    want, k = M.patchmatch(src, mask, ps, iters)
    print(IC.patchmatch_id(spec), k)
    got = gpu.inpaint_patchmatch(src, mask, ps, iters)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} px differ from the model"
    assert int(gpu._lib.pfx_int_inpaint_last(gpu._h, C.c_int(0))) == k["peels"]
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, False), got)
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, True), got)


def test_a_chain_of_65_overlapping_dabs_equals_single_dab_calls_in_order(gpu):
    name, src, mask, out, dabs, _ = next(c for c in IC.instant_cases() if c[0] == IC.CHAIN_65)
    one_call = gpu.inpaint_instant(src, mask, out, dabs)
    cur = out
    for d in dabs:
        cur = gpu.inpaint_instant(src, mask, cur, [d])
    assert np.array_equal(one_call, cur)
    assert not np.array_equal(one_call, gpu.inpaint_instant(src, mask, out, dabs[::-1]))      # the order matters on this input


def _peels(gpu):
    return int(gpu._lib.pfx_int_inpaint_last(gpu._h, C.c_int(0)))


@pytest.mark.parametrize("spec", IC.PATCHMATCH_EDGES, ids=IC.patchmatch_id)
def test_patchmatch_edges_match_the_model(gpu, spec):
    """one case per block-sized loop of k_inpaint.hip (tests/inpaint_cases.py says which; tests/test_inpaint_model_host.py holds each to its condition)"""
    src, mask, ps, iters = IC.patchmatch_case(spec)
    want, k, _ = IC.patchmatch_expected(spec)
    print(IC.patchmatch_id(spec), k)
    got = gpu.inpaint_patchmatch(src, mask, ps, iters)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} px differ from the model"
    assert _peels(gpu) == k["peels"]
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, False), got)
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, True), got)


def test_one_context_through_changing_geometry():
    """a huge box and source list, then a small canvas, then a long boundary list, on ONE context: the working block has grown and every offset inside it moves
    from call to call, so anything read from it before it is written would show.  Each result equals a fresh context's and the model's."""
    from paintfe_amd import GpuRenderer
    one = GpuRenderer(0)
    try:
        for spec in IC.GEOMETRY_SEQUENCE:
            src, mask, ps, iters = IC.patchmatch_case(spec)
            want, k, _ = IC.patchmatch_expected(spec)
            got = one.inpaint_patchmatch(src, mask, ps, iters)
            assert np.array_equal(got, want), (IC.patchmatch_id(spec), int((got != want).any(-1).sum()))
            assert _peels(one) == k["peels"]
            fresh = GpuRenderer(0)
            try:
                assert np.array_equal(fresh.inpaint_patchmatch(src, mask, ps, iters), got), IC.patchmatch_id(spec)
            finally:
                fresh.close()
    finally:
        one.close()


@pytest.mark.parametrize("fill", [0, 255], ids=["empty_mask", "all_hole"])
def test_patchmatch_without_a_hole_or_without_a_source_copies_src(gpu, fill):
    src, _, ps, iters = IC.patchmatch_case(IC.PATCHMATCH_SWEEP[0])
    mask = np.full(src.shape[:2], fill, np.uint8)
    assert np.array_equal(gpu.inpaint_patchmatch(src, mask, ps, iters), src)
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, False), src)
    assert np.array_equal(patchmatch_dev(gpu, src, mask, ps, iters, True), src)
    assert int(gpu._lib.pfx_int_inpaint_last(gpu._h, C.c_int(0))) == 0


def _instant_status(gpu, src, mask, out, dab_rows, w, h):
    from paintfe_amd import _lib
    arr = (_lib.InpaintDab * len(dab_rows))(*[_lib.InpaintDab(*r) for r in dab_rows])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return gpu._lib.pfx_inpaint_instant(gpu._h, p(src), p(mask), p(out), C.c_uint32(w), C.c_uint32(h), arr, C.c_uint32(len(dab_rows)))


def test_bad_dabs_and_overlapping_out_are_refused_and_leave_the_output_alone(gpu):
    W, H = IC.SWEEP_W, IC.SWEEP_H
    src = np.full((H, W, 4), 0xA5, np.uint8)
    mask = np.full((H, W), 255, np.uint8)
    out = np.full((H, W, 4), 0xA5, np.uint8)
    good = (60.0, 40.0, 12.0, 20.0, 0.5)
    for field in range(5):
        for bad in (float("nan"), float("inf"), float("-inf")):
            row = list(good)
            row[field] = bad
            assert _instant_status(gpu, src, mask, out, [good, tuple(row)], W, H) == -1, (field, bad)
    assert (out == 0xA5).all()
    assert _instant_status(gpu, src, mask, src, [good], W, H) == -1                         # out == src
    both = np.full(H * W * 4 + H * W, 0xA5, np.uint8)
    assert _instant_status(gpu, src, both[H * W * 4 - 16:], both[:H * W * 4], [good], W, H) == -1   # out overlaps the mask
    assert (src == 0xA5).all() and (both == 0xA5).all()
    with DevBuffers(gpu, src, mask) as (d_src, d_mask):       # the device forms
        from paintfe_amd import PfxError
        with pytest.raises(PfxError):
            gpu.inpaint_instant_dev(d_src, d_mask, d_src, W, H, [good])
        with pytest.raises(PfxError):
            gpu.inpaint_patchmatch_dev(d_src, d_mask, d_mask, W, H, 5, 3)
        with pytest.raises(PfxError):
            gpu.inpaint_patchmatch_dev(d_src, d_mask, d_src, W, H, 13, 3)
        assert (gpu.dev_download(d_src, src.shape) == 0xA5).all() and (gpu.dev_download(d_mask, mask.shape) == 255).all()
