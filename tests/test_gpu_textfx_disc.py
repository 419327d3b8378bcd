"""The text styles' disc kernel alone (k_textfx.hip: disc_kernel, through the seam pfx_int_textfx_disc_dev) against the tap-by-tap disc of
tests/textfx_disc_cases.py, on planes where every tap of the disc and every neighbour of its rim shows: every halo from 1 to 64, both tile shapes, the
maximum and the minimum.  Byte for byte; tests/test_textfx_disc_host.py shows that these inputs would not pass a disc with one tap wrong."""
import ctypes as C

import numpy as np
import pytest

from . import textfx_disc_cases as DC
from .dev_buffers import SENTINEL, DevBuffers, sentinel_like

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -5


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


@pytest.fixture(autouse=True)
def stop_after_a_device_error(gpu):
    """a HIP error behind a test ends the session: nothing more is launched on a device that has reported one"""
    yield
    from paintfe_amd import PfxError
    try:
        gpu.synchronize()
    except PfxError as e:
        pytest.exit(f"the device reported an error after this test: {e}", returncode=3)


def run_disc(gpu, plane, radius, take_min):
    """one launch on fresh planes with sentinels around them; the source must come back untouched"""
    h, w = plane.shape
    bufs = DevBuffers(gpu, plane, sentinel_like(plane))
    with bufs as (d_src, d_dst):
        gpu.textfx_disc_dev(d_src, d_dst, w, h, radius, take_min)
        got = gpu.dev_download(d_dst, plane.shape)
        assert np.array_equal(gpu.dev_download(d_src, plane.shape), plane)
        assert bufs.surroundings_intact()
    return got


def check(gpu, kind, radius, k=0, size=DC.PLANE):
    for take_min in (False, True):
        want = DC.expected(kind, radius, take_min, k, size)
        got = run_disc(gpu, DC.source(kind, radius, take_min, k, size), radius, take_min)
        assert np.array_equal(got, want), (kind, radius, "min" if take_min else "max", k, size, int((got != want).sum()))


@pytest.mark.parametrize("radius", DC.SWEEP, ids=lambda r: f"{r:g}")
def test_every_halo(gpu, radius):
    """one pixel alone in its window: the result is the disc itself, so a tap missing or a tap too many anywhere on its rim is a differing byte.  Up to a halo
    of 8 the pixel sits in turn on each side of the corners of the 64 x 32 tiles"""
    for k in range(len(DC.clear_centres(radius))):
        check(gpu, "clear", radius, k)


def test_the_sweep_reaches_every_level_and_read_count(gpu):
    """build_disc (pfx_textfx.cpp) gives a span of L columns the largest window of 4^level <= L columns, level at most 3, and ceil(L / 4^level) reads of
    it: over the sweep's row lengths that is every level and every read count from 1 to 4, with the lengths on both sides of each level's boundary"""
    from paintfe_amd import textfx_span
    lengths = set()
    for radius in DC.SWEEP:
        R = DC.reach_of(radius)
        halves = [textfx_span(radius, dy) for dy in range(-R, R + 1)]
        assert sorted(2 * half + 1 for half in halves if half >= 0) == sorted(DC.row_lengths(radius)), radius   # the library's spans are the membership's rows
        lengths |= {2 * half + 1 for half in halves if half >= 0}
    assert {3, 5, 15, 17, 63, 65} <= lengths
    words = {DC.span_word(L) for L in lengths}
    assert {level for level, _ in words} == {0, 1, 2, 3} and {reads for _, reads in words} == {1, 2, 3, 4}
    assert [DC.span_word(L)[0] for L in (3, 5, 15, 17, 63, 65)] == [0, 1, 1, 2, 2, 3]


@pytest.mark.parametrize("radius", DC.SALT_RADII)
def test_overlapping_discs(gpu, radius):
    check(gpu, "salt", radius)


@pytest.mark.parametrize("radius", DC.SEAM_RADII)
@pytest.mark.parametrize("size", DC.SEAM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_seams_and_an_image_shorter_than_the_halo(gpu, size, radius):
    check(gpu, "salt", radius, size=size)


@pytest.mark.parametrize("radius", DC.THIN_RADII)
@pytest.mark.parametrize("size", DC.THIN_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_row_one_column_one_pixel(gpu, size, radius):
    check(gpu, "noise", radius, size=size)


def test_refusals_leave_the_destination_alone(gpu):
    from paintfe_amd import _lib
    lib, ctx = _lib.load(), gpu.handle
    w, h = 40, 12
    plane = DC.noise((w, 3 * h))                                       # three planes' worth, so that a shifted pointer stays inside the allocation
    prior = sentinel_like(plane)

    def call(src, dst, cw=w, ch=h, radius=2.0, take_min=0, context=ctx):
        return lib.pfx_int_textfx_disc_dev(context, C.c_void_p(src or None), C.c_void_p(dst or None), cw, ch, radius, take_min)

    bufs = DevBuffers(gpu, plane, prior)
    with bufs as (d_src, d_dst):
        assert call(d_src, d_dst) == OK and call(d_src, d_dst, take_min=1) == OK      # the same arguments, nothing wrong: accepted
        gpu.synchronize()
        gpu.dev_upload(d_dst, prior)
        for bad in (float("nan"), float("inf"), float("-inf"), 0.0, -0.0, -1.0):
            assert call(d_src, d_dst, radius=bad) == ERR_INVALID, bad
        for bad in (64.01, 64.5, 65.0, 1000.0, 3.0e38):
            assert call(d_src, d_dst, radius=bad) == ERR_UNSUPPORTED, bad
        assert call(0, d_dst) == ERR_INVALID and call(d_src, 0) == ERR_INVALID and call(0, 0) == ERR_INVALID
        for cw, ch in ((0, h), (w, 0), (20000, 20000), (0xFFFFFFFF, 0xFFFFFFFF)):
            assert call(d_src, d_dst, cw, ch) == ERR_INVALID, (cw, ch)
        assert call(d_dst, d_dst) == ERR_INVALID                       # src is dst
        assert call(d_dst + w, d_dst) == ERR_INVALID and call(d_dst, d_dst + w) == ERR_INVALID     # they share rows
        assert call(d_src, d_dst, context=None) == ERR_INVALID
        gpu.synchronize()
        assert (gpu.dev_download(d_dst, prior.shape) == SENTINEL).all()
        assert np.array_equal(gpu.dev_download(d_src, plane.shape), plane) and bufs.surroundings_intact()
        assert call(d_src, d_dst, radius=64.0) == OK and call(d_src, d_dst, radius=0.5) == OK       # the largest and a radius below one pixel are served
        gpu.synchronize()
        assert np.array_equal(gpu.dev_download(d_dst, (h, w)), plane[:h])   # the disc of 0.5 is the pixel itself
