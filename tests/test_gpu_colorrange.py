"""The histogram, per-band Hue/Saturation and colour range on the device (k_colorrange.hip) against the CPU model (tests/colorrange_model.py), through the
Python surface of the C ABI.  The histogram (integer sums) and the per-band dialog (EXACT class) are held with np.array_equal; the colour range is equal to the
model off the pixels the model marks — where one f32 ulp of the power moves the byte — and within 1 on them.  tests/test_colorrange_model_host.py holds the
model to a scalar transcription of the reference and asserts that the cases of tests/colorrange_cases.py contain what they are here for."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import colorrange_cases as CC
from . import colorrange_model as CM
from .dev_buffers import SENTINEL, Dev, sentinel_like

pytestmark = pytest.mark.gpu

OK, ERR_INVALID = 0, -1
LANES, QUAD = 256, 4   # lanes of a workgroup; pixels of a lane's step on the 16-byte path


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


def status_of(fn):
    from paintfe_amd import PfxError
    try:
        fn()
    except PfxError as e:
        return e.status
    return OK


@functools.lru_cache(maxsize=None)
def band_sources():
    return CC.band_inputs()


@functools.lru_cache(maxsize=None)
def range_sources():
    return CC.range_inputs()


def tiled(img, w, h):
    """a w x h image of repeats of img"""
    ih, iw = img.shape[:2]
    return np.ascontiguousarray(np.tile(img, (-(-h // ih), -(-w // iw)) + (1,) * (img.ndim - 2))[:h, :w])


# ---- histogram --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_histogram_equals_the_model_at_the_small_sizes(gpu, masked):
    for (w, h) in CC.SMALL_SHAPES:
        img = CC.noise(w, h, 21)
        img[0, :5, 3] = 0
        mask = CC.selection(w, h, 22) if masked else None
        want = CM.histogram(img, mask)
        assert np.array_equal(gpu.histogram(img, mask=mask), want), (w, h)
        with Dev(gpu) as d:
            p_img, p_mask = d.put(img), d.put(mask) if masked else 0
            assert np.array_equal(gpu.histogram_dev(p_img, w, h, mask_ptr=p_mask), want), (w, h)
            assert np.array_equal(d.get(p_img, img.shape), img)     # only read


def test_histogram_beyond_one_full_grid_noise_and_flat(gpu):
    cap = gpu.colorrange_info(0)      # PFXK_HIST_MAX_BLOCKS: the launcher never starts more workgroups, each lane then walks on by a grid's stride
    w, h = 1031, 1021
    assert 0 < cap and cap * LANES * QUAD < w * h and (w * h) % 4 != 0      # more than one pass of the grid on the 16-byte path, and a tail behind it
    img = tiled(CC.noise(256, 256, 23), w, h)
    mask = tiled(CC.selection(256, 256, 24), w, h)
    for m in (None, mask):
        assert np.array_equal(gpu.histogram(img, mask=m), CM.histogram(img, m)), m is None
    with Dev(gpu) as d:      # off a 16-byte address a lane takes one pixel per step: a grid holds cap * LANES pixels, four passes and a tail here
        assert np.array_equal(gpu.histogram_dev(d.put(img, offset=4), w, h, mask_ptr=d.put(mask, offset=1)), CM.histogram(img, mask))
    flat = np.empty((h, w, 4), np.uint8)
    flat[...] = (200, 100, 50, 255)      # every lane on the same four bins
    got = gpu.histogram(flat)
    lum = int(CM.luminance_bin(flat[:1, :1])[0][0, 0])
    want = np.zeros((4, 256), np.uint32)
    want[0, 200] = want[1, 100] = want[2, 50] = want[3, lum] = w * h
    assert np.array_equal(got, want) and np.array_equal(want, CM.histogram(flat))


def test_histogram_of_all_colours_settles_every_luminance_rounding(gpu):
    cube = CC.all_colours()
    got = gpu.histogram(cube)
    assert np.array_equal(got[:3], np.full((3, 256), 1 << 16, np.uint32))
    assert np.array_equal(got, CM.histogram(cube))


def test_histogram_of_nothing_is_zero(gpu):
    img = CC.noise(67, 129, 25)
    assert not gpu.histogram(img, mask=np.zeros((129, 67), np.uint8)).any()
    clear = img.copy()
    clear[..., 3] = 0
    assert not gpu.histogram(clear).any() and not gpu.histogram(clear, mask=CC.selection(67, 129, 26)).any()


def test_histogram_pointer_offsets(gpu):
    w, h = 67, 129
    assert (w * h) % 4 != 0
    img, mask = CC.noise(w, h, 27), CC.selection(w, h, 28)
    with Dev(gpu) as d:
        aligned_img, off_img, aligned_mask, off_mask = d.put(img), d.put(img, offset=4), d.put(mask), d.put(mask, offset=1)
        for p_img in (aligned_img, off_img):
            assert np.array_equal(gpu.histogram_dev(p_img, w, h), CM.histogram(img))
            for p_mask in (aligned_mask, off_mask):
                assert np.array_equal(gpu.histogram_dev(p_img, w, h, mask_ptr=p_mask), CM.histogram(img, mask)), (p_img % 16, p_mask % 4)
        assert np.array_equal(d.get(off_img, img.shape), img) and np.array_equal(d.get(off_mask, mask.shape), mask)


# ---- per-band Hue/Saturation ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.BAND_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["lattice", "noise", "knee"])
def test_hsl_bands_equals_the_model(gpu, name, shape):
    w, h = shape
    img = CC.band_image(band_sources()[name], w, h)
    mask = CC.selection(w, h, 31)
    for set_name, (gh, gs, gl, bands) in CC.BAND_SETS.items():
        for m in (None, mask):
            for sparse in (CM.DENSE, CM.FROM_FLAT):
                want = CM.hsl_bands(img, gh, gs, gl, bands, mask=m, sparse=sparse)
                got = gpu.hsl_bands(img, gh, gs, gl, bands, mask=m, sparse=sparse, out=sentinel_like(img))
                assert np.array_equal(got, want), (set_name, m is None, sparse, int((got != want).any(axis=2).sum()))
    if h > 64:   # the zeroing is visible: the transparent chunk's colours survive the dense mode only
        dense = gpu.hsl_bands(img, *CC.BAND_SETS["six"][:3], CC.BAND_SETS["six"][3], sparse=CM.DENSE)
        flat = gpu.hsl_bands(img, *CC.BAND_SETS["six"][:3], CC.BAND_SETS["six"][3], sparse=CM.FROM_FLAT)
        assert dense[64:128, 0:64, :3].any() and not flat[64:128, 0:64].any()


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_hsl_bands_forms_agree_and_inputs_are_only_read(gpu, masked):
    gh, gs, gl, bands = CC.BAND_SETS["six"]
    for (w, h) in CC.BAND_SHAPES:
        img = CC.band_image(band_sources()["noise"], w, h)
        mask = CC.selection(w, h, 32)
        for sparse in (CM.DENSE, CM.FROM_FLAT, CM.IN_PLACE):
            want = CM.hsl_bands(img, gh, gs, gl, bands, mask=mask if masked else None, sparse=sparse)
            with Dev(gpu) as d:
                p_src, p_dst, p_mask = d.put(img), d.sentinel(img.shape), d.put(mask)
                gpu.hsl_bands_dev(p_src, p_dst, w, h, gh, gs, gl, bands, mask_ptr=p_mask if masked else 0, sparse=sparse)
                assert np.array_equal(d.get(p_dst, img.shape), want), (w, h, sparse)
                assert np.array_equal(d.get(p_src, img.shape), img) and np.array_equal(d.get(p_mask, mask.shape), mask)     # only read
                gpu.hsl_bands_dev(p_src, p_src, w, h, gh, gs, gl, bands, mask_ptr=p_mask if masked else 0, sparse=sparse)   # in place
                assert np.array_equal(d.get(p_src, img.shape), want), (w, h, sparse)
            inplace = img.copy()
            assert gpu.hsl_bands(inplace, gh, gs, gl, bands, mask=mask if masked else None, sparse=sparse, out=inplace) is inplace and np.array_equal(inplace, want)


# ---- colour range -----------------------------------------------------------------------------------------------------------------------------------------------------
def check_range(got, want, ambiguous, what):
    """equal off the marked pixels; a marked byte moves by one before the combine, and none of the four rules makes more of it"""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert not d[~ambiguous].any() and d.max(initial=0) <= 1, (what, int((d[~ambiguous] > 0).sum()), int(d.max(initial=0)))


@pytest.mark.parametrize("name", ["noise", "lattice"])
def test_color_range_equals_the_model_on_the_nine_sets(gpu, name):
    img = range_sources()[name]
    for s in CC.RANGE_SETS:
        want, amb = CM.color_range(img, *s)
        for fill in (SENTINEL, SENTINEL ^ 0xFF):      # two fills: a byte left unwritten differs from the model under at least one of them
            got = gpu.select_color_range(img, *s, out=np.full(img.shape[:2], fill, np.uint8))
            d = np.abs(got.astype(np.int16) - want.astype(np.int16))
            assert not d[~amb].any() and d.max() <= 1, (s, fill, int((d[~amb] > 0).sum()), int(d.max()))


def test_color_range_combine_modes_sizes_and_in_place(gpu):
    source = range_sources()["noise"]
    for (w, h) in CC.SMALL_SHAPES:
        img, base = CC.fit(source, w, h), CC.grey_base(w, h)
        for s in (CC.RANGE_SETS[1], CC.RANGE_SETS[3]):
            for mode in CC.COMBINE:
                want, amb = CM.color_range(img, *s, combine=mode, base=base)
                got = gpu.select_color_range(img, *s, combine=mode, base=base, out=np.full((h, w), SENTINEL, np.uint8))
                check_range(got, want, amb, (w, h, s, mode))
                none, _ = CM.color_range(img, *s, combine=mode, base=None)
                check_range(gpu.select_color_range(img, *s, combine=mode, out=np.full((h, w), SENTINEL, np.uint8)), none, amb, (w, h, s, mode, "NULL base"))
                inplace = base.copy()
                assert gpu.select_color_range(img, *s, combine=mode, base=inplace, out=inplace) is inplace
                check_range(inplace, want, amb, (w, h, s, mode, "in place"))
                with Dev(gpu) as d:
                    p_img, p_base, p_out = d.put(img), d.put(base), d.sentinel((h, w))
                    gpu.select_color_range_dev(p_img, w, h, *s, p_out, combine=mode, base_ptr=p_base)
                    check_range(d.get(p_out, (h, w)), want, amb, (w, h, s, mode, "dev"))
                    assert np.array_equal(d.get(p_img, img.shape), img) and np.array_equal(d.get(p_base, base.shape), base)     # only read
                    gpu.select_color_range_dev(p_img, w, h, *s, p_base, combine=mode, base_ptr=p_base)                             # in place
                    check_range(d.get(p_base, (h, w)), want, amb, (w, h, s, mode, "dev in place"))


def test_color_range_pointer_offsets_and_beyond_one_grid(gpu):
    s = CC.RANGE_SETS[0]
    # k_tools.h: stream_blocks caps a streaming launch at 8192 workgroups; off a 16-byte source a lane takes one pixel per step: 8192 * 256 pixels per pass
    cap_blocks = 8192
    small = ((4, 0, 0), (0, 1, 0), (0, 0, 1), (4, 1, 3), (0, 0, 0))
    for (w, h), offsets in (((67, 129), small), ((1031, 2039), ((4, 1, 3),))):   # the large image: the byte path alone, once
        assert (w * h) % 4 != 0
        img = tiled(range_sources()["noise"], w, h)
        base = tiled(CC.grey_base(256, 256), w, h)
        want, amb = CM.color_range(img, *s, combine="add", base=base)
        with Dev(gpu) as d:
            for off_img, off_base, off_out in offsets:
                p_img, p_base, p_out = d.put(img, offset=off_img), d.put(base, offset=off_base), d.sentinel((h, w), offset=off_out)
                gpu.select_color_range_dev(p_img, w, h, *s, p_out, combine="add", base_ptr=p_base)
                check_range(d.get(p_out, (h, w)), want, amb, (w, h, off_img, off_base, off_out))
    assert 1031 * 2039 > cap_blocks * LANES


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    w, h = 67, 5
    img, base = CC.noise(w, h, 41), CC.grey_base(w, h)
    nan, inf = float("nan"), float("inf")
    good = (30.0, 20.0, 0.1, 0.5)
    with Dev(gpu) as d:
        p_img, p_base, p_out, p_dst = d.put(img), d.put(base), d.sentinel((h, w)), d.sentinel(img.shape)
        bad_ranges = [tuple(v if i != k else b for i, v in enumerate(good)) for k in range(4) for b in (nan, inf, -inf)] + [(-0.5,) + good[1:], (360.5,) + good[1:]]
        for s in bad_ranges:
            assert status_of(lambda: gpu.select_color_range_dev(p_img, w, h, *s, p_out, combine="add", base_ptr=p_base)) == ERR_INVALID, s
            out = sentinel_like(base)
            assert status_of(lambda: gpu.select_color_range(img, *s, combine="add", base=base, out=out)) == ERR_INVALID and (out == SENTINEL).all(), s
        for mode in (4, 255):
            assert status_of(lambda: gpu.select_color_range_dev(p_img, w, h, *good, p_out, combine=mode)) == ERR_INVALID
            assert status_of(lambda: gpu.select_color_range_dev(p_img, w, h, *good, p_out, combine=mode, base_ptr=p_base)) == ERR_INVALID
            out = sentinel_like(base)
            assert status_of(lambda: gpu.select_color_range(img, *good, combine=mode, base=base, out=out)) == ERR_INVALID and (out == SENTINEL).all(), mode
        assert (d.get(p_out, (h, w)) == SENTINEL).all()      # none of the refused `_dev` calls above launched anything
        p_ok = d.sentinel((h, w))                             # the slider's ends are accepted: into a buffer of their own
        for edge in (0.0, 360.0):
            assert status_of(lambda: gpu.select_color_range_dev(p_img, w, h, edge, *good[1:], p_ok)) == OK
            assert np.array_equal(d.get(p_ok, (h, w)), CM.color_range(img, edge, *good[1:])[0])
        six = [(1.0, 2.0, 3.0)] * 6
        bad_bands = [(nan, 0.0, 0.0, six), (0.0, inf, 0.0, six), (0.0, 0.0, -inf, six)] + \
                    [(0.0, 0.0, 0.0, six[:k] + [tuple(b if i == j else 1.0 for i in range(3))] + six[k + 1:]) for k in (0, 5) for j in range(3) for b in (nan, inf)]
        for (gh, gs, gl, bands) in bad_bands:
            assert status_of(lambda: gpu.hsl_bands_dev(p_img, p_dst, w, h, gh, gs, gl, bands)) == ERR_INVALID, (gh, gs, gl, bands)
            out = sentinel_like(img)
            assert status_of(lambda: gpu.hsl_bands(img, gh, gs, gl, bands, out=out)) == ERR_INVALID and (out == SENTINEL).all()
        for sparse in (-1, 3):
            assert status_of(lambda: gpu.hsl_bands_dev(p_img, p_dst, w, h, 0.0, 0.0, 0.0, six, sparse=sparse)) == ERR_INVALID
        # aliasing: in place is the one overlap that is allowed; a device image off a dword is refused
        assert status_of(lambda: gpu.hsl_bands_dev(p_img, p_img + 16, w, h, 0.0, 0.0, 0.0, six)) == ERR_INVALID
        assert status_of(lambda: gpu.hsl_bands_dev(p_img + 1, p_dst, w, h, 0.0, 0.0, 0.0, six)) == ERR_INVALID
        assert status_of(lambda: gpu.hsl_bands_dev(p_img, p_dst, w, h, 0.0, 0.0, 0.0, six, mask_ptr=p_dst + 4)) == ERR_INVALID
        assert status_of(lambda: gpu.select_color_range_dev(p_img, w, h, *good, p_base + 16, base_ptr=p_base)) == ERR_INVALID
        assert status_of(lambda: gpu.select_color_range_dev(p_img, w, h, *good, p_img + 8)) == ERR_INVALID
        assert status_of(lambda: gpu.select_color_range_dev(p_img + 2, w, h, *good, p_out)) == ERR_INVALID
        assert gpu._lib.pfx_hsl_bands_dev(gpu.handle, C.c_void_p(p_img), C.c_void_p(p_dst), C.c_uint32(w), C.c_uint32(h), C.c_float(0), C.c_float(0), C.c_float(0), None, None,
                                          C.c_int(0)) == ERR_INVALID     # bands = NULL
        assert (d.get(p_out, (h, w)) == SENTINEL).all() and (d.get(p_dst, img.shape) == SENTINEL).all()
        assert np.array_equal(d.get(p_img, img.shape), img) and np.array_equal(d.get(p_base, base.shape), base)
        hist = np.full((4, 256), 0xA5A5A5A5, np.uint32)
        lib = gpu._lib
        for (ww, hh, ptr) in ((0, h, p_img), (w, 0, p_img), (20000, 20000, p_img), (w, h, 0), (w, h, p_img + 1)):
            st = lib.pfx_histogram_dev(gpu.handle, C.c_void_p(ptr or None), C.c_uint32(ww), C.c_uint32(hh), None, hist.ctypes.data_as(C.c_void_p))
            assert st == ERR_INVALID and (hist == 0xA5A5A5A5).all(), (ww, hh, ptr)
        assert lib.pfx_histogram_dev(gpu.handle, C.c_void_p(p_img), C.c_uint32(w), C.c_uint32(h), None, None) == ERR_INVALID
