"""Selection masks on the device (k_select.hip) against the CPU model (tests/select_model.py).  Everything is in the EXACT class: every comparison is
np.array_equal — device against model, host-buffer form against `_dev` form.  Sources are checked unmodified, in place is checked where the ABI allows it, and
the `_dev` runs sit between guard bytes, at dword-aligned and at odd addresses (the shape kernel's vector and byte paths)."""
import numpy as np
import pytest

from . import select_cases as SC
from . import select_model as M
from .dev_buffers import SENTINEL, Dev

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
MODE_NAMES = ["replace", "add", "subtract", "intersect"]
sizes = pytest.mark.parametrize("size", SC.SIZES, ids=SC.size_id)


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def refused(status, call, *args, **kwargs):
    from paintfe_amd import PfxError
    with pytest.raises(PfxError) as e:
        call(*args, **kwargs)
    assert e.value.status == status, e.value


def test_the_sizes_straddle_the_kernels_tiles(gpu):
    assert [gpu.select_last(k) for k in range(4)] == [SC.SEG, SC.BAND, SC.VEC, M.LASSO_MAX_POINTS]
    widths, heights = {w for w, _ in SC.SIZES}, {h for _, h in SC.SIZES}
    assert min(widths) == 1 and any(w < SC.SEG for w in widths) and any(SC.SEG < w < 2 * SC.SEG for w in widths)         # one step, a step and a ragged second
    assert any(h < SC.BAND for h in heights) and any(h > 2 * SC.BAND and h % SC.BAND for h in heights) and any(h > 4 * SC.BAND for h in heights)
    assert any((w * h) % SC.VEC for w, h in SC.SIZES) and any((w * h) % SC.VEC == 0 and w % SC.VEC for w, h in SC.SIZES)  # a byte tail; dwords across row ends
    assert gpu.select_last(99) == -1


# ---- rectangle, ellipse ----------------------------------------------------------------------------------------------------------------------------------------
def shape_calls(gpu, size):
    w, h = size
    for c in SC.rect_cases(w, h):
        yield ("rect",) + c, (lambda c=c, **k: gpu.select_rect(size, *c, **k)), (lambda base, mode, c=c: M.select_rect(base, w, h, *c, mode))
    for c in SC.ellipse_cases(w, h):
        yield ("ellipse",) + c, (lambda c=c, **k: gpu.select_ellipse(size, *c, **k)), (lambda base, mode, c=c: M.select_ellipse(base, w, h, *c, mode))


@sizes
def test_shapes_equal_the_model_in_every_mode(gpu, size):
    base = SC.random_bytes(*size, seed=21)       # every byte value, not just 0 / 255
    keep = base.copy()
    for what, call, model in shape_calls(gpu, size):
        for mode in M.MODES:
            want = model(base, mode)
            assert np.array_equal(call(combine=MODE_NAMES[mode], base=base), want), (what, mode)
            assert np.array_equal(call(combine=mode, base=None), model(None, mode)), (what, mode, "NULL base")
            inplace = base.copy()
            assert call(combine=mode, base=inplace, out=inplace) is inplace and np.array_equal(inplace, want), (what, mode, "in place")
    assert np.array_equal(base, keep)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("size", [(65, 66), (259, 131), (1, 97)], ids=SC.size_id)
def test_shape_dev_forms(gpu, size, offset):
    w, h = size
    base = SC.random_bytes(w, h, seed=22)
    rect, ell = SC.rect_cases(w, h)[3], SC.ellipse_cases(w, h)[0]
    for mode in M.MODES:
        with Dev(gpu) as d:
            d_base, d_out, d_in = d.put(base, offset), d.sentinel((h, w), offset), d.put(base, offset)
            gpu.select_rect_dev(w, h, *rect, d_out, combine=mode, base_ptr=d_base)
            assert np.array_equal(d.get(d_out, (h, w)), M.select_rect(base, w, h, *rect, mode))
            gpu.select_ellipse_dev(w, h, *ell, d_out, combine=MODE_NAMES[mode], base_ptr=d_base)
            assert np.array_equal(d.get(d_out, (h, w)), M.select_ellipse(base, w, h, *ell, mode))
            assert np.array_equal(d.get(d_base, (h, w)), base)                                   # the base is only read
            gpu.select_ellipse_dev(w, h, *ell, d_in, combine=mode, base_ptr=d_in)                  # in place
            assert np.array_equal(d.get(d_in, (h, w)), M.select_ellipse(base, w, h, *ell, mode))
            gpu.select_rect_dev(w, h, *rect, d_out, combine=mode)                                  # NULL base
            assert np.array_equal(d.get(d_out, (h, w)), M.select_rect(None, w, h, *rect, mode))
            if w * h > 1:
                refused(ERR_INVALID, gpu.select_rect_dev, w, h, *rect, d_in + 1, combine=mode, base_ptr=d_in)   # an overlap that is not in place
                assert np.array_equal(d.get(d_in, (h, w)), M.select_ellipse(base, w, h, *ell, mode))
    refused(ERR_INVALID, gpu.select_rect, size, 0, 0, 1, 1, combine=4)


# ---- lasso -------------------------------------------------------------------------------------------------------------------------------------------------------
@sizes
def test_lasso_equals_the_model_in_every_mode(gpu, size):
    w, h = size
    base = SC.random_bytes(w, h, seed=23)
    for name, pts in SC.lasso_cases(w, h).items():
        raw, most = SC.lasso_raw(size, name)
        if name == "star" and size == (259, 131):
            assert 300 <= most <= M.LASSO_MAX_POINTS                 # hundreds of crossings in one row: a 512-entry sort
        for mode in M.MODES:
            assert np.array_equal(gpu.select_lasso(size, pts, combine=mode, base=base), M.combine(base, raw, mode)), (name, mode)
        assert np.array_equal(gpu.select_lasso(size, pts), raw), (name, "NULL base")
        inplace = base.copy()
        gpu.select_lasso(size, pts, combine="subtract", base=inplace, out=inplace)
        assert np.array_equal(inplace, M.combine(base, raw, M.SUBTRACT)), (name, "in place")
    assert np.array_equal(base, SC.random_bytes(w, h, seed=23))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
def test_lasso_dev_form(gpu, offset):
    size = w, h = 259, 131
    base = SC.random_bytes(w, h, seed=24)
    for name in ("star", "bow-tie", "n0"):
        pts, (raw, _) = SC.lasso_cases(w, h)[name], SC.lasso_raw(size, name)
        with Dev(gpu) as d:
            d_base, d_out = d.put(base, offset), d.sentinel((h, w), offset)
            gpu.select_lasso_dev(w, h, pts, d_out, combine="intersect", base_ptr=d_base)
            assert np.array_equal(d.get(d_out, (h, w)), M.combine(base, raw, M.INTERSECT))
            gpu.select_lasso_dev(w, h, pts, d_base, combine="add", base_ptr=d_base)              # in place
            assert np.array_equal(d.get(d_base, (h, w)), M.combine(base, raw, M.ADD))
            gpu.select_lasso_dev(w, h, pts, d_out)
            assert np.array_equal(d.get(d_out, (h, w)), raw)


def test_lasso_refusals_leave_the_output_alone(gpu):
    size = w, h = 65, 66
    tri = SC.lasso_cases(w, h)["triangle"]
    too_many = np.tile(tri, (2731, 1))[:M.LASSO_MAX_POINTS + 1]
    bad = {"8193 points": (ERR_UNSUPPORTED, too_many), "NaN": (ERR_INVALID, np.array([(1, 1), (40, float("nan")), (3, 50)], np.float32)),
           "2e9": (ERR_INVALID, np.array([(1, 1), (2e9, 30), (3, 50)], np.float32)), "inf": (ERR_INVALID, np.array([(1, 1), (9, -np.inf), (3, 50)], np.float32))}
    for what, (status, pts) in bad.items():
        out = np.full((h, w), SENTINEL, np.uint8)
        refused(status, gpu.select_lasso, size, pts, out=out)
        assert (out == SENTINEL).all(), what
        with Dev(gpu) as d:
            d_out = d.sentinel((h, w))
            refused(status, gpu.select_lasso_dev, w, h, pts, d_out)
            assert (d.get(d_out, (h, w)) == SENTINEL).all(), what
    exactly = np.tile(tri, (2731, 1))[:M.LASSO_MAX_POINTS]          # the cap itself is accepted: the triangle 2730 times over and two more vertices
    assert np.array_equal(gpu.select_lasso(size, exactly), M.lasso_raw(w, h, exactly))


# ---- expand / contract -------------------------------------------------------------------------------------------------------------------------------------------
@sizes
def test_expand_and_contract_equal_the_model(gpu, size):
    for name, mask in SC.morph_masks(*size).items():
        keep = mask.copy()
        for radius in SC.morph_radii(size):
            assert np.array_equal(gpu.selection_expand(mask, radius), SC.morph_expected(size, name, "expand", radius)), (name, radius)
            assert np.array_equal(gpu.selection_contract(mask, radius), SC.morph_expected(size, name, "contract", radius)), (name, radius)
        assert np.array_equal(mask, keep)
    if size == SC.BIG:
        full = SC.morph_masks(*size)["full"]
        assert np.array_equal(gpu.selection_contract(full, SC.BIG_RADIUS), full)               # the canvas edge does not erode


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("size", [(65, 66), (259, 131)], ids=SC.size_id)
def test_expand_and_contract_dev_forms(gpu, size, offset):
    w, h = size
    for name in ("ramp", "sparse", "sparse-holes"):
        mask = SC.morph_masks(w, h)[name]
        for radius in (0, 5, 17):
            with Dev(gpu) as d:
                d_mask, d_out = d.put(mask, offset), d.sentinel((h, w), offset)
                gpu.selection_expand_dev(d_mask, w, h, radius, d_out)
                assert np.array_equal(d.get(d_out, (h, w)), SC.morph_expected(size, name, "expand", radius))
                assert gpu.select_last(5) == (2 if radius else 0)
                gpu.selection_contract_dev(d_mask, w, h, radius, d_out)
                assert np.array_equal(d.get(d_out, (h, w)), SC.morph_expected(size, name, "contract", radius))
                assert np.array_equal(d.get(d_mask, (h, w)), mask)                               # the source is only read
                gpu.selection_contract_dev(d_mask, w, h, radius, d_mask)                         # in place
                assert np.array_equal(d.get(d_mask, (h, w)), SC.morph_expected(size, name, "contract", radius))


def test_expand_and_contract_refuse_a_radius_whose_square_overflows(gpu):
    w, h = 65, 66
    mask = SC.morph_masks(w, h)["ramp"]
    for call, call_dev in ((gpu.selection_expand, gpu.selection_expand_dev), (gpu.selection_contract, gpu.selection_contract_dev)):
        out = np.full((h, w), SENTINEL, np.uint8)
        refused(ERR_INVALID, call, mask, M.MORPH_MAX_RADIUS + 1, out=out)
        assert (out == SENTINEL).all()
        with Dev(gpu) as d:
            d_mask, d_out = d.put(mask), d.sentinel((h, w))
            refused(ERR_INVALID, call_dev, d_mask, w, h, M.MORPH_MAX_RADIUS + 1, d_out)
            refused(ERR_INVALID, call_dev, d_mask, w, h, 3, d_mask + 1)                          # an overlap that is not in place
            assert (d.get(d_out, (h, w)) == SENTINEL).all() and np.array_equal(d.get(d_mask, (h, w)), mask)
    # the largest radius runs: every pixel of a 65 x 66 image is inside the disc
    assert np.array_equal(gpu.selection_expand(mask, M.MORPH_MAX_RADIUS), np.where(mask > 127, mask, 255))
    assert np.array_equal(gpu.selection_contract(mask, M.MORPH_MAX_RADIUS), np.zeros_like(mask))


# ---- feather -----------------------------------------------------------------------------------------------------------------------------------------------------
@sizes
def test_feather_equals_the_model(gpu, size):
    for name, mask in SC.feather_masks(*size).items():
        keep = mask.copy()
        for radius in SC.feather_radii(size):
            assert np.array_equal(gpu.selection_feather(mask, radius), SC.feather_expected(size, name, radius)), (name, radius)
            passes, _ = M.feather_params(radius)
            assert (gpu.select_last(4), gpu.select_last(5)) == (passes, 2 * passes)
        assert np.array_equal(mask, keep)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("size", [(65, 66), (259, 131)], ids=SC.size_id)
def test_feather_dev_form(gpu, size, offset):
    w, h = size
    mask = SC.feather_masks(w, h)["random"]
    for radius in (1.0, 9.0):
        with Dev(gpu) as d:
            d_mask, d_out = d.put(mask, offset), d.sentinel((h, w), offset)
            gpu.selection_feather_dev(d_mask, w, h, radius, d_out)
            assert np.array_equal(d.get(d_out, (h, w)), SC.feather_expected(size, "random", radius))
            assert np.array_equal(d.get(d_mask, (h, w)), mask)
            gpu.selection_feather_dev(d_mask, w, h, radius, d_mask)                              # in place
            assert np.array_equal(d.get(d_mask, (h, w)), SC.feather_expected(size, "random", radius))


def test_feather_refusals_leave_the_output_alone(gpu):
    w, h = 65, 66
    mask = SC.feather_masks(w, h)["disc"]
    for radius, status in ((513.0, ERR_UNSUPPORTED), (1e30, ERR_UNSUPPORTED), (float("inf"), ERR_INVALID), (-float("inf"), ERR_INVALID), (float("nan"), ERR_INVALID)):
        out = np.full((h, w), SENTINEL, np.uint8)
        refused(status, gpu.selection_feather, mask, radius, out=out)
        assert (out == SENTINEL).all(), radius
        with Dev(gpu) as d:
            d_mask, d_out = d.put(mask), d.sentinel((h, w))
            refused(status, gpu.selection_feather_dev, d_mask, w, h, radius, d_out)
            assert (d.get(d_out, (h, w)) == SENTINEL).all(), radius


# ---- translate, bounds ---------------------------------------------------------------------------------------------------------------------------------------------
@sizes
def test_translate_equals_the_model(gpu, size):
    w, h = size
    mask = SC.random_bytes(w, h, seed=25)
    keep = mask.copy()
    for dx, dy in [(0, 0), (1, 0), (-1, 0), (0, 1), (64, -3), (-2, 5), (w, 0), (0, -h), (w + 5, h + 5), (INT32_MIN, 0), (0, INT32_MIN), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert np.array_equal(gpu.selection_translate(mask, dx, dy), M.translate(mask, dx, dy)), (dx, dy)
    assert np.array_equal(mask, keep)
    refused(ERR_INVALID, gpu.selection_translate, mask, 1, 1, out=mask)                          # not an in-place op
    assert np.array_equal(mask, keep)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
def test_translate_dev_form(gpu, offset):
    w, h = 259, 131
    mask = SC.random_bytes(w, h, seed=26)
    with Dev(gpu) as d:
        d_mask, d_out = d.put(mask, offset), d.sentinel((h, w), offset)
        for dx, dy in [(64, -3), (-1, 0), (INT32_MIN, 7)]:
            gpu.selection_translate_dev(d_mask, w, h, dx, dy, d_out)
            assert np.array_equal(d.get(d_out, (h, w)), M.translate(mask, dx, dy))
        refused(ERR_INVALID, gpu.selection_translate_dev, d_mask, w, h, 1, 1, d_mask)
        assert np.array_equal(d.get(d_mask, (h, w)), mask)


@sizes
def test_bounds_equal_the_model(gpu, size):
    w, h = size
    single, last_column = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    single[h // 2, w // 3] = 200
    last_column[h - 1, w - 1] = 1
    masks = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "single": single, "value-1": last_column,
             "sparse": SC.morph_masks(w, h)["sparse"], "disc": SC.feather_masks(w, h)["disc"]}
    assert M.bounds(masks["empty"]).tolist() == [-1] * 4 and M.bounds(masks["full"]).tolist() == [0, 0, w - 1, h - 1]
    assert M.bounds(last_column).tolist() == [w - 1, h - 1, w - 1, h - 1]
    for offset in (0, 1):
        with Dev(gpu) as d:
            for name, mask in masks.items():
                d_mask = d.put(mask, offset)
                assert gpu.selection_bounds_dev(d_mask, w, h).tolist() == M.bounds(mask).tolist(), name
                assert np.array_equal(d.get(d_mask, (h, w)), mask)


# ---- fill / delete ---------------------------------------------------------------------------------------------------------------------------------------------------
@sizes
def test_fill_and_delete_equal_the_model(gpu, size):
    w, h = size
    layer, mask = SC.layer(w, h), SC.grey_mask(w, h)
    if w >= 16 and h >= 16:
        assert len(np.unique(mask)) == 256                           # every byte value at least once
    for offset in (0, 1):
        with Dev(gpu) as d:
            d_mask = d.put(mask, offset)
            for color in [(255, 0, 0, 255), (12, 200, 77, 128), (0, 0, 0, 0)]:
                d_layer = d.put(layer)
                gpu.selection_fill_dev(d_layer, d_mask, w, h, color)
                assert np.array_equal(d.get(d_layer, (h, w, 4)), M.fill_selected(layer, mask, color)), color
            d_layer = d.put(layer)
            gpu.selection_delete_dev(d_layer, d_mask, w, h)
            assert np.array_equal(d.get(d_layer, (h, w, 4)), M.delete_selected(layer, mask))
            assert np.array_equal(d.get(d_mask, (h, w)), mask)


def test_fill_and_delete_refusals(gpu):
    w, h = 65, 66
    layer, mask = SC.layer(w, h), SC.grey_mask(w, h)
    with Dev(gpu) as d:
        d_layer, d_mask, d_odd = d.put(layer), d.put(mask), d.put(layer, 1)
        refused(ERR_INVALID, gpu.selection_fill_dev, d_odd, d_mask, w, h, (1, 2, 3, 4))             # the layer is read as dwords
        refused(ERR_INVALID, gpu.selection_delete_dev, d_odd, d_mask, w, h)
        refused(ERR_INVALID, gpu.selection_fill_dev, d_layer, d_layer + 8, w, h, (1, 2, 3, 4))      # the mask inside the layer
        refused(ERR_INVALID, gpu.selection_delete_dev, d_layer, d_layer, w, h)
        assert np.array_equal(d.get(d_layer, (h, w, 4)), layer) and np.array_equal(d.get(d_odd, (h, w, 4)), layer)
