"""Background removal around the model on the device (k_matte.hip) against the CPU model (tests/matte_model.py), through the Python surface of the C ABI.
Everything here is in the bit-exact class: every comparison is np.array_equal (floats as bit patterns), tolerance 0.  tests/test_matte_model_host.py holds the
model to a scalar transcription of the reference, the expf it uses to the host's glibc, and asserts that the cases of tests/matte_cases.py contain what they are
here for.  The morphology's tile and apron, the resize's output tile and the feather's workgroup shapes come from the library (matte_info), so the sizes below
stay at the kernels' edges if those change."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import matte_cases as MC
from . import matte_model as MM
from .dev_buffers import SENTINEL, Dev

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


def status_of(fn):
    from paintfe_amd import PfxError
    try:
        fn()
    except PfxError as e:
        return e.status
    return OK


def settings_of(s: MM.Settings):
    from paintfe_amd import matte_settings
    return matte_settings(s.threshold, s.edge_feather, s.mask_expansion, s.smooth_edges, s.fill_holes)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def get_f32(d, ptr, shape):
    return d.get(ptr, (int(np.prod(shape)) * 4,)).view(np.float32).reshape(shape)


# ---- tensor -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_tensor_of_every_byte_on_the_copy_path(gpu):
    img = MC.every_byte_image()
    want = MM.tensor(img, 16)
    assert np.array_equal(bits(gpu.matte_tensor(img, 16)), bits(want))
    with Dev(gpu) as d:
        for offset in (0, 4):   # 16-byte aligned planes (four pixels per lane) and not
            p_img, p_out = d.put(img, offset), d.sentinel((3 * 16 * 16 * 4,), offset)
            gpu.matte_tensor_dev(p_img, 16, 16, 16, p_out)
            assert np.array_equal(bits(get_f32(d, p_out, (3, 16, 16))), bits(want)), offset
            assert np.array_equal(d.get(p_img, img.shape), img)


@pytest.mark.parametrize("w,h,size", [(96, 80, 32), (20, 24, 32), (33, 31, 31)])
def test_tensor_behind_the_resize(gpu, w, h, size):
    img = MC.rgba(w, h, 31)
    want = MM.tensor(img, size)
    assert np.array_equal(bits(gpu.matte_tensor(img, size)), bits(want))
    with Dev(gpu) as d:
        p_out = d.sentinel((3 * size * size * 4,))
        gpu.matte_tensor_dev(d.put(img), w, h, size, p_out)
        assert np.array_equal(bits(get_f32(d, p_out, (3, size, size))), bits(want))


# ---- score ------------------------------------------------------------------------------------------------------------------------------------------------------------
def score_inputs(n):
    out = {"logits": MC.planted(MC.logits(n, 40 + n % 7), 41), "probabilities": MC.probabilities(n, 42), "probabilities, planted": MC.planted(MC.probabilities(n, 43), 44),
           "all NaN": np.full(n, np.nan, np.float32)}
    if n > 2:
        for name, at in (("outlier at an odd index", 1), ("outlier at an even index", 2)):   # step 2 from n = 20 000 on: index 1 is then not sampled
            v = np.full(n, 0.5, np.float32)
            v[at] = 7.0
            out[name] = v
    return out


@pytest.mark.parametrize("n", MC.SCORE_SIZES)
def test_score_equals_the_model(gpu, n):
    for name, v in score_inputs(n).items():
        want = MM.confidence(v)
        assert gpu.matte_score(v) == want, (name, want)
        with Dev(gpu) as d:
            for offset in (0, 4):
                assert gpu.matte_score_dev(d.put(v, offset), n) == want, (name, offset)
    if n == 20_001:
        assert MM.confidence(score_inputs(n)["outlier at an odd index"])[0] and not MM.confidence(score_inputs(n)["outlier at an even index"])[0]


def test_score_of_nothing(gpu):
    with Dev(gpu) as d:
        assert gpu.matte_score_dev(d.put(np.zeros(4, np.float32)), 0) == (False, 0.0)


# ---- byte -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", MC.THRESHOLDS)
def test_byte_equals_the_model(gpu, threshold):
    v = MC.byte_values(threshold, 50)
    detected = MM.is_probability_space(v)
    with Dev(gpu) as d:
        p_v = d.put(v)
        for smooth in (True, False):
            for is_prob in (0, 1, -1):
                want = MM.byte(v, detected if is_prob < 0 else bool(is_prob), threshold, smooth)
                p_out = d.sentinel(v.shape)
                gpu.matte_byte_dev(p_v, 128, 128, settings_of(MM.Settings(threshold, 0.0, 0, smooth, 0)), p_out, is_probability=is_prob)
                assert np.array_equal(d.get(p_out, v.shape), want), (smooth, is_prob)
        # off a 16-byte address: one value per lane
        p_off, p_out = d.put(v, offset=4), d.sentinel(v.shape, offset=1)
        gpu.matte_byte_dev(p_off, 128, 128, settings_of(MM.Settings(threshold, 0.0, 0, True, 0)), p_out, is_probability=1)
        assert np.array_equal(d.get(p_out, v.shape), MM.byte(v, True, threshold, True))


# ---- expansion --------------------------------------------------------------------------------------------------------------------------------------------------------
def morph_shapes(gpu):
    t = gpu.matte_info(0)
    return [(1, 1), (1, 7), (t - 1, t - 1), (t, t), (t + 1, t + 1), (2 * t + 3, t + 5)]


def expansions(gpu):
    k = gpu.matte_info(1)
    return [s * e for e in (1, 2, k - 1, k, k + 1, 2 * k + 1, 64) for s in (1, -1)]


@pytest.mark.parametrize("shape_index", range(6))
def test_expand_equals_the_model(gpu, shape_index):
    w, h = morph_shapes(gpu)[shape_index]
    for name, g in MC.morph_inputs(w, h, 60 + shape_index).items():
        with Dev(gpu) as d:
            p_g = d.put(g)
            for e in expansions(gpu) + [0]:
                p_out = d.sentinel(g.shape)
                gpu.matte_expand_dev(p_g, w, h, e, p_out)
                assert np.array_equal(d.get(p_out, g.shape), MM.expand(g, e)), (name, w, h, e)
            assert np.array_equal(d.get(p_g, g.shape), g)


def test_expand_keeps_the_frozen_pixel(gpu):
    with Dev(gpu) as d:
        p_out = d.sentinel((1, 3))
        gpu.matte_expand_dev(d.put(MC.FROZEN_BARRIER_ROW), 3, 1, 2, p_out)
        assert d.get(p_out, (1, 3)).tolist() == [[200, 200, 255]]


@pytest.mark.parametrize("fill_holes", [1, 5, 20])
def test_close_is_a_dilation_run_then_an_erosion_run(gpu, fill_holes):
    w, h = morph_shapes(gpu)[-1]
    for name, g in MC.morph_inputs(w, h, 66).items():
        with Dev(gpu) as d:
            p_mid, p_out = d.sentinel(g.shape), d.sentinel(g.shape)
            gpu.matte_expand_dev(d.put(g), w, h, fill_holes, p_mid)
            gpu.matte_expand_dev(p_mid, w, h, -fill_holes, p_out)
            assert np.array_equal(d.get(p_out, g.shape), MM.close(g, fill_holes)), (name, fill_holes)


# ---- resize -----------------------------------------------------------------------------------------------------------------------------------------------------------
def resize_cases(gpu):
    tx, ty, tall_span, cap = gpu.matte_info(2), gpu.matte_info(3), gpu.matte_info(7), gpu.matte_info(6)
    assert tall_span + 200 < cap
    # the last two: one output tile reaches every source column — more than a full-height tile holds, so the shorter tile runs, at its own row edge too
    wide = [((tall_span + 200, 5), (50, gpu.matte_info(8) + 1)), ((cap, 3), (tx - 3, 2))]
    return wide + [((32, 32), (32, 32)), ((32, 32), (64, 64)), ((32, 32), (256, 256)), ((32, 32), (100, 75)), ((64, 64), (16, 16)), ((1, 1), (5, 5)),
            ((32, 32), (tx - 1, ty - 1)), ((32, 32), (tx, ty)), ((32, 32), (tx + 1, ty + 1)), ((37, 29), (2 * tx + 1, 3 * ty + 1)), ((300, 7), (40, 9))]


@pytest.mark.parametrize("case_index", range(13))
def test_resize_equals_channel_0_of_the_rgba_resize(gpu, case_index):
    (pw, ph), (w, h) = resize_cases(gpu)[case_index]
    for name, g in (("noise", MC.grey_noise(pw, ph, 70 + case_index)), ("step", MC.step_edge(pw, ph))):
        want = MM.resize(g, w, h)
        with Dev(gpu) as d:
            for offset in (0, 1):
                p_out = d.sentinel((h, w), offset)
                gpu.matte_resize_dev(d.put(g, offset), pw, ph, p_out, w, h)
                assert np.array_equal(d.get(p_out, (h, w)), want), (name, offset)


def test_resize_whose_tile_reaches_too_many_columns_is_unsupported(gpu):
    cap = gpu.matte_info(6)
    g = MC.grey_noise(cap + 40, 2, 79)
    with Dev(gpu) as d:
        p_out = d.sentinel((2, 20))
        assert status_of(lambda: gpu.matte_resize_dev(d.put(g), cap + 40, 2, p_out, 20, 2)) == ERR_UNSUPPORTED
        gpu.synchronize()
        assert (d.get(p_out, (2, 20)) == SENTINEL).all()


# ---- feather ----------------------------------------------------------------------------------------------------------------------------------------------------------
def feather_shapes(gpu):
    chunk, cols = gpu.matte_info(4), gpu.matte_info(5)
    return [(3, 2), (cols - 1, 63), (cols, 64), (cols + 1, 65), (chunk - 1, 5), (chunk, 6), (chunk + 1, 7), (70, 161)]


@pytest.mark.parametrize("shape_index", range(8))
def test_feather_equals_the_model(gpu, shape_index):
    w, h = feather_shapes(gpu)[shape_index]
    for name, g in (("noise", MC.grey_noise(w, h, 80 + shape_index)), ("step", MC.step_edge(w, h))):
        with Dev(gpu) as d:
            p_g = d.put(g)
            for ef in MC.FEATHERS:
                p_out = d.sentinel(g.shape)
                gpu.matte_feather_dev(p_g, w, h, ef, p_out)
                assert np.array_equal(d.get(p_out, g.shape), MM.feather(g, ef)), (name, w, h, ef)
    assert np.array_equal(MM.feather(g, 0.5), g) and not np.array_equal(MM.feather(g, 0.50001), g)


# ---- apply ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_apply_on_every_alpha_matte_pair(gpu):
    img, matte = MC.all_alpha_matte_pairs(90)
    want = MM.apply(img, matte)
    with Dev(gpu) as d:
        for offset in (0, 4):
            p_img, p_matte, p_out = d.put(img, offset), d.put(matte, offset // 4), d.sentinel(img.shape, offset)
            gpu.matte_apply_dev(p_img, p_matte, 256, 256, p_out)
            assert np.array_equal(d.get(p_out, img.shape), want), offset
            gpu.matte_apply_dev(p_img, p_matte, 256, 256, p_img)   # in place
            assert np.array_equal(d.get(p_img, img.shape), want), offset
            assert np.array_equal(d.get(p_matte, matte.shape), matte)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------------------------------------
PROB = 320


@functools.lru_cache(maxsize=None)
def model_output(kind):
    return MC.soft_blob(PROB, PROB, 100, as_logits=(kind == "logits"))


@functools.lru_cache(maxsize=None)
def document(w, h):
    return MC.rgba(w, h, 101)


@functools.lru_cache(maxsize=None)
def modelled(kind, preset, w, h):
    return MM.postprocess(model_output(kind), document(w, h), MC.PRESETS[preset])


def composed(gpu, d, p_values, p_img, w, h, s: MM.Settings, p_result):
    """the stage calls, as the header composes them; returns the pointer of the final matte"""
    S = settings_of(s)
    p_a, p_b = d.sentinel((PROB, PROB)), d.sentinel((PROB, PROB))
    gpu.matte_byte_dev(p_values, PROB, PROB, S, p_a)
    for e in (s.mask_expansion, s.fill_holes, -s.fill_holes):
        if e != 0:
            gpu.matte_expand_dev(p_a, PROB, PROB, e, p_b)
            p_a, p_b = p_b, p_a
    p_full, p_soft = d.sentinel((h, w)), d.sentinel((h, w))
    gpu.matte_resize_dev(p_a, PROB, PROB, p_full, w, h)
    gpu.matte_feather_dev(p_full, w, h, s.edge_feather, p_soft)
    gpu.matte_apply_dev(p_img, p_soft, w, h, p_result)
    return p_soft


@pytest.mark.parametrize("w,h", [(333, 250), (PROB, PROB)], ids=["onto 333x250", "onto 320x320"])
@pytest.mark.parametrize("kind,preset", [("logits", "default"), ("probabilities", "default"), ("logits", "portrait"), ("logits", "conservative"),
                                         ("probabilities", "aggressive")])
def test_postprocess_equals_the_stage_calls_and_the_model(gpu, kind, preset, w, h):
    s = MC.PRESETS[preset]
    values, img = model_output(kind), document(w, h)
    want, want_matte = modelled(kind, preset, w, h)
    assert 0 < int((want[..., 3] != img[..., 3]).sum()) and len(np.unique(want_matte)) > (2 if s.smooth_edges else 1)
    with Dev(gpu) as d:
        p_values, p_img = d.put(values), d.put(img)
        # the stage calls composed
        p_stage = d.sentinel(img.shape)
        p_stage_matte = composed(gpu, d, p_values, p_img, w, h, s, p_stage)
        assert np.array_equal(d.get(p_stage_matte, (h, w)), want_matte)
        assert np.array_equal(d.get(p_stage, img.shape), want)
        # one call, with the matte
        p_out, p_matte = d.sentinel(img.shape), d.sentinel((h, w))
        gpu.matte_postprocess_dev(p_values, PROB, PROB, p_img, w, h, settings_of(s), p_out, p_matte)
        assert np.array_equal(d.get(p_matte, (h, w)), want_matte)
        assert np.array_equal(d.get(p_out, img.shape), want)
        # without it, and with the verdict handed in
        p_out2 = d.sentinel(img.shape)
        gpu.matte_postprocess_dev(p_values, PROB, PROB, p_img, w, h, settings_of(s), p_out2, is_probability=int(kind == "probabilities"))
        assert np.array_equal(d.get(p_out2, img.shape), want)
        assert np.array_equal(d.get(p_img, img.shape), img) and np.array_equal(bits(get_f32(d, p_values, values.shape)), bits(values))
        # in place
        gpu.matte_postprocess_dev(p_values, PROB, PROB, p_img, w, h, settings_of(s), p_img)
        assert np.array_equal(d.get(p_img, img.shape), want)
    # the host tier
    got, got_matte = gpu.matte_postprocess(values, img, settings_of(s), with_matte=True)
    assert np.array_equal(got, want) and np.array_equal(got_matte, want_matte)
    assert np.array_equal(gpu.matte_postprocess(values, img, settings_of(s)), want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_context_working(gpu):
    w = h = 16
    n = w * h
    img, values, grey = MC.rgba(w, h, 110), MC.probabilities(n, 111).reshape(h, w), MC.grey_noise(w, h, 112)
    good = settings_of(MM.Settings())
    nan = float("nan")
    with Dev(gpu) as d:
        p_img, p_values, p_grey = d.put(img), d.put(values), d.put(grey)
        p_rgba_out, p_grey_out, p_tensor = d.sentinel(img.shape), d.sentinel(grey.shape), d.sentinel((3 * n * 4,))
        lib, ctx = gpu._lib, gpu._h
        u32, vp = C.c_uint32, C.c_void_p
        INV, UNS = ERR_INVALID, ERR_UNSUPPORTED
        cases = [
            ("tensor: size 0", INV, lambda: gpu.matte_tensor_dev(p_img, w, h, 0, p_tensor)),
            ("tensor: NULL image", INV, lambda: gpu.matte_tensor_dev(0, w, h, 16, p_tensor)),
            ("tensor: NULL tensor", INV, lambda: gpu.matte_tensor_dev(p_img, w, h, 16, 0)),
            ("tensor: zero width", INV, lambda: gpu.matte_tensor_dev(p_img, 0, h, 16, p_tensor)),
            ("tensor: over the document limit", INV, lambda: gpu.matte_tensor_dev(p_img, 20000, 20000, 16, p_tensor)),
            ("tensor: size over the limit", INV, lambda: gpu.matte_tensor_dev(p_img, w, h, 20000, p_tensor)),
            ("tensor: misaligned image", INV, lambda: gpu.matte_tensor_dev(p_img + 1, w, h, 4, p_tensor)),
            ("tensor: misaligned tensor", INV, lambda: gpu.matte_tensor_dev(p_img, w, h, 4, p_tensor + 2)),
            ("tensor: output inside the input", INV, lambda: gpu.matte_tensor_dev(p_img, w, h, 4, p_img + 8)),
            ("score: NULL values", INV, lambda: gpu.matte_score_dev(0, n)),
            ("score: misaligned values", INV, lambda: gpu.matte_score_dev(p_values + 2, n - 1)),
            ("score: too many values", INV, lambda: gpu.matte_score_dev(p_values, 256_000_001)),
            ("score: NULL is_probability", INV, lambda: gpu._check(lib.pfx_matte_score_dev(ctx, vp(p_values), C.c_size_t(n), None, C.byref(C.c_double())))),
            ("score: NULL confidence", INV, lambda: gpu._check(lib.pfx_matte_score_dev(ctx, vp(p_values), C.c_size_t(n), C.byref(C.c_int32()), None))),
            ("byte: NULL settings", INV, lambda: gpu._check(lib.pfx_matte_byte_dev(ctx, vp(p_values), u32(w), u32(h), C.c_int32(1), None, vp(p_grey_out)))),
            ("byte: NaN threshold", INV, lambda: gpu.matte_byte_dev(p_values, w, h, settings_of(MM.Settings(threshold=nan)), p_grey_out)),
            ("byte: infinite feather", INV, lambda: gpu.matte_byte_dev(p_values, w, h, settings_of(MM.Settings(edge_feather=float("inf"))), p_grey_out)),
            ("byte: is_probability 2", INV, lambda: gpu.matte_byte_dev(p_values, w, h, good, p_grey_out, is_probability=2)),
            ("byte: is_probability -2", INV, lambda: gpu.matte_byte_dev(p_values, w, h, good, p_grey_out, is_probability=-2)),
            ("byte: misaligned values", INV, lambda: gpu.matte_byte_dev(p_values + 1, w, h - 1, good, p_grey_out)),
            ("byte: output inside the input", INV, lambda: gpu.matte_byte_dev(p_values, w, h, good, p_values)),
            ("expand: in place", INV, lambda: gpu.matte_expand_dev(p_grey, w, h, 1, p_grey)),
            ("expand: NULL output", INV, lambda: gpu.matte_expand_dev(p_grey, w, h, 1, 0)),
            ("expand: 65", UNS, lambda: gpu.matte_expand_dev(p_grey, w, h, 65, p_grey_out)),
            ("expand: -65", UNS, lambda: gpu.matte_expand_dev(p_grey, w, h, -65, p_grey_out)),
            ("resize: zero height", INV, lambda: gpu.matte_resize_dev(p_grey, w, h, p_grey_out, w, 0)),
            ("resize: overlapping", INV, lambda: gpu.matte_resize_dev(p_grey, w, h, p_grey + 5, 4, 4)),
            ("feather: NaN", INV, lambda: gpu.matte_feather_dev(p_grey, w, h, nan, p_grey_out)),
            ("feather: in place", INV, lambda: gpu.matte_feather_dev(p_grey, w, h, 2.0, p_grey)),
            ("feather: 256.5", UNS, lambda: gpu.matte_feather_dev(p_grey, w, h, 256.5, p_grey_out)),
            ("apply: NULL matte", INV, lambda: gpu.matte_apply_dev(p_img, 0, w, h, p_rgba_out)),
            ("apply: misaligned result", INV, lambda: gpu.matte_apply_dev(p_img, p_grey, w, h - 1, p_rgba_out + 1)),
            ("apply: result shifted into the image", INV, lambda: gpu.matte_apply_dev(p_img, p_grey, w, h - 1, p_img + 4)),
            ("apply: result over the matte", INV, lambda: gpu.matte_apply_dev(p_img, p_grey, 8, 8, p_grey)),
            ("postprocess: NULL settings", INV, lambda: gpu._check(lib.pfx_matte_postprocess_dev(ctx, vp(p_values), u32(w), u32(h), C.c_int32(-1), vp(p_img), u32(w), u32(h), None,
                                                                                                  vp(p_rgba_out), None))),
            ("postprocess: NaN threshold", INV, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, settings_of(MM.Settings(threshold=nan)), p_rgba_out)),
            ("postprocess: is_probability 5", INV, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, good, p_rgba_out, is_probability=5)),
            ("postprocess: matte over the result", INV, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, good, p_rgba_out, p_rgba_out)),
            ("postprocess: matte over the values", INV, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, good, p_rgba_out, p_values)),
            ("postprocess: result shifted into the image", INV, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h - 1, good, p_img + 4)),
            ("postprocess: over the document limit", INV, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, 20000, 20000, good, p_rgba_out)),
            ("postprocess: expansion 65", UNS, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, settings_of(MM.Settings(mask_expansion=65)), p_rgba_out)),
            ("postprocess: fill_holes 65", UNS, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, settings_of(MM.Settings(fill_holes=65)), p_rgba_out)),
            ("postprocess: feather 257", UNS, lambda: gpu.matte_postprocess_dev(p_values, w, h, p_img, w, h, settings_of(MM.Settings(edge_feather=257.0)), p_rgba_out)),
        ]
        for name, want, call in cases:
            assert status_of(call) == want, name
            gpu.synchronize()
            assert (d.get(p_rgba_out, img.shape) == SENTINEL).all() and (d.get(p_grey_out, grey.shape) == SENTINEL).all(), name
            assert (d.get(p_tensor, (3 * n * 4,)) == SENTINEL).all(), name
            assert np.array_equal(d.get(p_img, img.shape), img) and np.array_equal(d.get(p_grey, grey.shape), grey), name
            assert np.array_equal(bits(get_f32(d, p_values, values.shape)), bits(values)), name
        # the caps themselves are accepted
        gpu.matte_expand_dev(p_grey, w, h, -64, p_grey_out)
        assert np.array_equal(d.get(p_grey_out, grey.shape), MM.expand(grey, -64))
        gpu.matte_feather_dev(p_grey, w, h, 256.0, p_grey_out)
        assert np.array_equal(d.get(p_grey_out, grey.shape), MM.feather(grey, 256.0))
    want = img.copy()
    want[..., :3] = 255 - want[..., :3]
    assert np.array_equal(gpu.invert_rgba(img), want)
