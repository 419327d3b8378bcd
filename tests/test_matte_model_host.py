"""The CPU model of background removal around the model (tests/matte_model.py), checked on the host (CPU only).

* Transcription: the model equals a pixel-loop transcription of src/ops/ai.rs in plain Python that hoists nothing, on images of a few pixels.
* Hand-derived answers for the places where the reference's wording decides: the frozen pixel, the centre of 128, the feather's 0.5, NaN, the sampling step.
* The feather's integer shortcut: trunc(f32(sum) / f32(2r + 1)) == sum // (2r + 1) for every r in 1 .. 256 and every sum the window can hold.
* The device-flavour expf equals the host's glibc expf on every f32 from +0 to +inf (a C checker compiled here; the oracle's own covers arguments <= 0 only).
* pfx_matte_pick_output (host only, no context) through ctypes.
* The shared cases contain what the GPU test uses them for."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import matte_cases as MC
from . import matte_model as MM
from . import oracle_lib as O
from .test_libm_model_host import needs_glibc_fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = float("nan")


# ---------------------------------------------------------------- the transcription: scalar loops, nothing hoisted
def t_exp(x):
    with O.libm_flavour("device"):
        return O.libm_eval("exp", F(x))[0]


def t_clamp(v, lo, hi):   # f32::clamp
    if v < lo:
        return lo
    if v > hi:
        return hi
    return v


def t_as_u8(v):   # `as u8`: truncating, saturating, NaN -> 0
    if v != v:
        return 0
    return int(min(max(math.trunc(float(v)), 0), 255))


def t_is_probability_space(data):
    if len(data) == 0:
        return False
    step = max(len(data) // 10000, 1)
    mn, mx = F(MM.F32_MAX), F(-MM.F32_MAX)
    for i in range(0, len(data), step):
        v = data[i]
        if v == v:   # f32::min / max: a NaN operand loses
            mn = v if v < mn else mn
            mx = v if v > mx else mx
    return bool(mn >= F(-0.05) and mx <= F(1.05))


def t_to_probability(v, already_prob):
    with np.errstate(all="ignore"):
        if already_prob:
            return t_clamp(v, F(0.0), F(1.0))
        return F(1.0) / (F(1.0) + t_exp(-v))


def t_confidence(data):
    if len(data) == 0:
        return 0.0
    is_prob = t_is_probability_space(data)
    decisive = 0
    for v in data:
        prob = float(t_to_probability(v, is_prob))
        if not (0.1 <= prob <= 0.9):
            decisive += 1
    return decisive / len(data)


def t_expansion(mask, expansion):
    h, w = mask.shape
    current = mask.copy()
    for _ in range(abs(expansion)):
        nxt = current.copy()
        for y in range(h):
            for x in range(w):
                center = int(current[y, x])
                if expansion > 0:
                    if center < 128:
                        best = center
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                nx, ny = x + dx, y + dy
                                if 0 <= nx < w and 0 <= ny < h:
                                    best = max(best, int(current[ny, nx]))
                        nxt[y, x] = best
                elif center > 128:
                    best = center
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            nx, ny = x + dx, y + dy
                            if 0 <= nx < w and 0 <= ny < h:
                                best = min(best, int(current[ny, nx]))
                    nxt[y, x] = best
        current = nxt
    return current


def t_blur(img, radius):
    h, w = img.shape
    r = max(int(math.ceil(F(radius))), 1)
    temp = np.zeros_like(img)
    for y in range(h):
        for x in range(w):
            s, count = F(0.0), F(0.0)
            for dx in range(-r, r + 1):
                s = s + F(img[y, min(max(x + dx, 0), w - 1)])
                count = count + F(1.0)
            temp[y, x] = t_as_u8(s / count)
    out = np.zeros_like(img)
    for y in range(h):
        for x in range(w):
            s, count = F(0.0), F(0.0)
            for dy in range(-r, r + 1):
                s = s + F(temp[min(max(y + dy, 0), h - 1), x])
                count = count + F(1.0)
            out[y, x] = t_as_u8(s / count)
    return out


def t_postprocess(probs, original, s):
    """postprocess_mask on probabilities of the image's own size (the resize is the oracle's and is not restated)"""
    h, w = probs.shape
    mask = np.zeros((h, w), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                prob = probs[y, x]
                if s.smooth_edges:
                    remapped = F(1.0) / (F(1.0) + t_exp(-(prob - F(s.threshold)) * F(12.0)))
                    mask[y, x] = t_as_u8(t_clamp(remapped * F(255.0), F(0.0), F(255.0)))
                else:
                    mask[y, x] = 255 if prob >= F(s.threshold) else 0
    if s.mask_expansion != 0:
        mask = t_expansion(mask, s.mask_expansion)
    if s.fill_holes > 0:
        mask = t_expansion(t_expansion(mask, s.fill_holes), -s.fill_holes)
    if F(s.edge_feather) > F(0.5):
        mask = t_blur(mask, s.edge_feather)
    out = original.copy()
    for y in range(h):
        for x in range(w):
            a = F(out[y, x, 3]) / F(255.0)
            m = F(mask[y, x]) / F(255.0)
            out[y, x, 3] = t_as_u8(t_clamp(a * m * F(255.0), F(0.0), F(255.0)))
    return out, mask


def test_model_equals_the_transcription_stage_by_stage():
    rng = np.random.default_rng(5)
    for (w, h) in ((1, 1), (5, 3), (7, 9)):
        g = rng.integers(0, 256, (h, w), dtype=np.uint8)
        g.ravel()[::4] = np.resize(np.array([127, 128, 129, 0, 255], np.uint8), g.ravel()[::4].size)
        for e in (-3, -1, 1, 2, 4):
            assert np.array_equal(MM.expand(g, e), t_expansion(g, e)), (w, h, e)
        assert np.array_equal(MM.close(g, 2), t_expansion(t_expansion(g, 2), -2))
        for ef in (0.50001, 1.0, 2.5, 7.0):
            assert np.array_equal(MM.feather(g, ef), t_blur(g, ef)), (w, h, ef)


def test_model_equals_the_transcription_of_the_score():
    rng = np.random.default_rng(6)
    for n in (1, 7, 60):
        for kind in ("logit", "prob", "nan"):
            v = (rng.uniform(-6, 6, n) if kind == "logit" else rng.uniform(-0.04, 1.04, n)).astype(np.float32)
            if kind == "nan" and n > 2:
                v[1], v[2] = np.nan, 0.5
            is_prob, conf = MM.confidence(v)
            assert is_prob == t_is_probability_space(v) and conf == t_confidence(v), (n, kind)
            for flag in (False, True):
                want = np.array([t_to_probability(x, flag) for x in v], np.float32)
                assert np.array_equal(MM.to_probability(v, flag).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("preset", sorted(MC.PRESETS))
def test_model_equals_the_transcription_of_the_pipeline(preset):
    s = MC.PRESETS[preset]
    if s.fill_holes > 2:
        s = MM.Settings(s.threshold, s.edge_feather, s.mask_expansion, s.smooth_edges, 2)   # the loops are slow; the count is not what is under test here
    w, h = 9, 7
    probs = MC.soft_blob(w, h, 11, as_logits=False)
    probs[0, 0], probs[3, 4] = np.nan, np.float32(s.threshold)
    img = MC.rgba(w, h, 12)
    got, got_matte = MM.postprocess(probs, img, s, is_probability=1)
    want, want_matte = t_postprocess(MM.to_probability(probs, True), img, s)
    assert np.array_equal(got_matte, want_matte) and np.array_equal(got, want)


def test_tensor_is_the_formula_on_every_byte():
    img = MC.every_byte_image()
    for c in range(3):
        assert sorted(img[..., c].ravel().tolist()) == list(range(256))
    got = MM.tensor(img, 16)
    for c in range(3):
        for y in range(16):
            for x in range(16):
                want = (F(img[y, x, c]) / F(255.0) - MM.MEAN[c]) / MM.STD[c]
                assert got[c, y, x] == want
    assert got.dtype == np.float32


# ---------------------------------------------------------------- hand-derived answers
def test_a_pixel_that_crossed_128_is_frozen():
    # 0 | 200 | 255, two dilations: the 0 takes max(0, 200) = 200 in the first and, at 200 >= 128, stays; a 5 x 5 window maximum would give 255
    assert MM.expand(MC.FROZEN_BARRIER_ROW, 2).tolist() == [[200, 200, 255]]
    assert MM.expand(MC.FROZEN_BARRIER_ROW, 1).tolist() == [[200, 200, 255]]   # the 200 itself is never below 128: it never takes the 255
    # eroding: 255 | 130 | 0: the 255 takes 130, the 130 takes 0; one more step and the first, still above 128, takes the 0 beside it
    assert MM.expand(np.array([[255, 130, 0]], np.uint8), -1).tolist() == [[130, 0, 0]]
    assert MM.expand(np.array([[255, 130, 0]], np.uint8), -2).tolist() == [[0, 0, 0]]
    assert MM.expand(np.array([[255, 100, 0]], np.uint8), -2).tolist() == [[100, 100, 0]]   # 100 <= 128: never replaced, and the 255 that took it is frozen


def test_a_centre_of_128_never_changes():
    g = np.array([[255, 128, 0]], np.uint8)
    assert MM.expand(g, 3)[0, 1] == 128 and MM.expand(g, -3)[0, 1] == 128
    assert MM.expand(g, 1).tolist() == [[255, 128, 128]] and MM.expand(g, -1).tolist() == [[128, 128, 0]]


def test_the_border_is_not_a_neighbour():
    assert MM.expand(np.array([[255]], np.uint8), -5).tolist() == [[255]]   # no in-image neighbour below it
    assert MM.expand(np.array([[0]], np.uint8), 5).tolist() == [[0]]


def test_feather_starts_above_one_half():
    g = np.array([[0, 0, 255, 255]], np.uint8)
    assert MM.feather_radius(0.5) == 0 and np.array_equal(MM.feather(g, 0.5), g)
    assert MM.feather_radius(np.nextafter(F(0.5), F(1))) == 1 and MM.feather_radius(0.50001) == 1
    # r = 1 on one row: windows (0,0,0) (0,0,255) (0,255,255) (255,255,255) -> 0, 85, 170, 255; the column pass of a one-row image repeats the byte
    assert MM.feather(g, 0.50001).tolist() == [[0, 85, 170, 255]]
    assert MM.feather_radius(1.0) == 1 and MM.feather_radius(1.01) == 2 and MM.feather_radius(256.0) == 256
    assert MM.feather(np.array([[0, 0, 255, 255]], np.uint8), 1.01).tolist() == [[51, 102, 153, 204]]   # five edge-clamped samples


def test_nan_probability_under_both_edge_modes():
    v = np.array([[NAN, 0.5, 1.0]], np.float32)
    assert MM.byte(v, True, 0.5, True).tolist() == [[0, 127, 254]]   # 1 / (1 + 1) * 255 = 127.5 -> 127; 1 / (1 + e^-6) * 255 = 254.37
    assert MM.byte(v, True, 0.5, False).tolist() == [[0, 255, 255]]
    assert np.isnan(MM.to_probability(v, True)[0, 0]) and np.isnan(MM.to_probability(v, False)[0, 0])


def test_the_sampling_step_at_its_edge():
    assert [MM.sample_step(n) for n in (1, 9_999, 10_000, 19_999, 20_000, 20_001)] == [1, 1, 1, 1, 2, 2]
    for n in (19_999, 20_000, 20_001):
        base = np.full(n, 0.5, np.float32)
        odd = base.copy()
        odd[1] = 7.0      # index 1: sampled at step 1, skipped at step 2
        even = base.copy()
        even[2] = 7.0     # index 2: always sampled
        assert MM.is_probability_space(odd) == (n >= 20_000), n
        assert not MM.is_probability_space(even)
        is_prob, conf = MM.confidence(odd)
        # as probabilities the 7.0 clamps to 1.0 and is decisive, the rest is 0.5; as logits sigmoid(0.5) = 0.62 is not, sigmoid(7) is
        assert conf == 1 / n and is_prob == (n >= 20_000)


def test_all_nan_is_probability_space_and_wholly_decisive():
    v = np.full(100, np.nan, np.float32)
    assert MM.is_probability_space(v)       # min stays f32::MAX >= -0.05, max stays f32::MIN <= 1.05
    assert MM.confidence(v) == (True, 1.0)
    assert MM.confidence(np.zeros(0, np.float32)) == (False, 0.0)
    assert not MM.is_probability_space(np.array([0.5, np.inf], np.float32)) and not MM.is_probability_space(np.array([-np.inf, 0.5], np.float32))
    assert MM.is_probability_space(np.array([-0.05, 1.05], np.float32)) and not MM.is_probability_space(np.array([np.nextafter(F(-0.05), F(-1))], np.float32))


def test_decisive_uses_the_f64_bounds():
    lo, hi = F(0.1), F(0.9)   # f32(0.1) > 0.1 and f32(0.9) < 0.9: both inside the f64 range
    v = np.array([lo, np.nextafter(lo, F(0)), hi, np.nextafter(hi, F(1))], np.float32)
    q = MM.to_probability(v, True).astype(np.float64)
    assert [not (0.1 <= x <= 0.9) for x in q] == [False, True, False, True]
    assert MM.confidence(v) == (True, 0.5)


def test_apply_truncates_the_product():
    img = np.array([[[1, 2, 3, 255], [4, 5, 6, 128], [7, 8, 9, 0], [1, 1, 1, 255]]], np.uint8)
    out = MM.apply(img, np.array([[255, 128, 255, 0]], np.uint8))
    assert out[0, :, 3].tolist() == [255, 64, 0, 0] and np.array_equal(out[..., :3], img[..., :3])   # 128 * 128 / 255 = 64.25


# ---------------------------------------------------------------- the feather's integer shortcut
def test_truncated_f32_quotient_is_the_integer_quotient_for_every_window():
    checked = 0
    for r in range(1, 257):
        count = 2 * r + 1
        sums = np.arange(255 * count + 1, dtype=np.int64)
        assert sums[-1] < 1 << 24   # the f32 sum of the window is exact
        q = (sums.astype(np.float32) / F(count)).astype(np.int64)   # trunc of the correctly rounded quotient
        assert np.array_equal(q, sums // count), r
        checked += sums.size
    print(f"{checked} (radius, sum) pairs")


# ---------------------------------------------------------------- expf on positive arguments
@needs_glibc_fma
def test_device_expf_equals_glibc_on_every_positive_f32(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "matte_expf_check")
    subprocess.check_call([cc, "-O2", "-fopenmp", "-o", exe, os.path.join(ROOT, "tests", "matte_expf_check.c"), "-lm", "-ldl"])
    O.lib()   # builds the oracle library when it is missing
    out = subprocess.run([exe, O.SO], capture_output=True, text=True, timeout=900, check=True).stdout.split()
    n, bad, first = int(out[0]), int(out[1]), out[2]
    print(f"expf on [+0, +inf] and 4 NaNs: {n} arguments, {bad} differences (first at bits {first})")
    assert n == 0x7f800000 + 1 + 4 and bad == 0
    # the two bounds themselves: the largest finite result and the first overflow
    top = F(float.fromhex("0x1.62e42ep6"))
    assert np.isfinite(MM.expf(top)) and np.isinf(MM.expf(np.nextafter(top, F(np.inf)))) and MM.expf(F(0.0)) == F(1.0)


# ---------------------------------------------------------------- pfx_matte_pick_output
def _pick(input_w, input_h, conf):
    from paintfe_amd import _lib
    lib = _lib.load()
    arr = (C.c_double * max(len(conf), 1))(*conf)
    picked = C.c_uint32(0xdeadbeef)
    st = lib.pfx_matte_pick_output(C.c_uint32(input_w), C.c_uint32(input_h), arr, C.c_uint32(len(conf)), C.byref(picked))
    return st, picked.value


PICK_CASES = [
    # (input w, h, confidences, expected index, why)
    (1024, 1024, [0.90, 0.91, 0.92, 0.93, 0.935], 4, "BiRefNet: the last output, and it is the best"),
    (1024, 1024, [0.94, 0.91, 0.92, 0.93, 0.935], 4, "BiRefNet: the last is within 0.01 of the best"),
    (1024, 1024, [0.95, 0.91, 0.92, 0.93, 0.935], 0, "BiRefNet: the last is outside the window, the best wins"),
    (1024, 1024, [0.90, 0.95, 0.92, 0.93], 1, "IS-Net (four outputs): the first is outside the window"),
    (1024, 1024, [0.945, 0.95, 0.92, 0.93], 0, "IS-Net: the first is inside the window"),
    (320, 320, [0.70, 0.705, 0.709, 0.60, 0.5, 0.4, 0.3], 0, "U2-Net: the first, inside the window"),
    (320, 320, [0.60, 0.705, 0.709, 0.60, 0.5, 0.4, 0.3], 2, "U2-Net: the first is outside"),
    (512, 512, [0.2, 0.8, 0.8, 0.1], 2, "unknown model: equal maxima, max_by keeps the last"),
    (512, 512, [0.8, 0.8], 0, "unknown model: the preferred first is one of the equal maxima"),
    (1024, 1024, [-1.0, 0.5, -1.0, 0.7, -1.0], 3, "BiRefNet: the preferred last output could not be read"),
    (320, 320, [-1.0, 0.3, 0.3], 2, "the first could not be read: the last of the equal maxima"),
    (640, 480, [0.0, 0.0, 0.0], 0, "all zero: everything is within the window"),
    (1024, 320, [0.1, 0.1, 0.1, 0.1, 0.1, 0.2], 5, "not square 1024: unknown, first is outside the window (0.1 < 0.19)"),
    (64, 64, [0.5, 0.49, 0.51], 0, "0.5 >= 0.51 - 0.01 holds in f64"),
]


@pytest.mark.parametrize("case", PICK_CASES, ids=[c[4] for c in PICK_CASES])
def test_pick_output(case):
    iw, ih, conf, want, _ = case
    assert MM.pick_output(iw, ih, conf) == want
    assert _pick(iw, ih, conf) == (0, want)


def test_pick_output_against_the_model_on_random_lists():
    rng = np.random.default_rng(9)
    for _ in range(400):
        n = int(rng.integers(1, 9))
        conf = np.round(rng.uniform(0.8, 0.84, n), 3)
        conf[rng.random(n) < 0.2] = -1.0
        iw = ih = int(rng.choice([320, 1024, 700]))
        want = MM.pick_output(iw, ih, conf.tolist())
        st, got = _pick(iw, ih, conf.tolist())
        assert (st, got) == ((0, want) if want is not None else (-1, 0xdeadbeef)), conf


def test_pick_output_refusals():
    from paintfe_amd import _lib
    lib = _lib.load()
    picked = C.c_uint32(77)
    one = (C.c_double * 1)(0.5)
    assert lib.pfx_matte_pick_output(C.c_uint32(320), C.c_uint32(320), None, C.c_uint32(1), C.byref(picked)) == -1
    assert lib.pfx_matte_pick_output(C.c_uint32(320), C.c_uint32(320), one, C.c_uint32(1), None) == -1
    assert lib.pfx_matte_pick_output(C.c_uint32(320), C.c_uint32(320), one, C.c_uint32(0), C.byref(picked)) == -1
    assert _pick(320, 320, [-1.0, -1.0]) == (-1, 0xdeadbeef) and _pick(320, 320, [NAN]) == (-1, 0xdeadbeef)
    assert picked.value == 77


# ---------------------------------------------------------------- the shared cases hold what they are for
def test_cases_contain_what_the_gpu_test_aims_at():
    assert MC.PRESETS["default"] == MM.Settings() and len(MC.PRESETS) == 4
    for t in MC.THRESHOLDS:
        v = MC.byte_values(t, 1)
        flat = v.ravel()
        assert np.isnan(flat).sum() == 2 and (flat == F(t)).sum() >= 2 and np.nanmin(flat) < 0 and np.nanmax(flat) > 1
        assert not MM.is_probability_space(v)
        hard = MM.byte(v, True, t, False)
        assert set(np.unique(hard)) == {0, 255}
        soft = MM.byte(v, True, t, True)
        assert len(np.unique(soft)) > 100
    for n in MC.SCORE_SIZES:
        lg, pr = MC.planted(MC.logits(n, 2), 3), MC.planted(MC.probabilities(n, 4), 5)
        assert not MM.is_probability_space(lg)
        if n >= 8:
            assert np.isnan(lg).sum() == 1 and np.isinf(pr).sum() == 2
        clean = MC.probabilities(n, 4)
        assert MM.is_probability_space(clean)
        if n > 1:
            assert 0.0 < MM.confidence(clean)[1] < 1.0
    m = MC.morph_inputs(37, 21, 6)
    assert {127, 128, 129} <= set(np.unique(m["noise"])) and m["corners"].sum() == 4 * 255
    two = MM.expand(m["barrier"], 2)
    assert (two[:, 0::5] == 200).all() and (two[:, 3::5][:, :-1] == 255).all()   # left of a 200: frozen at 200; right of a 255: 255
    img, matte = MC.all_alpha_matte_pairs(8)
    assert len({(int(a), int(b)) for a, b in zip(img[..., 3].ravel(), matte.ravel())}) == 65536
    blob = MC.soft_blob(64, 64, 7, as_logits=True)
    assert not MM.is_probability_space(blob) and MM.is_probability_space(MC.soft_blob(64, 64, 7, as_logits=False))
