"""CPU checks of tests/gauss_model.py itself: the float64 model of the default-mode Gaussian keeps flat images, agrees with the CPU
oracle to the stated +-1 LSB, and its checker rejects outputs of deliberately wrong models on the inputs the GPU test uses (so the GPU
test can see each of these bug classes).  No GPU: the tap tables come from the library's host-side builder."""
import numpy as np
import pytest

from . import gauss_model as G
from . import inputs as I
from . import oracle_lib as O


@pytest.mark.parametrize("sigma", [0.5, 2.0, 5.4, 16.0, 26.6])
def test_flat_images_are_fixed_points_of_the_model(sigma):
    r = G.radius_of(sigma)
    for parts in (12, 22):
        eps = G.eps_mfma(r, parts)
        for level in (0, 1, 127, 128, 254, 255):
            flat = np.full((40, 70, 4), level, np.uint8)
            m = G.model_mfma(flat, sigma, parts)
            assert np.abs(m - level).max() < 0.02, (sigma, parts, level, float(np.abs(m - level).max()))
            G.check(m, eps, flat, f"flat {level} sigma {sigma} parts {parts}")


@pytest.mark.parametrize("sigma", [0.5, 2.0, 5.4, 11.0, 16.0, 20.0, 26.6])
def test_model_agrees_with_the_oracle(sigma):
    """within +-1 everywhere, and equal to the f32 oracle on all channels outside the band but a small counted share (the table moves
    an image by < 0.1 LSB per pass, the oracle's own f32 rounding is ~1e-5 LSB)"""
    r = G.radius_of(sigma)
    for img in (I.random_rgba(150, 90, 3 + r), G.impulse_image(r, sigma, 0, 120, 100)):
        ref = O.gaussian_blur(img, sigma)
        m = G.model_mfma(img, sigma)
        got = G.model_rounded(m)
        assert np.abs(got.astype(int) - ref).max() <= 1, sigma
        amb = np.abs(m - np.floor(m) - 0.5) <= G.eps_mfma(r)
        share = float(((got != ref) & ~amb).mean())
        assert share < 0.02, f"sigma {sigma}: {share:.2e} of the channels differ from the oracle"
        G.check_true_gaussian(img, sigma, G.eps_mfma(r), ref, f"oracle sigma {sigma}")


def test_eps_is_small_and_grows_with_the_k_blocks():
    e = [G.eps_mfma(r) for r in (1, 16, 17, 48, 49, 80)]
    assert e == sorted(e) and e[0] > 0.004 and e[-1] < 0.02, e
    assert [G.nkb(r) for r in (1, 16, 17, 32, 33, 48, 49, 64, 65, 80)] == [4, 4, 6, 6, 8, 8, 10, 10, 12, 12]
    assert G.eps_mfma(80, 22) < 0.02 and G.eps_valu(300) < 0.02


# ------------------------------------------------------------------ sensitivity: every wrong model is rejected

def _wrong_outputs(img, sigma):
    """device-like outputs of models with one deliberate mistake each"""
    r = G.radius_of(sigma)
    w1, w2, ws = G.f16_tables(sigma)
    h, w = img.shape[:2]
    out = {}
    tail = ws.copy(); tail[-1] = 0.0
    out["tail tap zero"] = G.sep_conv(img, tail) * 2.0 ** -16
    out["taps shifted by one"] = G.sep_conv(img, np.roll(ws, 1)) * 2.0 ** -16
    if r < 80:   # at 12 K blocks the whole table error (sum|delta| / 2 * 255 / 256 = 0.017 LSB at r = 80) is as small as eps itself
        out["f32 taps instead of the f16 table"] = G.sep_conv(img, 256.0 * G.f32_taps(sigma)) * 2.0 ** -16
    Hx = G.horiz(img, ws)
    for c in (1, 2, 3):   # one channel's vertical pass reads a stale ring row: image rows 31 mod 32 hold the previous row's H (an isolated impulse
        #                   in R blurs below 1/2 LSB from sigma ~ 6 on: nothing to see there; small sigmas add channel 0 below)
        stale = Hx.copy()
        rows = np.arange(31, h, 32)
        stale[rows, :, c] = Hx[rows - 1, :, c]
        out[f"channel {c} with the previous row's H"] = G.vert(stale, ws) * 2.0 ** -16
    if r <= 4:
        stale = Hx.copy(); rows = np.arange(31, h, 32); stale[rows, :, 0] = Hx[rows - 1, :, 0]
        out["channel 0 with the previous row's H"] = G.vert(stale, ws) * 2.0 ** -16
    out["right border clamps one column early"] = G.sep_conv(img, ws, clamp_hi_x=w - 2) * 2.0 ** -16
    rounded = {k: G.model_rounded(v) for k, v in out.items()}
    m = G.model_mfma(img, sigma)
    rounded["truncation instead of rounding"] = np.clip(np.floor(m), 0, 255).astype(np.uint8)
    f16 = np.asarray(m, np.float16).astype(np.float64)   # the epilogue in half precision, rounded half away from zero
    rounded["f16 epilogue, half away from zero"] = np.clip(np.floor(f16 + 0.5), 0, 255).astype(np.uint8)
    return m, rounded


@pytest.mark.parametrize("sigma", [0.8, 1.2, G.sigma_for_radius(16), G.sigma_for_radius(17), 16.0, G.sigma_for_radius(80)])
def test_checker_rejects_each_wrong_model(sigma):
    r = G.radius_of(sigma)
    eps = G.eps_mfma(r)
    img = G.impulse_image(r, sigma, 0)
    m, wrong = _wrong_outputs(img, sigma)
    G.check(m, eps, G.model_rounded(m), f"sigma {sigma}: the model itself")
    for name, dev in wrong.items():
        with pytest.raises(AssertionError, match="differ from the model") as ei:
            G.check(m, eps, dev, f"sigma {sigma}: {name}")
        print(ei.value)


def test_checker_bounds():
    m = np.array([0.2, 0.5, 0.495, 254.6, 255.003, -0.001, 7.5 + 1e-3])
    G.check(m, 0.01, np.array([0, 0, 0, 255, 255, 0, 8]), max_ambiguous=1.0)
    G.check(m, 0.01, np.array([0, 1, 1, 255, 255, 0, 7]), max_ambiguous=1.0)    # inside the band either neighbour
    with pytest.raises(AssertionError, match="differ from the model"):
        G.check(m, 0.01, np.array([1, 0, 0, 255, 255, 0, 8]), max_ambiguous=1.0)
    with pytest.raises(AssertionError, match="vacuous"):
        G.check(np.full(100, 3.5), 0.01, np.full(100, 4))
