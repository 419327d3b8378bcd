"""Inputs of the background-removal tests, shared by tests/test_matte_model_host.py (which asserts that they contain what they are here for) and
tests/test_gpu_matte.py."""
import numpy as np

from .matte_model import Settings

# the dialog's "Default" button and its three presets (ref: src/ui/dialogs/effects/ai.rs:150-186); Default equals RemoveBgSettings::default()
PRESETS = {
    "default": Settings(0.5, 0.0, 0, True, 0),
    "portrait": Settings(0.5, 1.0, 1, True, 8),
    "conservative": Settings(0.3, 1.0, 2, True, 5),
    "aggressive": Settings(0.7, 0.0, -1, False, 0),
}

SCORE_SIZES = (1, 9_999, 10_000, 20_001, 65_540)
THRESHOLDS = (0.05, 0.5, 0.95)
FEATHERS = (0.5, 0.50001, 1.0, 1.01, 20.0, 256.0)
FROZEN_BARRIER_ROW = np.array([[0, 200, 255]], np.uint8)   # two dilations: the 0 takes 200 and is frozen there


def rgba(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def every_byte_image():
    """16 x 16: channel c holds every byte value once, each channel in another order; alpha varies too (it must not show)"""
    k = np.arange(256, dtype=np.uint8)
    img = np.stack([k, k[::-1], np.roll(k, 77), (k * 5 + 3).astype(np.uint8)], axis=-1)
    return np.ascontiguousarray(img.reshape(16, 16, 4))


def logits(n, seed):
    return np.random.default_rng(seed).uniform(-20.0, 20.0, n).astype(np.float32)


def probabilities(n, seed):
    """bimodal like a decoder output, with a soft band: some values inside 0.1 .. 0.9"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.08, n), rng.uniform(0.93, 1.0, n))
    soft = rng.random(n) < 0.2
    return np.where(soft, rng.uniform(0.0, 1.0, n), v).astype(np.float32)


def planted(values, seed):
    """NaN and both infinities at random places (never index 0, so that the cases below can aim at it)"""
    v = values.copy()
    if v.size >= 8:
        at = np.random.default_rng(seed).choice(np.arange(1, v.size), 3, replace=False)
        v[at[0]], v[at[1]], v[at[2]] = np.nan, np.inf, -np.inf
    return v


def byte_values(threshold, seed):
    """128 x 128 probabilities-or-logits: random in -0.2 .. 1.3 plus 0, 1, the threshold, its two f32 neighbours, NaN, -0.2 and 1.3"""
    t = np.float32(threshold)
    v = np.random.default_rng(seed).uniform(-0.2, 1.3, (128, 128)).astype(np.float32)
    special = [0.0, 1.0, t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2)), np.nan, -0.2, 1.3]
    v.ravel()[:len(special)] = np.array(special, np.float32)
    v.ravel()[5000:5000 + len(special)] = np.array(special, np.float32)
    return v


def morph_inputs(w, h, seed):
    """name -> (h, w) uint8: random bytes with 127 / 128 / 129 planted, an 8-px checkerboard, a 255 in each corner, the frozen-barrier row repeated"""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    noise.ravel()[::7] = np.resize(np.array([127, 128, 129], np.uint8), noise.ravel()[::7].size)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((xx // 8 + yy // 8) & 1) * 255).astype(np.uint8)
    corners = np.zeros((h, w), np.uint8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 255
    barrier = np.zeros((h, w), np.uint8)
    barrier[:, 1::5] = 200
    barrier[:, 2::5] = 255
    return {"noise": noise, "checker": checker, "corners": corners, "barrier": barrier}


def grey_noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def step_edge(w, h):
    g = np.zeros((h, w), np.uint8)
    g[:, w // 2:] = 255
    g[h // 2:, :] ^= 255
    return g


def soft_blob(w, h, seed, as_logits):
    """a model-like output: a soft-edged blob with holes and specks, as probabilities or as logits"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    d = np.hypot((xx - w * 0.45) / (w * 0.3), (yy - h * 0.55) / (h * 0.35))
    z = (1.0 - d) * 9.0 + rng.normal(0.0, 1.2, (h, w))
    z[rng.random((h, w)) < 0.002] *= -1.0   # holes inside, specks outside
    z = z.astype(np.float32)
    if as_logits:
        return z
    return (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)


def all_alpha_matte_pairs(seed):
    """a 256 x 256 image whose alpha is the row and a matte that is the column: all 65 536 pairs; rgb random"""
    img = rgba(256, 256, seed)
    img[..., 3] = np.arange(256, dtype=np.uint8)[:, None]
    matte = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :], (256, 256)))
    return img, matte
