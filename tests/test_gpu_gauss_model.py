"""GPU: the default-mode Gaussian held to the float64 model of its own arithmetic (tests/gauss_model.py), not just to +-1 LSB of the f32
oracle.  Where the model's value lies more than eps (the derived bound, 0.005 .. 0.015 LSB) from a rounding boundary the device byte
must be the model's; across row segments, strip widths, aligned / unaligned instantiations and bands the outputs must be bit-identical.

Covers every radius 1 .. 80 of the matrix-core kernel (every Toeplitz alignment, K-block count 4 .. 12) on impulse / edge / adversarial /
ramp images, both piece counts the model knows ("gauss_parts" 12 shipped, 22), 32- and 64-column strips, row segments 1, 2, 3, 5 and
automatic, 4-byte-misaligned buffers with w % 4 == 0, odd widths, small and ragged shapes, bands, the default-mode selection, the VALU
path (radius > 80 and in place) and the fused chain epilogue.  Run with -s for the measured ambiguous / differing shares."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libpfx.so is loaded (tests/test_gpu_fullsize.py: PyTorch must bring up the HIP runtime first)

from . import gauss_model as G
from . import inputs as I
from . import oracle_lib as O

pytestmark = pytest.mark.gpu

DEFAULT_KNOBS = {"gauss_cols64": 6, "gauss_parts": 12, "gauss_mfma_segments": 0}


@pytest.fixture(scope="module")
def r():
    from paintfe_amd import GpuRenderer
    rr = GpuRenderer(0)
    rr.set_exact(False)
    yield rr
    for k, v in DEFAULT_KNOBS.items():
        rr.tune(k, v)
    rr.close()


def run(r, img, sigma, knobs=None, offset=0, in_place=False, first_row=0):
    """gaussian_blur_dev on device copies of img; offset: bytes added to both buffer addresses (4 = 16-byte misaligned)"""
    h, w = img.shape[:2]
    a = r.dev_alloc(img.nbytes + 64)
    b = a if in_place else r.dev_alloc(img.nbytes + 64)
    try:
        for k, v in (knobs or {}).items():
            r.tune(k, v)
        r.dev_upload(a + offset, img)
        r.gaussian_blur_dev(a + offset, b + offset, w, h, sigma, first_row=first_row)
        r.synchronize()
        return r.dev_download(b + offset, img.shape)
    finally:
        for k in (knobs or {}):
            r.tune(k, DEFAULT_KNOBS[k])
        r.dev_free(a)
        if b != a:
            r.dev_free(b)


def report(what, res: G.CheckResult, eps):
    print(f"gauss_model: {what}: eps {eps:.4f} ambiguous {res.ambiguous:.2e} differ {res.differ:.2e} worst {res.worst:.4f}")


@pytest.mark.parametrize("radius", range(1, G.MFMA_MAXR + 1))
def test_every_radius_every_variant_matches_the_model(r, radius):
    sigma = G.sigma_for_radius(radius)
    eps = G.eps_mfma(radius)
    img = G.impulse_image(radius, sigma, variant=radius % 2, min_w=200, min_h=660)   # 660 rows: 5 segments of >= 4 steps
    h, w = img.shape[:2]
    m = G.model_mfma(img, sigma)
    base = run(r, img, sigma)
    res = G.check(m, eps, base, f"r={radius} shipped")
    G.check_true_gaussian(img, sigma, eps, base, f"r={radius}")
    report(f"r={radius} nkb={G.nkb(radius)} {w}x{h}", res, eps)
    wa = w - w % 4   # the aligned instantiation needs w % 4 == 0
    img4 = np.ascontiguousarray(img[:, :wa])
    base4 = base if wa == w else run(r, img4, sigma)
    if wa != w:
        G.check(G.model_mfma(img4, sigma), eps, base4, f"r={radius} width {wa}")
    for cols in (0, 7):
        for seg in (0, 1, 2, 3, 5):
            out = run(r, img4, sigma, {"gauss_cols64": cols, "gauss_mfma_segments": seg})
            assert np.array_equal(out, base4), f"r={radius} cols64={cols} segments={seg}: {int((out != base4).sum())} channels differ"
    for seg in (0, 3):   # the unaligned instantiation through 4-byte-offset buffers, w % 4 == 0
        out = run(r, img4, sigma, {"gauss_mfma_segments": seg}, offset=4)
        assert np.array_equal(out, base4), f"r={radius} misaligned buffers, segments={seg}: {int((out != base4).sum())} channels differ"
    odd = np.ascontiguousarray(img4[:, :wa - 1])
    mo = G.model_mfma(odd, sigma)
    oo = run(r, odd, sigma)
    G.check(mo, eps, oo, f"r={radius} odd width {wa - 1}")
    assert np.array_equal(run(r, odd, sigma, {"gauss_mfma_segments": 2}), oo), f"r={radius} odd width, 2 segments"
    e22 = G.eps_mfma(radius, 22)
    o22 = run(r, img4, sigma, {"gauss_parts": 22})
    res22 = G.check(G.model_mfma(img4, sigma, 22), e22, o22, f"r={radius} gauss_parts=22")
    report(f"r={radius} parts 22", res22, e22)
    assert np.array_equal(run(r, img4, sigma, {"gauss_parts": 22, "gauss_mfma_segments": 3}), o22), f"r={radius} parts 22, 3 segments"


@pytest.mark.parametrize("sigma", [1.0, 5.3, 10.6, 16.0, 26.6])
def test_shapes_match_the_model(r, sigma):
    """widths either side of 32, 64 and 4k, heights either side of 32 and 128, single rows / columns, images smaller than the window"""
    rad = G.radius_of(sigma)
    eps = G.eps_mfma(rad)
    src = G.impulse_image(rad, sigma, 1, min_w=260, min_h=260)
    for (w, h) in [(31, 33), (32, 32), (33, 31), (63, 127), (64, 128), (65, 129), (68, 40), (4, 200), (8, 8), (1, 50), (50, 1), (1, 1), (3, 100),
                   (100, 3), (129, 257), (260, 31)]:
        img = np.ascontiguousarray(src[:h, :w])
        G.check(G.model_mfma(img, sigma), eps, run(r, img, sigma), f"sigma {sigma} {w}x{h}", max_ambiguous=8 * eps + 0.05)


@pytest.mark.parametrize("sigma", [3.0, 16.0, 26.6])
def test_bands_match_the_model_and_the_whole_image(r, sigma):
    rad = G.radius_of(sigma)
    eps = G.eps_mfma(rad)
    img = G.impulse_image(rad, sigma, 0, min_w=196, min_h=2 * rad + 200)
    H = img.shape[0]
    m = G.model_mfma(img, sigma)
    whole = run(r, img, sigma)
    G.check(m, eps, whole, f"sigma {sigma} whole")
    bh = 2 * rad + 64
    for fr in (0, 1, 31, 32, 33, 100):
        band = np.ascontiguousarray(img[fr:fr + bh])
        out = run(r, band, sigma, first_row=fr)
        lo, hi = (0 if fr == 0 else rad), min(bh, H - fr) - (0 if fr + bh >= H else rad)
        assert np.array_equal(out[lo:hi], whole[fr + lo:fr + hi]), f"sigma {sigma} band at {fr}: differs from the whole-image call"
        G.check(m[fr + lo:fr + hi], eps, out[lo:hi], f"sigma {sigma} band at {fr}")


@pytest.mark.parametrize("sigma", [3.0, 12.0])
def test_selection_in_default_mode_matches_the_model(r, sigma):
    """blur_with_selection in the default mode: the padded bounding box blurred as its own image (matrix-core kernel), selected pixels
    (grey mask values included) follow the model, the others are the source"""
    img = I.random_rgba(200, 120, 9)
    img[:, 100:, 1] = 255
    mask = np.zeros((120, 200), np.uint8)
    mask[30:70, 50:140] = 255
    mask[35, 60] = 0
    mask[100:110, 180:200] = 7
    dev = r.gaussian_blur_core(img, sigma, mask)
    m, sel = G.crop_mask_model(img, mask, sigma, G.model_mfma)
    G.check(m[sel], G.eps_mfma(G.radius_of(sigma)), dev[sel], f"selection sigma {sigma}")
    assert np.array_equal(dev[~sel], img[~sel]), "unselected pixels changed"


@pytest.mark.parametrize("sigma,in_place", [(26.7, False), (40.0, False), (100.0, False), (2.0, True), (16.0, True)])
def test_valu_path_matches_the_fma_model(r, sigma, in_place):
    rad = G.radius_of(sigma)
    img = np.ascontiguousarray(G.impulse_image(20, G.sigma_for_radius(20), 0)[:150, :236])
    eps = G.eps_valu(rad)
    out = run(r, img, sigma, in_place=in_place)
    res = G.check(G.model_valu(img, sigma), eps, out, f"VALU sigma {sigma} in_place={in_place}")
    report(f"VALU sigma {sigma} in_place={in_place}", res, eps)


@pytest.mark.parametrize("sigma", [3.0, 8.0, 14.0, 20.0])
def test_chain_epilogue_equals_the_ops_on_the_model(r, sigma):
    """pfx_chain_dev Gaussian -> pointwise ops in the matrix-core kernel's store (chain_mfma = 1): on pixels whose four blurred channels are all
    outside the band, the chain's result is the oracle's ops applied to the model's rounded blur"""
    from .test_gpu_chain import run_chain
    rad = G.radius_of(sigma)
    eps = G.eps_mfma(rad)
    img = np.ascontiguousarray(G.impulse_image(rad, sigma, 1, 256, 160)[:160, :256])
    m = G.model_mfma(img, sigma)
    firm = (np.abs(m - np.floor(m) - 0.5) > eps).all(-1)
    assert firm.mean() > 0.9
    blur = G.model_rounded(m)
    try:
        r.tune("chain_mfma", 1)
        for heavy in (0, 1):
            r.tune("chain_fuse_heavy", heavy)
            for post in ([("adjust", "hsl", (30.0, -20.0, 10.0))], [("adjust", "exposure", (0.4,)), ("adjust", "invert")]):
                got = run_chain(r, img, [("gaussian", sigma)] + post)
                want = blur
                for o in post:
                    want = O.adjust(want, o[1], o[2] if len(o) > 2 else ())
                bad = (got != want).any(-1) & firm
                assert not bad.any(), f"sigma {sigma} heavy={heavy} {post[0][1]}: {int(bad.sum())} firm pixels differ"
    finally:
        r.tune("chain_mfma", 1); r.tune("chain_fuse_heavy", 0)


def test_noise_sigma16_ambiguous_and_differing_shares(r):
    img = I.random_rgba(1024, 512, 5)
    sigma = 16.0
    eps = G.eps_mfma(48)
    out = run(r, img, sigma)
    res = G.check(G.model_mfma(img, sigma), eps, out, "noise sigma 16")
    report("noise 1024x512 sigma 16", res, eps)
    assert res.differ <= res.ambiguous
    G.check_true_gaussian(img, sigma, eps, out, "noise sigma 16")
