"""The kernels that evaluate a transcendental per pixel, held to an exact model of their device libm (GPU).

Each device result is compared at tolerance 0 with the oracle's device flavour (oracle_lib.libm_flavour("device"): the call
evaluated the way the kernel evaluates it; k_effects2.hip's header, k_libm.h).  A byte may differ from that model only when
the oracle counted ambiguous calls (an f64 result within 4 f64 ulps of an f32 rounding boundary, where the device's f64
routine may round the other way): then by at most 1, on at most that many pixels.  Every case also keeps its comparison
with the reference's glibc flavour: LIBM (+-1 on < 0.1 % of channels) for twist and gaussian noise, EXACT for the rest.
tests/test_libm_model_host.py checks the model itself and that it rejects perturbed models on these same inputs.
"""
import numpy as np
import pytest

from . import libm_cases as LC
from . import oracle_lib as O
from .libm_checks import check_glibc, check_model

pytestmark = pytest.mark.gpu
EXACT, LIBM = "exact", "libm"


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    return GpuBackend(0)


def run_effect(gpu, name, img, kw, mask, cls):
    what = f"{name} {img.shape[1]}x{img.shape[0]} {kw} mask={mask is not None}"
    got = gpu.effect(name, img, mask=mask, **kw)
    check_glibc(got, getattr(O, name)(img, mask=mask, **kw), cls, what)
    return check_model(got, lambda: getattr(O, name)(img, mask=mask, **kw), what)


@pytest.mark.parametrize("angle", LC.TWIST_ANGLES)
def test_twist_vs_device_model(gpu, angle):
    amb = sum(run_effect(gpu, "twist", img, kw, mask, LIBM) for img, kw, mask in LC.twist_cases(angle))
    print(f"twist {angle}: ambiguous calls {amb}")


def test_gaussian_noise_vs_device_model(gpu):
    amb = sum(run_effect(gpu, "add_noise", img, kw, mask, LIBM) for img, kw, mask in LC.noise_cases())
    knife = LC.noise_knife_edge(O)
    assert knife is not None
    img, kw = knife
    got = gpu.effect("add_noise", img, **kw)
    amb += check_model(got, lambda: O.add_noise(img, **kw), f"add_noise knife edge {kw}")
    assert not np.array_equal(got, O.add_noise(img, **kw)), "the knife-edge case must separate the device from glibc"
    print(f"gaussian noise: ambiguous calls {amb}")


def test_noise_colour_branch_is_exact(gpu):
    """gaussian noise without monochrome draws uniform values (no libm call): exact against both flavours"""
    for img, kw, mask in LC.noise_cases():
        kw = dict(kw, monochrome=False)
        assert run_effect(gpu, "add_noise", img, kw, mask, EXACT) == 0


@pytest.mark.parametrize("radius", LC.REDUCE_RADII)
def test_reduce_noise_vs_device_model(gpu, radius):
    """EXACT against both flavours: libm_exp is glibc's expf bit for bit.  Strength 0 sends the off-centre weights of a
    non-flat window into the underflow branch; a NaN strength makes the weight sum NaN and returns the source pixel"""
    for img, kw, mask in LC.reduce_noise_cases(radius):
        assert run_effect(gpu, "reduce_noise", img, kw, mask, EXACT) == 0
    img, kw, _ = LC.reduce_noise_cases(radius)[-1]
    assert np.array_equal(gpu.effect("reduce_noise", img, **kw), img), "NaN strength returns the source"


def test_vignette_vs_device_model(gpu):
    for img, kw, mask in LC.vignette_cases():
        assert run_effect(gpu, "vignette", img, kw, mask, EXACT) == 0


@pytest.mark.parametrize("case", ["compact", "spread"])
def test_displacement_brushes_vs_device_model(gpu, case):
    """the device field is bit-equal (as uint32) to the glibc oracle, to the host pfx_displacement_brush and to the device
    flavour; the warped image is bit-exact"""
    name, w, h, start, batches = next(c for c in LC.dab_batches() if c[0] == case)
    ref = LC.oracle_field(O, start, batches)
    with O.libm_flavour("device"):
        model = LC.oracle_field(O, start, batches)
    host = start.copy()
    for batch in batches:
        for d in batch:
            gpu.r.displacement_brush(host, *d)
    dev = gpu.r.dev_alloc(w * h * 8)
    try:
        gpu.r.dev_upload(dev, start)
        for batch in batches:
            gpu.r.displacement_brushes_dev(dev, w, h, batch)
        got = gpu.r.dev_download(dev, (h, w, 2), np.float32)
        for other, what in ((ref, "glibc oracle"), (host, "host pfx_displacement_brush"), (model, "device-flavour oracle")):
            bad = int((got.view(np.uint32) != other.view(np.uint32)).sum())
            assert bad == 0, f"{case}: field differs from the {what} in {bad} floats"
        img = LC.image(w, h, 5)
        src = gpu.r.dev_alloc(w * h * 4)
        dst = gpu.r.dev_alloc(w * h * 4)
        try:
            gpu.r.dev_upload(src, img)
            gpu.r.warp_displacement_dev(src, w, h, dev, w, h, dst)
            out = gpu.r.dev_download(dst, (h, w, 4), np.uint8)
        finally:
            gpu.r.dev_free(src)
            gpu.r.dev_free(dst)
        assert np.array_equal(out, O.warp_displacement(img, ref)), f"{case}: warped image"
    finally:
        gpu.r.dev_free(dev)
