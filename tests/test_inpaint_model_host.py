"""The content-aware fill CPU model (tests/inpaint_model.py) against the reference's two inpaint goldens, the sweeps' counters, and
pfx_inpaint_ring_offsets against the model (no GPU).

* The model reproduces `inpaint/instant_brush_center` and `inpaint/patchmatch_checkerboard` at tolerance 0.  The instant golden is weak — on its input the
  routine changes no pixel — which is why every sweep case is held to a counter: at least 20 changed pixels, or exactly 0 where the case says "nothing".
* The PatchMatch sweep reaches what it is named for: every patch size and both iteration counts, a hole at least 4 peels deep, the sequential-f32 SSD branch
  (integer sum >= 2^24), boundary pixels left unfilled.
* The integer SSD of the model equals its line-by-line f32 form.
* pfx_inpaint_ring_offsets equals the model's 64 floats bit for bit."""
import ctypes as C

import numpy as np
import pytest

from paintfe_amd import _lib, inpaint_ring_offsets

from . import inpaint_cases as IC
from . import inpaint_model as M


@pytest.fixture(scope="module")
def goldens():
    return IC.load_goldens()


def test_model_reproduces_the_instant_golden(goldens):
    src, mask, out, dabs = IC.golden_instant()
    img, changed = M.instant_list(src, mask, out, dabs)
    assert np.array_equal(img, goldens["inpaint/instant_brush_center"])
    assert changed == 0      # the golden's weakness, on record


def test_model_reproduces_the_patchmatch_golden(goldens):
    src, mask, ps, iters = IC.golden_patchmatch()
    img, k = M.patchmatch(src, mask, ps, iters)
    assert np.array_equal(img, goldens["inpaint/patchmatch_checkerboard"])
    assert k["peels"] == 8 and k["unfilled"] == 0 and k["big_sums"] == 0


@pytest.mark.parametrize("case", IC.instant_cases(), ids=lambda c: c[0])
def test_instant_sweep_cases_change_pixels(case):
    name, src, mask, out, dabs, expect = case
    img, changed = M.instant_list(src, mask, out, dabs)
    print(name, "pixels changed:", changed)
    assert src.shape == (IC.SWEEP_H, IC.SWEEP_W, 4)
    if expect == "nothing":
        assert changed == 0 and np.array_equal(img, out)
    else:
        assert changed >= 20
    assert np.array_equal(img[mask == 0], out[mask == 0])      # only painted-over pixels are touched


def test_instant_sweep_holds_what_it_is_named_for():
    cases = {c[0]: c for c in IC.instant_cases()}
    assert {0.0, 0.5, 1.0} <= {d[4] for c in cases.values() for d in c[4]}
    assert any(d[0] != int(d[0]) and d[1] != int(d[1]) for d in cases["fractional_centre"][4])
    assert set(np.unique(cases["mask_values_1_200_255"][2])) == {0, 1, 200, 255}
    assert not cases["transparent_out_noise"][3].any()
    five = cases["five_overlapping_dabs"][4]
    assert len(five) == 5 and len({d[3] for d in five}) == 2


def test_patchmatch_sweep_holds_what_it_is_named_for():
    specs = IC.PATCHMATCH_SWEEP
    assert {s[3] for s in specs} >= {3, 4, 5, 7, 9, 11} and {s[4] for s in specs} == {3, 6}
    assert {s[0] for s in specs} == {(61, 45), (64, 64)} and {s[2] for s in specs} >= {"palette", "gradnoise", "bw_split"}
    assert {s[1] for s in specs} >= {"corner", "edge", "two", "L", "ring", "blob", "deep"}
    for s in specs:
        _, mask, _, _ = IC.patchmatch_case(s)
        assert 0 < int((mask > 0).sum()) <= 260
    assert set(np.unique(IC.patchmatch_case(specs[5])[1])) == {0, 1, 200, 255}


@pytest.fixture(scope="module")
def sweep_counters():
    return {IC.patchmatch_id(s): M.patchmatch(*IC.patchmatch_case(s))[1] for s in IC.PATCHMATCH_SWEEP if s[1] in ("deep", "small", "ring_pixel_island")}


def test_patchmatch_sweep_counters(sweep_counters):
    for name, k in sweep_counters.items():
        print(name, k)
    assert all(k["peels"] >= 4 for n, k in sweep_counters.items() if "-deep-" in n)
    assert sweep_counters["64x64-small-bw_split-p11-i3"]["big_sums"] > 0
    assert sweep_counters["64x64-ring_pixel_island-palette-p3-i3"]["unfilled"] > 0
    assert sweep_counters["61x45-ring_pixel_island-gradnoise-p1-i6"]["unfilled"] > 0


def test_integer_ssd_equals_the_sequential_f32_ssd():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 40, 4), dtype=np.uint8)
    bw = np.zeros((40, 40, 4), np.uint8)
    bw[:, 20:, :3] = 255
    mask = (rng.random((40, 40)) < 0.15).astype(np.uint8) * 255
    k = M._Counters()
    for image in (img, bw):
        for _ in range(150):
            ax, ay, bx, by = (int(v) for v in rng.integers(0, 40, 4))
            half = int(rng.integers(1, 6))
            mv = max((2 * half + 1) ** 2, 4) // 4
            a, b = M._ssd(image, mask, ax, ay, bx, by, half, mv, k), M.ssd_sequential(image, mask, ax, ay, bx, by, half, mv)
            assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)
    assert k.big_sums > 0


@pytest.mark.parametrize("radius", [24.0, 18.0, 0.5, 1000.0])
def test_ring_offsets_match_the_model(radius):
    assert np.array_equal(inpaint_ring_offsets(radius).view(np.uint32), M.ring_offsets(radius).view(np.uint32))


def test_ring_offsets_null_out_is_a_no_op():
    fn = _lib.load().pfx_inpaint_ring_offsets
    fn.restype = None
    fn(C.c_float(24.0), C.c_void_p(None))
