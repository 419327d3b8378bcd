"""The shape rasteriser's CPU model (tests/shape_model.py) against the reference's 20 shape goldens, and pfx_shape_bounds against the model (no GPU).

* The 14 goldens of kinds without per-pixel libm match the glibc flavour at max diff 0.
* The 6 goldens of the libm kinds are held to the project's LIBM class (+-1 on < 0.1 % of channels) under the glibc flavour.  Channels off by one of
  65 536, with this host's glibc: pentagon_filled 3, hexagon_filled 4, pentagon_outline / hexagon_outline / octagon_outline / star5_outline 0.  They
  sit where the truncating `as u8` of the fill / outline colour mix amplifies a last-ulp difference of one atan2f / cosf result; `%` (fmodf) and the
  casts are as the reference's, and the same model with every atan2 / cos / sin correctly rounded (the device flavour) reproduces all six at 0: the
  seven channels are calls this glibc does not round correctly, not a defect of the restatement.
* Perturbed models (alpha truncated instead of rounded; one multiply-add contracted) change at least one golden.
* pfx_shape_bounds, called through ctypes, equals the model's box."""
import ctypes as C
import math

import numpy as np
import pytest

from paintfe_amd import _lib, shape_bounds

from . import shape_cases as SC
from . import shape_model as M
from .test_gpu_libm_model import EXACT, LIBM, check_glibc


@pytest.fixture(scope="module")
def goldens():
    return SC.load_goldens()


@pytest.mark.parametrize("name", SC.GOLDEN_EXACT)
def test_model_reproduces_the_exact_kinds_goldens(goldens, name):
    img, _ = M.preview(SC.GOLDEN[name], SC.GOLDEN_W, SC.GOLDEN_H, "glibc")
    check_glibc(img, goldens[f"shapes/{name}"], EXACT, name)


@pytest.mark.parametrize("name", SC.GOLDEN_LIBM)
def test_model_reproduces_the_libm_kinds_goldens_in_the_libm_class(goldens, name):
    img, _ = M.preview(SC.GOLDEN[name], SC.GOLDEN_W, SC.GOLDEN_H, "glibc")
    ref = goldens[f"shapes/{name}"]
    print(name, "channels off by one:", int((img != ref).sum()))
    check_glibc(img, ref, LIBM, name)


@pytest.mark.parametrize("name", SC.GOLDEN_LIBM)
def test_device_flavour_reproduces_the_libm_kinds_goldens_in_the_libm_class(goldens, name):
    img, amb = M.preview(SC.GOLDEN[name], SC.GOLDEN_W, SC.GOLDEN_H, "device")
    print(name, "ambiguous calls:", amb)
    check_glibc(img, goldens[f"shapes/{name}"], LIBM, name)


@pytest.mark.parametrize("perturb", ["trunc_alpha", "fma_rotate"])
def test_goldens_reject_perturbed_models(goldens, perturb):
    changed = [n for n in sorted(SC.GOLDEN)
               if not np.array_equal(M.preview(SC.GOLDEN[n], SC.GOLDEN_W, SC.GOLDEN_H, "device", perturb)[0], goldens[f"shapes/{n}"])
               and np.array_equal(M.preview(SC.GOLDEN[n], SC.GOLDEN_W, SC.GOLDEN_H, "device")[0], goldens[f"shapes/{n}"])]
    assert changed, f"no golden notices the {perturb} defect"


def bounds_cases():
    cases = [(f"golden-{n}", s, SC.GOLDEN_W, SC.GOLDEN_H) for n, s in sorted(SC.GOLDEN.items())]
    for rot in (0.0, 0.3, math.pi / 4, -2.1):
        cases.append((f"rot{rot:.2f}", M.shape("triangle", "both", cx=50.3, cy=41.7, hw=30.5, hh=12.25, rotation=rot), 131, 77))
        cases.append((f"parallelogram-rot{rot:.2f}", M.shape("parallelogram", "both", cx=60.0, cy=40.0, hw=25.0, hh=15.0, rotation=rot), 131, 77))
    cases += [("off-left", M.shape("ellipse", "filled", cx=-3.5, cy=40.0, hw=20.0, hh=10.0), 131, 77),
              ("off-right", M.shape("ellipse", "filled", cx=125.5, cy=40.0, hw=20.0, hh=10.0), 131, 77),
              ("off-top", M.shape("heart", "filled", cx=60.0, cy=-2.25, hw=20.0, hh=10.0), 131, 77),
              ("off-bottom", M.shape("star5", "filled", cx=60.0, cy=75.0, hw=20.0, hh=10.0, rotation=0.3), 131, 77),
              ("outside-right", M.shape("rectangle", "both", cx=400.0, cy=40.0, hw=20.0, hh=10.0), 131, 77),
              ("outside-above", M.shape("rectangle", "both", cx=40.0, cy=-400.0, hw=20.0, hh=10.0), 131, 77),
              ("touching-outside", M.shape("rectangle", "both", cx=-22.0, cy=40.0, hw=20.0, hh=10.0), 131, 77),
              ("zero-size", M.shape("rectangle", "both", cx=40.25, cy=30.75, hw=0.0, hh=0.0), 131, 77),
              ("zero-size-on-pixel-edge", M.shape("ellipse", "both", cx=40.0, cy=30.0, hw=0.0, hh=0.0), 131, 77),
              ("huge", M.shape("hexagon", "both", cx=1e30, cy=-1e30, hw=3e38, hh=3e38, rotation=1.0), 131, 77)]
    return cases


@pytest.mark.parametrize("case", bounds_cases(), ids=lambda c: c[0])
def test_shape_bounds_matches_the_model(case):
    _, s, w, h = case
    want = M.bounds(s, w, h)
    assert shape_bounds(SC.to_api(s), w, h) == want
    if case[0].startswith("outside") or case[0] == "touching-outside":
        assert want == (0, 0, 0, 0)
    if case[0].startswith("zero-size"):
        assert want[2] >= 4 and want[3] >= 4      # the pad alone


def test_shape_bounds_refuses_bad_arguments():
    lib = _lib.load()
    box = (C.c_int32 * 4)(7, 7, 7, 7)
    good = SC.to_api(SC.GOLDEN["ellipse_filled"]).to_c()
    assert lib.pfx_shape_bounds(C.byref(good), C.c_uint32(128), C.c_uint32(128), box) == 0 and tuple(box) == (22, 22, 84, 84)
    box = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.pfx_shape_bounds(None, C.c_uint32(128), C.c_uint32(128), box) == _lib.ERR_INVALID
    assert lib.pfx_shape_bounds(C.byref(good), C.c_uint32(128), C.c_uint32(128), None) == _lib.ERR_INVALID
    assert lib.pfx_shape_bounds(C.byref(good), C.c_uint32(0), C.c_uint32(128), box) == _lib.ERR_INVALID
    assert lib.pfx_shape_bounds(C.byref(good), C.c_uint32(20000), C.c_uint32(20000), box) == _lib.ERR_INVALID
    for field, value in (("kind", 17), ("fill_mode", 3), ("cx", math.nan), ("cy", math.inf), ("hw", -math.inf), ("hh", math.nan), ("rotation", math.inf)):
        bad = SC.to_api(SC.GOLDEN["ellipse_filled"]).to_c()
        setattr(bad, field, value)
        assert lib.pfx_shape_bounds(C.byref(bad), C.c_uint32(128), C.c_uint32(128), box) == _lib.ERR_INVALID, field
    assert tuple(box) == (7, 7, 7, 7)


def test_sweep_cases_hold_what_they_are_named_for():
    for kind in M.KINDS:
        g = SC.sweep_geometries(kind)
        lo = lambda d: min(d["hw"], d["hh"])
        assert any(d["hw"] != d["hh"] for d in g.values()) and any(d["rotation"] != 0.0 for d in g.values())
        assert any(d["outline_width"] == 0.0 for d in g.values()) and any(d["outline_width"] > lo(d) for d in g.values())
        assert any(d["corner_radius"] > lo(d) for d in g.values()) and any(d["hw"] == 0.3 for d in g.values())
        assert any(d.get("primary", (0, 0, 0, 255))[3] < 255 and d.get("secondary", (0, 0, 0, 255))[3] < 255 for d in g.values())
        x0, _, bw, _ = M.bounds(M.shape(kind, "both", **g["odd_x0_clipped_right"]), SC.SWEEP_W, SC.SWEEP_H)
        assert x0 % 2 == 1 and x0 + bw == SC.SWEEP_W
    for _, s, bw in SC.width_cases():
        assert M.bounds(s, SC.SWEEP_W, SC.SWEEP_H)[2] == bw
