"""GPU: the two-pass VALU Gaussian (k_gauss.hip: gauss_h_kernel / gauss_v_kernel) on the rows of tests/gauss_valu_cases.py: every vertical tile
shape, radii 17 .. 850, both sides of every switch point of the tile choice, widths and heights beside the tiles' edges.

  * bit-exact mode: every (radius, shape) row equals the oracle at tolerance 0;
  * default mode, radius >= 81 (the fmaf build of the two passes, out of place): within 1 LSB of the oracle and held to the float64 model
    of its arithmetic (gauss_model.model_valu, eps_valu) like test_gpu_gauss_model.py::test_valu_path_matches_the_fma_model;
  * in place (src == dst), with the caller's scratch and with the context's: the bytes of the out-of-place call (bit-exact mode), the model
    (default mode, where in place is the only road to the fmaf passes at radius <= 80);
  * every vertical tile shape forced through the "gauss_v_cfg" knob gives the bytes of the shipped choice, in both modes; a forced shape that
    does not fit LDS is refused, writes nothing and leaves the context usable;
  * the radius limit: 850 runs, 851 is refused as unsupported with dst untouched;
  * a selection whose padded bounding box is the whole image, at radius 381.

tests/test_gauss_valu_cases_host.py shows, without a device, that the rows' oracle results are what the reference's arithmetic gives and that
the tall and wide rows see a dropped tap or a wrong clamp."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libpfx.so is loaded (tests/test_gpu_fullsize.py: PyTorch must bring up the HIP runtime first)

from . import gauss_model as G
from . import gauss_valu_cases as V
from . import oracle_lib as O

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def r():
    from paintfe_amd import GpuRenderer
    rr = GpuRenderer(0)
    yield rr
    rr.tune("gauss_v_cfg", 0)
    rr.set_exact(False)
    rr.close()


@pytest.fixture(autouse=True)
def stop_after_a_device_error(r):
    """a HIP error behind a test ends the session: nothing more is launched on a device that has reported one"""
    yield
    from paintfe_amd import PfxError
    try:
        r.synchronize()
    except PfxError as e:
        pytest.exit(f"the device reported an error after this test: {e}", returncode=3)


def run(r, img, sigma, exact, in_place=False, own_tmp=False, knob=0, prefill=None):
    """gaussian_blur_dev on device copies of img.  own_tmp: the caller supplies the f32 intermediate (w * h * 16 bytes), else the context's
    scratch is used.  knob: the "gauss_v_cfg" value for this call (process-wide: always put back to 0).  prefill: dst's bytes before the call."""
    h, w = img.shape[:2]
    r.set_exact(exact)
    a = r.dev_alloc(img.nbytes + 64)
    b = a if in_place else r.dev_alloc(img.nbytes + 64)
    t = r.dev_alloc(w * h * 16 + 64) if own_tmp else 0
    try:
        r.dev_upload(a, img)
        if prefill is not None:
            assert not in_place
            r.dev_upload(b, np.full(img.shape, prefill, np.uint8))
        r.tune("gauss_v_cfg", knob)
        try:
            r.gaussian_blur_dev(a, b, w, h, sigma, tmp_ptr=t)
        finally:
            r.tune("gauss_v_cfg", 0)
            r.synchronize()
        return r.dev_download(b, img.shape)
    except Exception as e:
        if prefill is not None:
            e.dst = r.dev_download(b, img.shape)
        raise
    finally:
        r.dev_free(a)
        if b != a:
            r.dev_free(b)
        if t:
            r.dev_free(t)


def differing(a, b):
    return int((a != b).sum())


def check_model(img, sigma, radius, out, what):
    res = G.check(G.model_valu(img, sigma), G.eps_valu(radius), out, what)
    print(f"gauss_valu_edges: {what}: eps {G.eps_valu(radius):.4f} ambiguous {res.ambiguous:.2e} differ {res.differ:.2e} worst {res.worst:.4f}")


@pytest.mark.parametrize("radius", V.RADII)
def test_every_row_equals_the_oracle_in_exact_mode(r, radius):
    sigma = G.sigma_for_radius(radius)
    for (w, h) in V.shapes(radius):
        out = run(r, V.image(w, h, radius), sigma, exact=True)
        want = V.oracle(w, h, radius)
        assert np.array_equal(out, want), f"r={radius} {w}x{h} tile {V.v_tile(radius)[:3]}: {differing(out, want)} bytes differ from the oracle"


@pytest.mark.parametrize("radius", [x for x in V.RADII if x > G.MFMA_MAXR])
def test_every_row_matches_the_fma_model_in_default_mode(r, radius):
    sigma = G.sigma_for_radius(radius)
    for (w, h) in V.shapes(radius):
        img = V.image(w, h, radius)
        out = run(r, img, sigma, exact=False)
        d = int(np.abs(out.astype(np.int16) - V.oracle(w, h, radius).astype(np.int16)).max())
        assert d <= 1, f"r={radius} {w}x{h}: {d} LSB from the oracle"
        check_model(img, sigma, radius, out, f"r={radius} {w}x{h}")


def in_place_shapes(radius):
    return [V.tall_shape(radius), V.wide_shape(radius), V.tile_edge_shapes(V.v_tile(radius)[2])[2], (V.H_TILE + 1, 3)]


@pytest.mark.parametrize("radius", [17, 80, 381, 850])
def test_in_place_exact(r, radius):
    sigma = G.sigma_for_radius(radius)
    for (w, h) in in_place_shapes(radius):
        img = V.image(w, h, radius)
        apart = run(r, img, sigma, exact=True)
        for own_tmp in (True, False):
            out = run(r, img, sigma, exact=True, in_place=True, own_tmp=own_tmp)
            assert np.array_equal(out, apart), f"r={radius} {w}x{h} own_tmp={own_tmp}: in place differs from out of place in {differing(out, apart)} bytes"
            assert np.array_equal(out, V.oracle(w, h, radius)), f"r={radius} {w}x{h} own_tmp={own_tmp}: differs from the oracle"


@pytest.mark.parametrize("radius", [17, 80])
def test_in_place_default_mode_matches_the_fma_model(r, radius):
    sigma = G.sigma_for_radius(radius)
    for (w, h) in in_place_shapes(radius):
        img = V.image(w, h, radius)
        outs = []
        for own_tmp in (True, False):
            out = run(r, img, sigma, exact=False, in_place=True, own_tmp=own_tmp)
            check_model(img, sigma, radius, out, f"in place r={radius} {w}x{h} own_tmp={own_tmp}")
            outs.append(out)
        assert np.array_equal(outs[0], outs[1]), f"r={radius} {w}x{h}: the result depends on whose scratch holds the intermediate"


@pytest.mark.parametrize("radius", sorted(V.FORCED))
def test_forced_tile_shapes_give_the_shipped_bytes(r, radius):
    sigma = G.sigma_for_radius(radius)
    knobs = V.FORCED[radius]
    assert knobs[0] == 0
    seen = set()
    for exact in (True, False):
        in_place = (not exact) and radius <= G.MFMA_MAXR   # default mode up to radius 80: only in place runs the two passes
        for knob in knobs[1:]:
            cfg, tx, rows, lds = V.v_tile(radius, knob)
            assert cfg == knob and lds <= V.LDS_LIMIT
            seen.add(cfg)
            for (w, h) in V.forced_shapes(radius, knob):
                img = V.image(w, h, radius)
                base = run(r, img, sigma, exact, in_place=in_place, knob=0)
                out = run(r, img, sigma, exact, in_place=in_place, knob=knob)
                assert np.array_equal(out, base), (f"r={radius} {w}x{h} exact={exact} tile {tx}x{rows} (gauss_v_cfg={knob}): "
                                                   f"{differing(out, base)} bytes differ from the shipped tile {V.v_tile(radius)[1:3]}")
                if exact:
                    assert np.array_equal(out, V.oracle(w, h, radius)), f"r={radius} {w}x{h} gauss_v_cfg={knob}: differs from the oracle"
                else:
                    check_model(img, sigma, radius, out, f"r={radius} {w}x{h} gauss_v_cfg={knob}")
    assert seen == set(knobs[1:])


@pytest.mark.parametrize("exact", [True, False])
def test_a_forced_shape_that_does_not_fit_is_refused(r, exact):
    from paintfe_amd import PfxError
    radius, knob = V.REFUSED
    assert V.v_tile(radius, knob)[3] > V.LDS_LIMIT
    sigma = G.sigma_for_radius(radius)
    w, h = 13, 270
    img = V.image(w, h, radius)
    try:
        with pytest.raises(PfxError) as ei:
            run(r, img, sigma, exact, knob=knob, prefill=0xA5)
        assert (ei.value.dst == 0xA5).all(), "the refused call wrote into dst"
    finally:
        r.tune("gauss_v_cfg", 0)
    out = run(r, img, sigma, exact)   # the context is usable, and the knob is back
    if exact:
        assert np.array_equal(out, V.oracle(w, h, radius))
    else:
        check_model(img, sigma, radius, out, f"after the refusal, r={radius}")


def test_radius_limit(r):
    from paintfe_amd import PfxError
    assert G.radius_of(G.sigma_for_radius(V.MAX_RADIUS)) == V.MAX_RADIUS and G.radius_of(283.34) == V.MAX_RADIUS + 1
    w, h = 9, 7
    img = V.image(w, h, V.MAX_RADIUS)
    for exact in (True, False):
        out = run(r, img, G.sigma_for_radius(V.MAX_RADIUS), exact, prefill=0xA5)
        if exact:
            assert np.array_equal(out, V.oracle(w, h, V.MAX_RADIUS))
        else:
            check_model(img, G.sigma_for_radius(V.MAX_RADIUS), V.MAX_RADIUS, out, "radius 850")
        with pytest.raises(PfxError) as ei:
            run(r, img, 283.34, exact, prefill=0xA5)
        assert ei.value.status == ERR_UNSUPPORTED, ei.value
        assert (ei.value.dst == 0xA5).all(), "the refused call wrote into dst"


def test_selection_whose_padded_box_is_the_whole_image(r):
    radius = 381
    sigma = G.sigma_for_radius(radius)
    w, h = 40, 300
    img = V.image(w, h, radius)
    mask = np.zeros((h, w), np.uint8)
    mask[120:170, 10:30] = 255
    mask[130, 15] = 0
    mask[2:5, 36:40] = 9
    assert radius >= max(w, h)   # the bounding box padded by the radius covers the image
    r.set_exact(True)
    try:
        out = r.gaussian_blur_core(img, sigma, mask)
    finally:
        r.set_exact(False)
    want = O.gaussian_blur(img, sigma, mask)
    assert np.array_equal(out, want), f"{differing(out, want)} bytes differ from the oracle"
    assert not np.array_equal(out, img) and np.array_equal(out[mask == 0], img[mask == 0])
