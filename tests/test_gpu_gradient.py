"""The gradient tool and the perspective crop on the device (k_gradient.hip) against the CPU model (tests/gradient_model.py), through the C ABI.  Everything is
in the EXACT class — single correctly rounded f32 operations, an exact remainder, integer arithmetic — so every comparison is np.array_equal.
tests/test_gradient_model_host.py holds the model to a scalar transcription and to hand-derived answers and asserts that the cases below reach every branch,
so nothing here passes vacuously.  Every base pointer is tried at offset 0 (where 64 x 8, 130 x 70 at scale 3 and the large case take the four-pixel arm) and
4 bytes in (the pixel arm)."""
import ctypes as C

import numpy as np
import pytest

from . import gradient_cases as GC
from . import gradient_model as M
from .dev_buffers import SENTINEL, DevBuffers, differing, sentinel_like

pytestmark = pytest.mark.gpu

OK, ERR_INVALID = 0, -1
LEADS = pytest.mark.parametrize("lead", [0, 4], ids=["aligned", "4-bytes-in"])


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


def describe(g):
    from paintfe_amd import gradient
    return gradient(g["start"], g["end"], g["shape"], g["repeat"], g["mode"], g["preview_scale"])


def no_selection(w, h):
    return np.full((h, w), 255, np.uint8)       # uploaded in every case, handed over only where the case has a selection


# ---- render ----------------------------------------------------------------------------------------------------------------------------------------------------------
def run_render(gpu, name, lead, sel_lead=None):
    c = GC.CASES[name]
    w, h, sel = c["w"], c["h"], GC.selection_of(name)
    want, want_pm, _ = GC.rendered(name)
    sel_bufs = DevBuffers(gpu, no_selection(w, h) if sel is None else sel, lead=lead if sel_lead is None else sel_lead)
    bufs = DevBuffers(gpu, sentinel_like(want), sentinel_like(want), lead=lead)
    with sel_bufs as (d_sel,), bufs as (d_out, d_pm):
        gpu.gradient_render_dev(describe(c["g"]), GC.lut(), w, h, d_out, selection_ptr=0 if sel is None else d_sel, premul_ptr=d_pm if c["premul"] else 0)
        got, got_pm = gpu.dev_download(d_out, want.shape), gpu.dev_download(d_pm, want.shape)
        n = differing(got, want)
        print(f"{name} lead={lead}: {n} differing pixels of {want.shape[0] * want.shape[1]}")
        assert np.array_equal(got, want), n
        assert np.array_equal(got_pm, want_pm) if c["premul"] else (got_pm == SENTINEL).all()
        assert bufs.surroundings_intact() and sel_bufs.surroundings_intact()
        assert np.array_equal(gpu.dev_download(d_sel, (h, w)), no_selection(w, h) if sel is None else sel)      # only read


@LEADS
@pytest.mark.parametrize("name", GC.NAMES)
def test_render_equals_the_model(gpu, name, lead):
    run_render(gpu, name, lead)


@pytest.mark.parametrize("name", [n for n in GC.NAMES if n.startswith("64x8-") and GC.CASES[n]["sel"] is not None])
def test_render_four_pixel_arm_with_a_selection_off_a_dword(gpu, name):
    """the selection is a byte plane: any address is allowed, and one byte in the quads read it byte by byte"""
    run_render(gpu, name, 0, sel_lead=1)


@pytest.mark.parametrize("name", ["67x5-scale2", "130x70-reflected-clamp-erase", "64x8-linear-clamp-colour", "1x1"])
def test_render_through_host_buffers(gpu, name):
    c = GC.CASES[name]
    want, want_pm, _ = GC.rendered(name)
    got, got_pm = gpu.gradient_render(describe(c["g"]), GC.lut(), c["w"], c["h"], selection=GC.selection_of(name), premultiplied=True)
    assert np.array_equal(got, want) and np.array_equal(got_pm, want_pm)
    assert np.array_equal(gpu.gradient_render(describe(c["g"]), GC.lut(), c["w"], c["h"], selection=GC.selection_of(name)), want)


@LEADS
def test_render_past_the_grid_stride_bound(gpu, lead):
    """4100 x 2049: more quads than 8192 workgroups x 256 lanes, so every lane of the four-pixel arm takes a second trip (offset 0); the pixel arm takes five"""
    w, h = GC.BIG
    g, want = GC.big()
    bufs = DevBuffers(gpu, sentinel_like(want), lead=lead)
    with bufs as (d_out,):
        gpu.gradient_render_dev(describe(g), GC.lut(), w, h, d_out)
        got = gpu.dev_download(d_out, want.shape)
        assert bufs.surroundings_intact()
    assert np.array_equal(got, want), differing(got, want)


# ---- commit and apply --------------------------------------------------------------------------------------------------------------------------------------------------
@LEADS
@pytest.mark.parametrize("name,is_eraser", GC.COMMITS)
def test_commit_equals_the_model(gpu, name, is_eraser, lead):
    c = GC.CASES[name]
    w, h = c["w"], c["h"]
    layer, preview, want = GC.layer(w, h), GC.rendered(name)[0], GC.committed(name, is_eraser)
    bufs = DevBuffers(gpu, layer, preview, lead=lead)
    with bufs as (d_layer, d_preview):
        gpu.gradient_commit_dev(d_layer, d_preview, w, h, is_eraser)                                # the layer in place
        got = gpu.dev_download(d_layer, layer.shape)
        assert np.array_equal(got, want), differing(got, want)
        assert np.array_equal(gpu.dev_download(d_preview, preview.shape), preview) and bufs.surroundings_intact()
    assert np.array_equal(gpu.gradient_commit(layer, preview, is_eraser), want)                     # through host buffers
    assert np.array_equal(layer, GC.layer(w, h))


APPLY_NAMES = [n for n in GC.NAMES if GC.CASES[n]["g"]["preview_scale"] == 1]


@LEADS
@pytest.mark.parametrize("name", APPLY_NAMES)
def test_apply_equals_render_then_commit_and_the_model(gpu, name, lead):
    c = GC.CASES[name]
    w, h, sel, g = c["w"], c["h"], GC.selection_of(name), describe(c["g"])
    layer = GC.layer(w, h)
    want = M.commit(layer, GC.rendered(name)[0], c["g"]["mode"] == M.TRANSPARENCY)
    assert not np.array_equal(want, layer)
    sel_bufs = DevBuffers(gpu, no_selection(w, h) if sel is None else sel, lead=lead)
    bufs = DevBuffers(gpu, layer, layer, sentinel_like(layer), lead=lead)
    with sel_bufs as (d_sel,), bufs as (d_fused, d_two, d_preview):
        s = 0 if sel is None else d_sel
        gpu.gradient_apply_dev(g, GC.lut(), d_fused, w, h, selection_ptr=s)
        gpu.gradient_render_dev(g, GC.lut(), w, h, d_preview, selection_ptr=s)
        gpu.gradient_commit_dev(d_two, d_preview, w, h, c["g"]["mode"] == M.TRANSPARENCY)
        fused, two = gpu.dev_download(d_fused, layer.shape), gpu.dev_download(d_two, layer.shape)
        assert np.array_equal(fused, two), differing(fused, two)
        assert np.array_equal(fused, want), differing(fused, want)
        assert bufs.surroundings_intact() and sel_bufs.surroundings_intact()


# ---- perspective crop ----------------------------------------------------------------------------------------------------------------------------------------------------
@LEADS
@pytest.mark.parametrize("quad", GC.CROP_NAMES)
@pytest.mark.parametrize("w,h", GC.CROP_SIZES)
def test_crop_equals_the_model(gpu, w, h, quad, lead):
    from paintfe_amd import perspective_crop_plan
    corners, layer = GC.quads(w, h)[quad], GC.layer(w, h)
    want, _ = GC.cropped(w, h, quad)
    assert perspective_crop_plan(corners, w, h) == (want.shape[1], want.shape[0])
    bufs = DevBuffers(gpu, layer, sentinel_like(want), lead=lead)
    with bufs as (d_layer, d_out):
        gpu.perspective_crop_dev(corners, [d_layer], [d_out], w, h)
        got = gpu.dev_download(d_out, want.shape)
        print(f"{w}x{h} {quad} lead={lead}: {differing(got, want)} differing pixels of {want.shape[0] * want.shape[1]}")
        assert np.array_equal(got, want), differing(got, want)
        assert np.array_equal(gpu.dev_download(d_layer, layer.shape), layer) and bufs.surroundings_intact()
    if lead == 0:
        assert np.array_equal(gpu.perspective_crop(corners, layer), want)                            # one layer through host buffers


@pytest.mark.parametrize("w,h", GC.CROP_SIZES)
def test_crop_three_layers_in_one_call_equal_three_calls(gpu, w, h):
    corners = GC.quads(w, h)["beyond"]
    layers = [GC.layer(w, h, seed) for seed in (3, 4, 5)]
    wants = [GC.cropped(w, h, "beyond", seed)[0] for seed in (3, 4, 5)]
    assert not np.array_equal(wants[0], wants[1])
    bufs = DevBuffers(gpu, *layers, *[sentinel_like(x) for x in wants], *[sentinel_like(x) for x in wants])
    with bufs as ptrs:
        ins, together, alone = ptrs[:3], ptrs[3:6], ptrs[6:]
        gpu.perspective_crop_dev(corners, ins, together, w, h)
        for k in range(3):
            gpu.perspective_crop_dev(corners, [ins[k]], [alone[k]], w, h)
        for k in range(3):
            a, b = gpu.dev_download(together[k], wants[k].shape), gpu.dev_download(alone[k], wants[k].shape)
            assert np.array_equal(a, b) and np.array_equal(a, wants[k]), k
        assert bufs.surroundings_intact()


@pytest.mark.parametrize("w,h", GC.CROP_SIZES)
def test_crop_refuses_a_quad_the_reference_returns_none_for(gpu, w, h):
    from paintfe_amd import PfxError, perspective_crop_plan
    corners, layer = GC.none_quad(w, h), GC.layer(w, h)
    assert perspective_crop_plan(corners, w, h) is None
    bufs = DevBuffers(gpu, layer, sentinel_like(layer))
    with bufs as (d_layer, d_out):
        with pytest.raises(PfxError) as e:
            gpu.perspective_crop_dev(corners, [d_layer], [d_out], w, h)
        assert e.value.status == ERR_INVALID
        assert (gpu.dev_download(d_out, layer.shape) == SENTINEL).all() and bufs.surroundings_intact()
    with pytest.raises(PfxError):
        gpu.perspective_crop(corners, layer)


# ---- the argument contract -----------------------------------------------------------------------------------------------------------------------------------------------
W, H = 67, 5
SLOT, N_SLOTS = 4096, 8
NAN, INF = float("nan"), float("inf")
GOOD = M.gradient(*GC.drag(W, H), M.RADIAL, True)
QUAD = GC.quads(W, H)["inside"]
# entry point -> its buffers in call order: name, kind (in / out / opt = an optional input / optout = an optional output; rgba or mask)
CONTRACT = {
    "pfx_gradient_render_dev": [("sel", "opt:mask"), ("preview", "out:rgba"), ("premul", "optout:rgba")],
    "pfx_gradient_render": [("sel", "opt:mask"), ("preview", "out:rgba"), ("premul", "optout:rgba")],
    "pfx_gradient_commit_dev": [("layer", "out:rgba"), ("preview", "in:rgba")],
    "pfx_gradient_commit": [("layer", "out:rgba"), ("preview", "in:rgba")],
    "pfx_gradient_apply_dev": [("sel", "opt:mask"), ("layer", "out:rgba")],
    "pfx_perspective_crop_dev": [("layer0", "in:rgba"), ("layer1", "in:rgba"), ("cropped0", "out:rgba"), ("cropped1", "out:rgba")],
    "pfx_perspective_crop": [("layer", "in:rgba"), ("cropped", "out:rgba")],
}


@pytest.fixture(scope="module")
def arena(gpu):
    rng = np.random.default_rng(22)
    pattern = rng.integers(0, 256, SLOT * N_SLOTS, dtype=np.uint8)
    pattern[rng.random(pattern.size) < 0.4] = 0
    dev = gpu.dev_alloc(pattern.size)
    yield dict(pattern=pattern, host=pattern.copy(), dev=dev)
    gpu.dev_free(dev)


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_argument_contract(gpu, arena, name):
    lib, bufs, dev = gpu._lib, CONTRACT[name], name.endswith("_dev")
    fn = getattr(lib, name)
    fn.restype = C.c_int
    slots = {b: i for i, (b, _) in enumerate(bufs)}
    base_addr = arena["dev"] if dev else arena["host"].ctypes.data
    address = lambda b, shift=0: base_addr + slots[b] * SLOT + shift
    lut = np.ascontiguousarray(GC.lut())
    is_crop = "crop" in name

    def restore():
        arena["host"][:] = arena["pattern"]
        gpu.dev_upload(arena["dev"], arena["pattern"])
        gpu.synchronize()

    def untouched():
        gpu.synchronize()
        return np.array_equal(gpu.dev_download(arena["dev"], arena["pattern"].shape), arena["pattern"]) and np.array_equal(arena["host"], arena["pattern"])

    def call(ptrs=None, g=GOOD, dims=(W, H), table=True, corners=QUAD, n_layers=None, eraser=0):
        """ptrs: buffer name -> address (None = NULL); g None = a NULL descriptor; table False = a NULL LUT; corners None = NULL corners"""
        p = {b: address(b) for b, _ in bufs}
        p.update(ptrs or {})
        a = {b: C.c_void_p(p[b]) for b, _ in bufs}
        d = None if g is None else C.byref(describe(g))
        t = lut.ctypes.data_as(C.c_void_p) if table else None
        w, h = C.c_uint32(dims[0]), C.c_uint32(dims[1])
        cs = None if corners is None else (C.c_float * 8)(*[float(v) for c in corners for v in c])
        if name.startswith("pfx_gradient_render"):
            return fn(gpu.handle, d, t, a["sel"], w, h, a["preview"], a["premul"])
        if name.startswith("pfx_gradient_commit"):
            return fn(gpu.handle, a["layer"], a["preview"], w, h, C.c_int(eraser))
        if name == "pfx_gradient_apply_dev":
            return fn(gpu.handle, d, t, a["sel"], a["layer"], w, h)
        if name == "pfx_perspective_crop_dev":
            ins, outs = (C.c_void_p * 2)(p["layer0"], p["layer1"]), (C.c_void_p * 2)(p["cropped0"], p["cropped1"])
            return fn(gpu.handle, cs, ins, outs, C.c_uint32(2 if n_layers is None else n_layers), w, h)
        return fn(gpu.handle, cs, a["layer"], a["cropped"], C.c_size_t(SLOT), w, h)

    wrong = []

    def expect(what, status, want):
        if status != want:
            wrong.append(f"{what}: {status}, expected {want}")

    restore()
    expect("the valid call", call(), OK)
    for b, kind in bufs:
        if kind.startswith("opt"):
            expect(f"the valid call without {b}", call({b: None}), OK)
    restore()
    # ---- refusals ----
    for b, kind in bufs:
        if not kind.startswith("opt"):
            expect(f"{b} = NULL", call({b: None}), ERR_INVALID)
    expect("20000 x 20000", call(dims=(20000, 20000)), ERR_INVALID)
    expect("w = 0", call(dims=(0, H)), ERR_INVALID)
    expect("h = 0", call(dims=(W, 0)), ERR_INVALID)
    if is_crop:
        expect("corners = NULL", call(corners=None), ERR_INVALID)
        for k in range(4):
            for bad in (NAN, INF, -INF):
                corners = [tuple(c) for c in QUAD]
                corners[k] = (bad, corners[k][1]) if k % 2 else (corners[k][0], bad)
                expect(f"corner {k} = {bad}", call(corners=corners), ERR_INVALID)
        expect("a quad the reference returns None for", call(corners=GC.none_quad(W, H)), ERR_INVALID)
        if dev:
            expect("n_layers = 0", call(n_layers=0), ERR_INVALID)
            expect("n_layers = 1025", call(n_layers=1025), ERR_INVALID)
    elif "commit" not in name:
        expect("g = NULL", call(g=None), ERR_INVALID)
        expect("lut = NULL", call(table=False), ERR_INVALID)
        for field in ("start", "end"):
            for bad in (NAN, INF, -INF):
                expect(f"{field}.x = {bad}", call(g=dict(GOOD, **{field: (bad, 1.0)})), ERR_INVALID)
                expect(f"{field}.y = {bad}", call(g=dict(GOOD, **{field: (1.0, bad)})), ERR_INVALID)
        expect("shape = 4", call(g=dict(GOOD, shape=4)), ERR_INVALID)
        expect("shape = -1", call(g=dict(GOOD, shape=-1)), ERR_INVALID)
        expect("mode = 2", call(g=dict(GOOD, mode=2)), ERR_INVALID)
        expect("preview_scale = 0", call(g=dict(GOOD, preview_scale=0)), ERR_INVALID)
        if name == "pfx_gradient_apply_dev":
            expect("preview_scale = 2", call(g=dict(GOOD, preview_scale=2)), ERR_INVALID)
    if dev:
        for b, kind in bufs:
            if kind.endswith("rgba"):
                for off in (1, 2, 3):
                    expect(f"{b} + {off}", call({b: address(b, off)}), ERR_INVALID)
    for o, kind in bufs:
        if "out" in kind:
            for b, _ in bufs:
                if b != o:
                    expect(f"{o} overlaps {b}", call({o: address(b, 16)}), ERR_INVALID)
                    expect(f"{o} is {b}", call({o: address(b)}), ERR_INVALID)
    clean = untouched()
    assert not wrong, "\n".join(wrong)
    assert clean, "a refused call wrote to a buffer"
