"""The floating selection on the device (k_overlay.hip) against the CPU model (tests/overlay_model.py).  Everything is in the EXACT class — single-rounded f32
with the host's cosf / sinf, on top of a scale step that is already bit-exact — so every comparison is np.array_equal.  tests/test_overlay_model_host.py asserts
that the cases reach every branch (fringe, general blend, the early returns, overwrite and mask-denied pixels), so nothing here passes vacuously."""
import ctypes as C

import numpy as np
import pytest

from . import overlay_cases as OC
from . import overlay_model as M
from .dev_buffers import SENTINEL, DevBuffers, differing, sentinel_like
from .test_overlay_model_host import describe

pytestmark = pytest.mark.gpu

OK, ERR_INVALID = 0, -1


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


# ---- commit --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", OC.MODES)
@pytest.mark.parametrize("aa", [True, False], ids=["aa", "no-aa"])
@pytest.mark.parametrize("name", OC.NAMES)
def test_commit_equals_the_model(gpu, name, aa, mode):
    base, src, mask = OC.inputs(name, mode)
    want, _ = OC.committed(name, aa, mode)
    got = gpu.overlay_commit(describe(OC.overlay_of(name, aa, mode)), src, base, overwrite_mask=mask)
    n = differing(got, want)
    print(f"{name} aa={aa} {mode}: {n} differing pixels")
    assert np.array_equal(got, want), n


@pytest.mark.parametrize("lead", [0, 4], ids=["aligned", "4-bytes-in"])
@pytest.mark.parametrize("name,aa,mode", [("rot-0.3", True, "overwrite-masked"), ("grow-bicubic", True, "blend"), ("off-top-left", False, "overwrite"),
                                          ("wholly-outside", True, "blend")])
def test_commit_forms_agree(gpu, name, aa, mode, lead):
    base, src, _ = OC.inputs(name, mode)
    mask = OC.overwrite_mask(src.shape[1], src.shape[0])           # uploaded in every mode, handed over in the masked one
    want, _ = OC.committed(name, aa, mode)
    ov = describe(OC.overlay_of(name, aa, mode))
    bufs = DevBuffers(gpu, src, mask, base, sentinel_like(base), lead=lead)
    with bufs as (d_src, d_mask, d_base, d_out):
        m = d_mask if mode == "overwrite-masked" else 0
        gpu.overlay_commit_dev(ov, d_src, d_base, d_out, overwrite_mask_ptr=m)                     # out of place: every byte of out is written
        assert np.array_equal(gpu.dev_download(d_out, base.shape), want)
        assert np.array_equal(gpu.dev_download(d_src, src.shape), src) and np.array_equal(gpu.dev_download(d_mask, mask.shape), mask)
        assert np.array_equal(gpu.dev_download(d_base, base.shape), base)                          # only read
        gpu.overlay_commit_dev(ov, d_src, d_base, d_base, overwrite_mask_ptr=m)                    # in place
        assert np.array_equal(gpu.dev_download(d_base, base.shape), want)
        assert bufs.surroundings_intact()


# ---- preview -------------------------------------------------------------------------------------------------------------------------------------------------------
def run_preview(gpu, ov, src):
    shape = (ov["doc_h"], ov["doc_w"], 4)
    bufs = DevBuffers(gpu, src, np.full(shape, SENTINEL, np.uint8))
    with bufs as (d_src, d_out):
        gpu.overlay_preview_dev(describe(ov), d_src, d_out)
        got = gpu.dev_download(d_out, shape)
        assert np.array_equal(gpu.dev_download(d_src, src.shape), src) and bufs.surroundings_intact()
    return got


@pytest.mark.parametrize("own_scale", [False, True], ids=["scale-1", "own-scale"])
@pytest.mark.parametrize("name", OC.NAMES)
def test_preview_equals_the_model(gpu, name, own_scale):
    ov = OC.overlay_of(name) if own_scale else OC.overlay_of(name, scale=(1.0, 1.0))
    (_, _), (sw, sh), _, _ = OC.CASES[name]
    want = OC.previewed(name, own_scale)
    got = run_preview(gpu, ov, OC.source(sw, sh))
    assert np.array_equal(got, want), differing(got, want)
    if name in ("aligned-copy", "half-pixel"):                      # the translation-only path, and it draws something
        assert ov["rotation"] == 0.0 and want.any()


def test_preview_translation_only_paths(gpu):
    src = OC.source(20, 20)
    for centre in ((-40.0, 30.0), (-10.0, 30.0), (3.5, -2.0), (125.0, 66.0), (300.0, 30.0)):      # wholly off the left edge; exactly touching it; clipped; off the right
        ov = M.overlay(20, 20, 130, 70, centre, scale=(1.0, 0.5))
        want = M.preview(ov, src)
        assert np.array_equal(run_preview(gpu, ov, src), want), centre
        if centre[0] <= -10.0 or centre[0] >= 300.0:
            assert not want.any()                                   # origin + scaled size <= 0: nothing is drawn (the reference panics below zero)


# ---- rasterize -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [True, False], ids=["aa", "no-aa"])
@pytest.mark.parametrize("name", ["rot-0.3", "off-top-left", "grow-bicubic"])
def test_rasterize_equals_the_model(gpu, name, aa):
    from paintfe_amd import overlay_geometry
    (_, _), (sw, sh), _, _ = OC.CASES[name]
    src, ov = OC.source(sw, sh), OC.overlay_of(name, aa)
    want, (col, row) = M.rasterize(ov, src)
    g = overlay_geometry(describe(ov))
    assert (g.raster_col, g.raster_row, g.raster_h, g.raster_w, 4) == (col, row) + want.shape
    bufs = DevBuffers(gpu, src, sentinel_like(want))
    with bufs as (d_src, d_out):
        assert gpu.overlay_rasterize_dev(describe(ov), d_src, d_out) is True
        got = gpu.dev_download(d_out, want.shape)
        assert np.array_equal(got, want), differing(got, want)
        assert bufs.surroundings_intact()
        gpu.dev_upload(d_src, np.zeros_like(src))                   # an all-transparent source: the reference's None
        assert gpu.overlay_rasterize_dev(describe(ov), d_src, d_out) is False


# ---- extract -------------------------------------------------------------------------------------------------------------------------------------------------------
def same_overlay(got, want):
    return ((got.source_w, got.source_h, got.doc_w, got.doc_h) == (want["source_w"], want["source_h"], want["doc_w"], want["doc_h"])
            and np.float32(got.center_x) == np.float32(want["center"][0]) and np.float32(got.center_y) == np.float32(want["center"][1])
            and (got.rotation, got.scale_x, got.scale_y, got.anchor_x, got.anchor_y) == (0.0, 1.0, 1.0, 0.0, 0.0)
            and (got.interpolation, got.anti_aliasing, got.overwrite_transparent) == (1, 1, 0))


@pytest.mark.parametrize("w,h", [(130, 70), (67, 5)])
def test_extract_with_a_selection_equals_the_model(gpu, w, h):
    layer, sel = OC.layer(w, h), OC.selection(w, h)
    sel[0, :] = 0                                                   # the box does not start at the first row
    clip, clip_mask, blanked, want_ov = M.extract(layer, sel)
    assert ((sel > 0) & (sel < 255)).any() and clip.shape[0] < h
    bufs = DevBuffers(gpu, layer, sel, sentinel_like(layer), np.full((h, w), SENTINEL, np.uint8))
    with bufs as (d_layer, d_sel, d_clip, d_cmask):
        ov = gpu.overlay_extract_dev(d_layer, d_sel, w, h, d_clip, d_cmask)
        assert ov is not None and same_overlay(ov, want_ov)
        assert np.array_equal(gpu.dev_download(d_clip, clip.shape), clip) and np.array_equal(gpu.dev_download(d_cmask, clip_mask.shape), clip_mask)
        assert (gpu.dev_download(d_clip, layer.shape).ravel()[clip.size:] == SENTINEL).all()                   # tightly packed: nothing behind the box
        assert np.array_equal(gpu.dev_download(d_layer, layer.shape), blanked) and np.array_equal(gpu.dev_download(d_sel, sel.shape), sel)
        assert bufs.surroundings_intact()


def test_extract_without_a_selection_and_the_reference_s_none(gpu):
    w, h = 130, 70
    layer = OC.layer(w, h)
    clip, _, blanked, want_ov = M.extract(layer, None)
    bufs = DevBuffers(gpu, layer, np.zeros((h, w), np.uint8), sentinel_like(layer), np.full((h, w), SENTINEL, np.uint8))
    with bufs as (d_layer, d_sel, d_clip, d_cmask):
        assert gpu.overlay_extract_dev(d_layer, d_sel, w, h, d_clip, d_cmask) is None                          # an empty selection
        clear = layer.copy()
        clear[..., 3] = 0
        gpu.dev_upload(d_layer, clear)
        assert gpu.overlay_extract_dev(d_layer, 0, w, h, d_clip, d_cmask) is None                              # no selection, nothing on the layer
        assert np.array_equal(gpu.dev_download(d_layer, layer.shape), clear)
        assert (gpu.dev_download(d_clip, layer.shape) == SENTINEL).all() and (gpu.dev_download(d_cmask, (h, w)) == SENTINEL).all()
        gpu.dev_upload(d_layer, layer)
        ov = gpu.overlay_extract_dev(d_layer, 0, w, h, d_clip, 0)                                              # no selection: the whole layer, no clip mask
        assert ov is not None and same_overlay(ov, want_ov)
        assert np.array_equal(gpu.dev_download(d_clip, layer.shape), clip) and np.array_equal(gpu.dev_download(d_layer, layer.shape), blanked)
        assert (gpu.dev_download(d_cmask, (h, w)) == SENTINEL).all() and bufs.surroundings_intact()


@pytest.mark.parametrize("w,h", [(130, 70), (67, 5)])
def test_extract_then_commit_restores_the_layer(gpu, w, h):
    """needs no model: with a 0 / 255 selection the lifted pixels go back where they were — onto alpha 0, where alpha_blend returns the source.  The returned
    descriptor has overwrite off, so commit skips samples with alpha 0 (:2130): a selected pixel that was transparent comes back as (0, 0, 0, 0), whatever colour
    it carried under its alpha 0.  The round trip is therefore exact on a layer whose transparent pixels are (0, 0, 0, 0) — what a TiledImage holds — and on any
    other layer it is exact everywhere but on those pixels, which read (0, 0, 0, 0).  Both are held here."""
    sel = OC.selection(w, h, seed=6, values=(0, 255, 255))
    coloured = OC.layer(w, h)
    clean = coloured.copy()
    clean[clean[..., 3] == 0] = 0
    lost = (sel == 255) & (coloured[..., 3] == 0)
    assert lost.sum() >= 20 and coloured[lost][:, :3].any()
    for layer in (clean, coloured):
        with DevBuffers(gpu, layer, sel, sentinel_like(layer), np.zeros((h, w), np.uint8)) as (d_layer, d_sel, d_clip, d_cmask):
            ov = gpu.overlay_extract_dev(d_layer, d_sel, w, h, d_clip, d_cmask)
            assert ov is not None and not np.array_equal(gpu.dev_download(d_layer, layer.shape), layer)
            gpu.overlay_commit_dev(ov, d_clip, d_layer, d_layer)
            back = gpu.dev_download(d_layer, layer.shape)
            if layer is clean:
                assert np.array_equal(back, layer)
            else:
                assert np.array_equal(back[~lost], layer[~lost]) and not back[lost].any()


# ---- the argument contract -----------------------------------------------------------------------------------------------------------------------------------------
W, H, SW, SH = 67, 5, 16, 4
SLOT, N_SLOTS = 4096, 8
CONTRACT_OV = M.overlay(SW, SH, W, H, (30.0, 2.5), rotation=0.3, overwrite_transparent=True)
NAN, INF = float("nan"), float("inf")
# entry point -> (its buffers in call order: name, kind; kind = rgba in / out, mask in / out, optional), the other pointer arguments
CONTRACT = {
    "pfx_overlay_commit_dev": [("source", "in:rgba"), ("mask", "opt:mask"), ("base", "in:rgba"), ("out", "out:rgba")],
    "pfx_overlay_commit": [("source", "in:rgba"), ("mask", "opt:mask"), ("base", "in:rgba"), ("out", "out:rgba")],
    "pfx_overlay_preview_dev": [("source", "in:rgba"), ("out", "out:rgba")],
    "pfx_overlay_rasterize_dev": [("source", "in:rgba"), ("out", "out:rgba")],
    "pfx_overlay_extract_dev": [("layer", "out:rgba"), ("selection", "opt:mask"), ("clip", "out:rgba"), ("clip_mask", "out:mask")],
}


@pytest.fixture(scope="module")
def arena(gpu):
    rng = np.random.default_rng(21)
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
    has = C.c_int(7)
    out_ov = describe(CONTRACT_OV)

    def restore():
        arena["host"][:] = arena["pattern"]
        gpu.dev_upload(arena["dev"], arena["pattern"])
        gpu.synchronize()

    def untouched():
        gpu.synchronize()
        return np.array_equal(gpu.dev_download(arena["dev"], arena["pattern"].shape), arena["pattern"]) and np.array_equal(arena["host"], arena["pattern"])

    def call(ptrs=None, ov=CONTRACT_OV, doc=(W, H), extra_null=False):
        """ptrs: buffer name -> address (None = NULL); ov None = a NULL descriptor; extra_null: the call's last pointer (has_pixels, the returned descriptor) NULL"""
        p = {b: address(b) for b, _ in bufs}
        p.update(ptrs or {})
        a = [C.c_void_p(p[b]) for b, _ in bufs]
        d = None if ov is None else C.byref(describe(ov))
        if name == "pfx_overlay_extract_dev":
            args = [a[0], a[1], C.c_uint32(doc[0]), C.c_uint32(doc[1]), a[2], a[3], None if extra_null else C.byref(out_ov)]
        elif name == "pfx_overlay_rasterize_dev":
            args = [d, *a, None if extra_null else C.byref(has)]
        else:
            args = [d, *a]
        return fn(gpu.handle, *args)

    wrong = []

    def expect(what, status, want):
        if status != want:
            wrong.append(f"{what}: {status}, expected {want}")

    restore()
    expect("the valid call", call(), OK)
    restore()
    # ---- refusals ----
    for b, kind in bufs:
        if not kind.startswith("opt"):
            expect(f"{b} = NULL", call({b: None}), ERR_INVALID)
    if name == "pfx_overlay_extract_dev":
        expect("out = NULL", call(extra_null=True), ERR_INVALID)
        expect("20000 x 20000", call(doc=(20000, 20000)), ERR_INVALID)
        expect("doc_w = 0", call(doc=(0, H)), ERR_INVALID)
    else:
        expect("ov = NULL", call(ov=None), ERR_INVALID)
        expect("20000 x 20000", call(ov=dict(CONTRACT_OV, doc_w=20000, doc_h=20000)), ERR_INVALID)
        for field, value in (("rotation", NAN), ("center", (INF, 2.5)), ("scale", (1.0, NAN)), ("anchor", (-INF, 0.0))):
            expect(f"{field} = {value}", call(ov=dict(CONTRACT_OV, **{field: value})), ERR_INVALID)
        expect("interpolation = 4", call(ov=dict(CONTRACT_OV, interpolation=4)), ERR_INVALID)
    if name == "pfx_overlay_rasterize_dev":
        expect("has_pixels = NULL", call(extra_null=True), ERR_INVALID)
    if dev:
        for b, kind in bufs:
            if kind.endswith("rgba"):
                for off in (1, 2, 3):
                    expect(f"{b} + {off}", call({b: address(b, off)}), ERR_INVALID)
    for o, kind in bufs:
        if kind.startswith("out"):
            for b, _ in bufs:
                if b != o:
                    expect(f"{o} overlaps {b}", call({o: address(b, 16)}), ERR_INVALID)
    clean = untouched()
    # ---- the one allowed aliasing ----
    if name.startswith("pfx_overlay_commit"):
        expect("out == base", call({"out": address("base")}), OK)
        restore()
    assert not wrong, "\n".join(wrong)
    assert clean, "a refused call wrote to a buffer"
