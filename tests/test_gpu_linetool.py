"""The line / curve tool on the device (k_linetool.hip) against the CPU model (tests/linetool_model.py), through the C ABI.  The tool is in the EXACT class:
every comparison is np.array_equal.  Each case of tests/linetool_cases.py runs with and without the selection, and each time in one call, in pieces through
pfx_int_line_piece_entries, and through host buffers.  tests/test_linetool_model_host.py holds the model to a scalar transcription of the reference and asserts
that the cases reach their branches."""
import ctypes as C

import numpy as np
import pytest

from . import linetool_cases as LC
from . import linetool_model as M
from .dev_buffers import DevBuffers, differing

pytestmark = pytest.mark.gpu

OK, ERR_INVALID = 0, -1
SMALL_PIECES = 97   # chunk-list entries per launch for every case but the piece case: tens of pieces


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


def c_tool(t):
    from paintfe_amd import line_tool
    return line_tool(t["p"], t["size"], t["color"], t["pattern"], t["cap_style"], t["end_shape"], t["arrow_side"], t["anti_alias"])


def piece_seam(gpu):
    seam = gpu._lib.pfx_int_line_piece_entries
    seam.restype, seam.argtypes = C.c_uint64, [C.c_uint64]
    return seam


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("use_sel", [False, True], ids=["no-sel", "sel"])
@pytest.mark.parametrize("name", LC.NAMES)
def test_render_equals_the_model(gpu, name, use_sel):
    c = LC.CASES[name]
    w, h, tool, last = c["w"], c["h"], c_tool(c["tool"]), LC.last_of(c)
    want, want_bounds, _ = LC.expected(name, use_sel)
    preview, sel = LC.preview_of(c), LC.selection(w, h)        # the selection is uploaded in every case, handed over only where the case runs with it
    limit = LC.PIECE_LIMIT if name == LC.PIECE_CASE else SMALL_PIECES
    seam = piece_seam(gpu)
    sel_bufs = DevBuffers(gpu, sel, lead=1)                    # a byte plane: any address
    bufs = DevBuffers(gpu, preview, preview)
    with sel_bufs as (d_sel,), bufs as (d_one, d_pieces):
        s = d_sel if use_sel else 0
        bounds = gpu.line_render_dev(tool, d_one, w, h, last, selection_ptr=s)
        assert seam(limit) == 8 << 20
        try:
            bounds_pieces = gpu.line_render_dev(tool, d_pieces, w, h, last, selection_ptr=s)
        finally:
            assert seam(0) == limit
        got, got_pieces = gpu.dev_download(d_one, preview.shape), gpu.dev_download(d_pieces, preview.shape)
        print(f"{name}: {differing(got, want)} differing pixels of {w * h} in one call, {differing(got_pieces, want)} in pieces")
        assert np.array_equal(got, want), differing(got, want)
        assert np.array_equal(got_pieces, want), differing(got_pieces, want)
        assert same_bits(bounds, want_bounds) and same_bits(bounds_pieces, want_bounds)
        assert np.array_equal(gpu.dev_download(d_sel, (h, w)), sel)                       # only read
        assert bufs.surroundings_intact() and sel_bufs.surroundings_intact()
    before = preview.copy()
    host, host_bounds = gpu.line_render(tool, preview, last, sel if use_sel else None)
    assert np.array_equal(host, want) and same_bits(host_bounds, want_bounds) and np.array_equal(preview, before)


def test_a_two_frame_drag_and_the_release_stay_on_the_device(gpu):
    """frame 2 clears with frame 1's bounds; the composite after each frame; then the release onto the layer and, in mask-edit mode, onto the conceal bytes"""
    w, h = LC.W, LC.H
    rng = np.random.default_rng(11)
    layer = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    conceal = rng.integers(0, 256, (h, w), dtype=np.uint8)
    stale = LC.seeded_preview(w, h)                                                       # what an earlier tool left in the preview: frame 1 clears it all
    want1, b1, _ = M.render(LC.DRAG[0], stale, None, None)
    want2, b2, _ = M.render(LC.DRAG[1], want1, None, b1)
    bufs = DevBuffers(gpu, layer, stale, np.zeros_like(layer))
    mask_bufs = DevBuffers(gpu, conceal, lead=3)
    with bufs as (d_layer, d_preview, d_out), mask_bufs as (d_conceal,):
        got_b1 = gpu.line_render_dev(c_tool(LC.DRAG[0]), d_preview, w, h, None)
        gpu.flatten_preview_dev([d_layer], [(0, 1.0, True, 0)], w, h, d_out, d_preview, 0)
        assert np.array_equal(gpu.dev_download(d_preview, layer.shape), want1) and same_bits(got_b1, b1)
        got_b2 = gpu.line_render_dev(c_tool(LC.DRAG[1]), d_preview, w, h, got_b1)
        gpu.flatten_preview_dev([d_layer], [(0, 1.0, True, 0)], w, h, d_out, d_preview, 0)
        got2 = gpu.dev_download(d_preview, layer.shape)
        assert np.array_equal(got2, want2), differing(got2, want2)
        assert same_bits(got_b2, b2) and not np.array_equal(want2, want1)
        frame = gpu.dev_download(d_out, layer.shape)
        gpu.flatten_dev([d_layer], [(0, 1.0, True, 0)], w, h, d_out)
        assert not np.array_equal(frame, gpu.dev_download(d_out, layer.shape))            # the last frame shows the line
        gpu.stroke_commit_mask_dev(d_conceal, d_preview, w, h, reveal=False)
        assert np.array_equal(gpu.dev_download(d_conceal, conceal.shape), M.commit_mask(conceal, want2, None, False))
        gpu.stroke_commit_dev(d_layer, d_preview, w, h)
        committed = gpu.dev_download(d_layer, layer.shape)
        assert np.array_equal(gpu.dev_download(d_preview, layer.shape), want2)
        assert bufs.surroundings_intact() and mask_bufs.surroundings_intact()
    assert np.array_equal(committed, gpu.brush_commit(layer, want2, 0)) and not np.array_equal(committed, layer)


def test_control_points_far_outside_the_canvas(gpu):
    """legal: the saturating casts and NaN rules decide what is drawn — here a curve through the canvas between far points, and an overflowing one that draws nothing"""
    w, h = LC.W, LC.H
    far = LC.tool([(-3000.0, 20.0), (-10.0, 900.0), (80.0, -700.0), (2500.0, 40.0)], 4, end_shape=1, arrow_side=2)
    huge = LC.tool([(-3e38, 20.0), (3e38, 3e38), (-3e38, -3e38), (3e38, 40.0)], 4, pattern=1, end_shape=1, arrow_side=2)
    stale = LC.seeded_preview(w, h)
    for tool, draws in ((far, True), (huge, False)):
        want, want_b, _ = M.render(tool, stale, None, None)
        bufs = DevBuffers(gpu, stale)
        with bufs as (d_pv,):
            gpu.line_render_dev(c_tool(tool), d_pv, w, h, None)
            got = gpu.dev_download(d_pv, stale.shape)
            assert bufs.surroundings_intact()
        assert np.array_equal(got, want) and bool(want.any()) == draws


@pytest.mark.parametrize("use_sel", [False, True], ids=["no-sel", "sel"])
@pytest.mark.parametrize("reveal", [False, True], ids=["conceal", "reveal"])
def test_commit_mask_equals_the_model_over_all_pairs(gpu, reveal, use_sel):
    old, pv = LC.commit_inputs()
    sel = LC.selection(256, 256)
    want = M.commit_mask(old, pv, sel if use_sel else None, reveal)
    assert not np.array_equal(want, old)
    sel_bufs = DevBuffers(gpu, sel, lead=1)
    bufs = DevBuffers(gpu, pv)
    mask_bufs = DevBuffers(gpu, old, lead=1)                                              # conceal bytes: any address
    with sel_bufs as (d_sel,), bufs as (d_pv,), mask_bufs as (d_old,):
        gpu.stroke_commit_mask_dev(d_old, d_pv, 256, 256, reveal, selection_ptr=d_sel if use_sel else 0)
        got = gpu.dev_download(d_old, old.shape)
        assert np.array_equal(got, want), int((got != want).sum())
        assert np.array_equal(gpu.dev_download(d_pv, pv.shape), pv) and np.array_equal(gpu.dev_download(d_sel, sel.shape), sel)
        assert bufs.surroundings_intact() and sel_bufs.surroundings_intact() and mask_bufs.surroundings_intact()
    before = old.copy()
    host = gpu.stroke_commit_mask(old, pv, reveal, sel if use_sel else None)
    assert np.array_equal(host, want) and np.array_equal(old, before)


@pytest.mark.parametrize("w,h", [(65, 3), (1, 1), (131, 70)])
def test_commit_mask_on_odd_sizes(gpu, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    old, pv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    pv[..., 3][rng.random((h, w)) < 0.3] = 0
    for reveal in (False, True):
        assert np.array_equal(gpu.stroke_commit_mask(old, pv, reveal), M.commit_mask(old, pv, None, reveal))


# ---- the argument contract -----------------------------------------------------------------------------------------------------------------------------------------------
W, H = 67, 5
SLOT, N_SLOTS = 4096, 4
NAN, INF = float("nan"), float("inf")
GOOD = LC.tool([(2.0, 1.0), (20.0, 4.0), (40.0, 0.5), (64.0, 3.0)], 3.0, LC.GREEN, 2, 0, 1, 2, True)
# entry point -> its buffers in call order: name, kind (in / out / opt = an optional input; rgba or mask)
CONTRACT = {
    "pfx_line_render_dev": [("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_line_render": [("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_stroke_commit_mask_dev": [("conceal", "out:mask"), ("preview", "in:rgba"), ("sel", "opt:mask")],
    "pfx_stroke_commit_mask": [("conceal", "out:mask"), ("preview", "in:rgba"), ("sel", "opt:mask")],
}


@pytest.fixture(scope="module")
def arena(gpu):
    rng = np.random.default_rng(29)
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
    is_render = "render" in name

    def restore():
        arena["host"][:] = arena["pattern"]
        gpu.dev_upload(arena["dev"], arena["pattern"])
        gpu.synchronize()

    def untouched():
        gpu.synchronize()
        return np.array_equal(gpu.dev_download(arena["dev"], arena["pattern"].shape), arena["pattern"]) and np.array_equal(arena["host"], arena["pattern"])

    def call(ptrs=None, tool="good", dims=(W, H), last=(0.0, 0.0, 67.0, 5.0), want_bounds=True):
        """ptrs: buffer name -> address (None = NULL); tool None = a NULL descriptor, a dict, or a ready struct; last None = NULL"""
        p = {b: address(b) for b, _ in bufs}
        p.update(ptrs or {})
        a = {b: C.c_void_p(p[b]) for b, _ in bufs}
        w, h = C.c_uint32(dims[0]), C.c_uint32(dims[1])
        if not is_render:
            return fn(gpu.handle, a["conceal"], a["preview"], a["sel"], w, h, C.c_int(0)), None
        t = GOOD if isinstance(tool, str) else tool
        d = None if t is None else C.byref(c_tool(t) if isinstance(t, dict) else t)
        lb = None if last is None else (C.c_float * 4)(*last)
        out = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0) if want_bounds else None
        return fn(gpu.handle, d, a["preview"], a["sel"], w, h, lb, out), out

    wrong = []

    def expect(what, result, want):
        if result[0] != want:
            wrong.append(f"{what}: {result[0]}, expected {want}")
        elif want != OK and result[1] is not None and tuple(result[1]) != (7.0, 7.0, 7.0, 7.0):
            wrong.append(f"{what}: refused, but bounds_out was written")

    restore()
    expect("the valid call", call(), OK)
    expect("the valid call without sel", call({"sel": None}), OK)
    if is_render:
        expect("the valid call without bounds_out", call(want_bounds=False), OK)
        expect("the valid call without last_bounds", call(last=None), OK)
        expect("a negative size", call(tool=dict(GOOD, size=-3.0)), OK)                   # any finite size, as the clone stamp takes it
    restore()
    # ---- refusals ----
    for b, kind in bufs:
        if not kind.startswith("opt"):
            expect(f"{b} = NULL", call({b: None}), ERR_INVALID)
    expect("20000 x 20000", call(dims=(20000, 20000)), ERR_INVALID)
    expect("w = 0", call(dims=(0, H)), ERR_INVALID)
    expect("h = 0", call(dims=(W, 0)), ERR_INVALID)
    if is_render:
        expect("tool = NULL", call(tool=None), ERR_INVALID)
        for bad in (NAN, INF, -INF):
            expect(f"size = {bad}", call(tool=dict(GOOD, size=bad)), ERR_INVALID)
            for k in range(4):
                for axis in (0, 1):
                    pts = [list(q) for q in GOOD["p"]]
                    pts[k][axis] = bad
                    expect(f"p{k}[{axis}] = {bad}", call(tool=dict(GOOD, p=pts)), ERR_INVALID)
                lb = [0.0, 0.0, 67.0, 5.0]
                lb[k] = bad
                expect(f"last_bounds[{k}] = {bad}", call(last=lb), ERR_INVALID)
        for field, values in (("pattern", (-1, 3)), ("cap_style", (-1, 2)), ("end_shape", (-1, 2)), ("arrow_side", (-1, 3))):
            for bad in values:
                t = c_tool(GOOD)
                setattr(t, field, bad)
                expect(f"{field} = {bad}", call(tool=t), ERR_INVALID)
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
                    expect(f"{o} is {b}", call({o: address(b)}), ERR_INVALID)     # in place is refused: the preview is only read
    clean = untouched()
    assert not wrong, "\n".join(wrong)
    assert clean, "a refused call wrote to a buffer"
