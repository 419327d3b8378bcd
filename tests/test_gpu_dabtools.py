"""The clone stamp, the heal brush's live stroke and the pencil on the device (k_dabtools.hip) against the CPU model (tests/dabtools_model.py), through the C ABI.
Clone and pencil are in the EXACT class: every comparison is np.array_equal.  The heal ring evaluates cos / sin as the f64 routine rounded once, so it is
compared exactly with the model's `device` flavour at every pixel that is not fragile, in alpha alone at fragile pixels, and not at all at fragile pixels
with fewer than two in-canvas samples (where `count < 1` itself may flip).  tests/test_dabtools_model_host.py holds the model to a scalar transcription, asserts
that the cases reach their branches, and caps the fragile pixels of the cases built for the cap."""
import ctypes as C

import numpy as np
import pytest

from . import dabtools_cases as DC
from . import dabtools_model as M
from .dev_buffers import DevBuffers, differing

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


def clone_tool(t):
    from paintfe_amd import clone_stamp_tool
    return clone_stamp_tool(t["size"], t["hardness"], t["anti_aliased"], t["offset"])


def heal_tool(t):
    from paintfe_amd import heal_ring_tool
    return heal_ring_tool(t["size"], t["hardness"], t["sample_radius"])


def no_selection(w, h):
    return np.full((h, w), 255, np.uint8)       # uploaded in every case, handed over only where the case has a selection


def run_stroke(gpu, case, dev_call, host_call, source, preview, check):
    """the stroke in one call, one call per piece onto a second copy of the preview, and through host buffers; `check(got, dirty)` compares with the model"""
    w, h, sel = case["w"], case["h"], DC.selection_of(case)
    pieces = DC.segments_of(case)
    pts = np.concatenate(pieces)
    sel_bufs = DevBuffers(gpu, no_selection(w, h) if sel is None else sel, lead=1)      # a byte plane: any address
    bufs = DevBuffers(gpu, source, preview, preview)
    with sel_bufs as (d_sel,), bufs as (d_src, d_one, d_pieces):
        s = 0 if sel is None else d_sel
        dirty = dev_call(d_src, d_one, w, h, pts, s)
        boxes = [dev_call(d_src, d_pieces, w, h, p, s) for p in pieces]
        got, got_pieces = gpu.dev_download(d_one, preview.shape), gpu.dev_download(d_pieces, preview.shape)
        assert np.array_equal(got, got_pieces), differing(got, got_pieces)              # a stroke split over calls gives the same bytes
        assert dirty == (min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes))
        check(got, dirty)
        assert np.array_equal(gpu.dev_download(d_src, source.shape), source)            # only read
        assert np.array_equal(gpu.dev_download(d_sel, (h, w)), no_selection(w, h) if sel is None else sel)
        assert bufs.surroundings_intact() and sel_bufs.surroundings_intact()
    before = preview.copy()
    host, host_dirty = host_call(source, preview, pts, sel)
    assert np.array_equal(host, got) and host_dirty == dirty and np.array_equal(preview, before)


@pytest.mark.parametrize("name", DC.CLONE_NAMES)
def test_clone_equals_the_model(gpu, name):
    c = DC.CLONE[name]
    want, want_dirty, _ = DC.clone_expected(name)
    tool = clone_tool(c["tool"])

    def check(got, dirty):
        print(f"{name}: {differing(got, want)} differing pixels of {c['w'] * c['h']}")
        assert np.array_equal(got, want), differing(got, want)
        assert dirty == want_dirty

    run_stroke(gpu, c, lambda s, p, w, h, pts, sel: gpu.clone_stamp_dev(tool, s, p, w, h, pts, selection_ptr=sel),
               lambda s, p, pts, sel: gpu.clone_stamp(tool, s, p, pts, selection=sel), DC.source(c["w"], c["h"]), DC.clone_preview(name), check)


@pytest.mark.parametrize("name", DC.HEAL_NAMES)
def test_heal_equals_the_model_where_no_sample_can_move(gpu, name):
    c = DC.HEAL[name]
    want, want_dirty, stats, fragile, count = DC.heal_expected(name, "device")
    tool = heal_tool(c["tool"])

    def check(got, dirty):
        solid = ~fragile
        alpha_only = fragile & (count >= 2)
        left_out = fragile & (count < 2)
        touched = stats["covered"] if stats["covered"] is not None else np.zeros(fragile.shape, bool)
        print(f"{name}: zone {c['zone']}; of {int(touched.sum())} covered pixels {int((alpha_only & touched).sum())} fragile ones compared in alpha alone, "
              f"{int((left_out & touched).sum())} left out; colour differs at {differing(got[alpha_only], want[alpha_only])} fragile pixels")
        assert np.array_equal(got[solid], want[solid]), differing(got[solid], want[solid])
        assert np.array_equal(got[alpha_only][:, 3], want[alpha_only][:, 3])
        assert dirty == want_dirty

    run_stroke(gpu, c, lambda s, p, w, h, pts, sel: gpu.heal_ring_dev(tool, s, p, w, h, pts, selection_ptr=sel),
               lambda s, p, pts, sel: gpu.heal_ring(tool, s, p, pts, selection=sel), DC.source(c["w"], c["h"]), DC.heal_preview(name), check)


@pytest.mark.parametrize("limit", [1, 7, 40])
@pytest.mark.parametrize("tool", ["clone", "heal"])
def test_a_stroke_sent_in_pieces_gives_the_same_bytes(gpu, tool, limit):
    """a stroke whose chunk lists pass the per-launch limit (8 Mi entries) goes to the device in consecutive pieces; the limit lowered to 1, 7 and 40 entries
    cuts the stroke into many (a size-41 dab alone touches up to six chunks of 131 x 70: a piece holds at least one dab)"""
    name = "131x70-size41-hard0.0-aa-off17.5,-9.5-sel-seeded" if tool == "clone" else "131x70-full-size41-hard0.5-ring30.0-sel-seeded"
    c = (DC.CLONE if tool == "clone" else DC.HEAL)[name]
    w, h, sel, pts = c["w"], c["h"], DC.selection_of(c), DC.points_of(c)
    preview = DC.clone_preview(name) if tool == "clone" else DC.heal_preview(name)
    t = clone_tool(c["tool"]) if tool == "clone" else heal_tool(c["tool"])
    call = gpu.clone_stamp_dev if tool == "clone" else gpu.heal_ring_dev
    seam = gpu._lib.pfx_int_dab_piece_entries
    seam.restype, seam.argtypes = C.c_uint64, [C.c_uint64]
    bufs = DevBuffers(gpu, DC.source(w, h), preview, preview, sel)
    with bufs as (d_src, d_whole, d_cut, d_sel):
        whole_box = call(t, d_src, d_whole, w, h, pts, selection_ptr=d_sel)
        assert seam(limit) == 8 << 20
        try:
            cut_box = call(t, d_src, d_cut, w, h, pts, selection_ptr=d_sel)
        finally:
            assert seam(0) == limit
        whole, cut = gpu.dev_download(d_whole, preview.shape), gpu.dev_download(d_cut, preview.shape)
        assert bufs.surroundings_intact()
    assert np.array_equal(whole, cut), differing(whole, cut)
    assert whole_box == cut_box and not np.array_equal(whole, preview)


@pytest.mark.parametrize("name", DC.PENCIL_NAMES)
def test_pencil_equals_the_model(gpu, name):
    c = DC.PENCIL[name]
    w, h, sel = c["w"], c["h"], DC.selection_of(c)
    want, want_dirty, _ = DC.pencil_expected(name)
    lists = DC.pencil_cell_lists(w, h)
    cells, preview = np.concatenate(lists), DC.pencil_preview(w, h)
    sel_bufs = DevBuffers(gpu, no_selection(w, h) if sel is None else sel, lead=1)
    bufs = DevBuffers(gpu, preview, preview)
    with sel_bufs as (d_sel,), bufs as (d_one, d_pieces):
        s = 0 if sel is None else d_sel
        dirty = gpu.pencil_dev(c["color"], d_one, w, h, cells, selection_ptr=s)
        for piece in lists:
            gpu.pencil_dev(c["color"], d_pieces, w, h, piece, selection_ptr=s)
        got, got_pieces = gpu.dev_download(d_one, preview.shape), gpu.dev_download(d_pieces, preview.shape)
        assert np.array_equal(got, want), differing(got, want)
        assert np.array_equal(got_pieces, want)
        assert dirty == M.cells_box(cells, w, h)                   # the listed in-canvas cells, the selection not consulted ...
        if sel is None:
            assert dirty == want_dirty                             # ... which is the reference's box where nothing is masked
        else:
            assert dirty[0] <= want_dirty[0] and dirty[1] <= want_dirty[1] and (want_dirty == (0, 0, 0, 0) or (dirty[2] >= want_dirty[2] and dirty[3] >= want_dirty[3]))
        assert bufs.surroundings_intact() and sel_bufs.surroundings_intact()
    host, host_dirty = gpu.pencil(c["color"], preview, cells, selection=sel)
    assert np.array_equal(host, want) and host_dirty == dirty


def test_pencil_skips_cells_outside_the_canvas(gpu):
    """the helper lists in-canvas cells only; a caller's own list may hold anything"""
    w, h = 65, 3
    preview = DC.pencil_preview(w, h)
    cells = np.array([(-1, 0), (0, -1), (65, 1), (3, 3), (2147483647, 1), (-2147483648, -2147483648), (64, 2), (0, 0)], np.int32)
    want, _ = M.pencil_cells((1.0, 1.0, 1.0, 1.0), preview, None, cells)
    bufs = DevBuffers(gpu, preview)
    with bufs as (d_pv,):
        assert gpu.pencil_dev((1.0, 1.0, 1.0, 1.0), d_pv, w, h, cells) == (0, 0, 65, 3)
        got = gpu.dev_download(d_pv, preview.shape)
        assert bufs.surroundings_intact()
    assert np.array_equal(got, want) and differing(got, preview) == 2


@pytest.mark.parametrize("is_eraser", [False, True], ids=["paint", "eraser"])
@pytest.mark.parametrize("mode", [0, 3], ids=["normal", "mode3"])
@pytest.mark.parametrize("w,h", [(131, 70), (65, 1), (1, 1)])
def test_stroke_commit_on_the_device_equals_brush_commit(gpu, w, h, mode, is_eraser):
    layer, sel = DC.source(w, h, seed=5), DC.selection(w, h)
    preview = DC.seeded_preview(w, h, DC.source(w, h, seed=6)[..., 3])
    preview[..., 3][::2, ::3] = 0
    for selection in (None, sel):
        want = gpu.brush_commit(layer, preview, mode, is_eraser=is_eraser, selection=selection)
        assert w * h == 1 or not np.array_equal(want, layer)
        sel_bufs = DevBuffers(gpu, sel, lead=1)
        bufs = DevBuffers(gpu, layer, preview)
        with sel_bufs as (d_sel,), bufs as (d_layer, d_preview):
            gpu.stroke_commit_dev(d_layer, d_preview, w, h, mode, is_eraser, selection_ptr=0 if selection is None else d_sel)
            got = gpu.dev_download(d_layer, layer.shape)
            assert np.array_equal(got, want), differing(got, want)
            assert np.array_equal(gpu.dev_download(d_preview, preview.shape), preview)
            assert bufs.surroundings_intact() and sel_bufs.surroundings_intact()


def test_a_drag_frame_and_the_release_stay_on_the_device(gpu):
    """frame by frame onto the resident preview, the composite after each frame, then the release: the sequence INTEGRATION.md gives"""
    w, h = DC.BIG
    layer = DC.source(w, h)
    tool = dict(size=7, hardness=0.5, anti_aliased=True, offset=(17.5, -9.5))
    pieces = DC.segments(w, h)
    want_preview = np.zeros((h, w, 4), np.uint8)
    bufs = DevBuffers(gpu, layer, np.zeros_like(layer), np.zeros_like(layer))
    with bufs as (d_layer, d_preview, d_out):
        for piece in pieces:
            gpu.clone_stamp_dev(clone_tool(tool), d_layer, d_preview, w, h, piece)
            gpu.flatten_preview_dev([d_layer], [(0, 1.0, True, 0)], w, h, d_out, d_preview, 0)
            want_preview, _ = M.clone_stroke(tool, layer, want_preview, None, piece)
        assert np.array_equal(gpu.dev_download(d_preview, layer.shape), want_preview)
        frame = gpu.dev_download(d_out, layer.shape)
        gpu.flatten_dev([d_layer], [(0, 1.0, True, 0)], w, h, d_out)
        without = gpu.dev_download(d_out, layer.shape)
        gpu.stroke_commit_dev(d_layer, d_preview, w, h)
        committed = gpu.dev_download(d_layer, layer.shape)
        assert bufs.surroundings_intact()
    assert np.array_equal(committed, gpu.brush_commit(layer, want_preview, 0)) and not np.array_equal(committed, layer)
    assert not np.array_equal(frame, without)                                          # the last frame shows the stroke


# ---- the argument contract -----------------------------------------------------------------------------------------------------------------------------------------------
W, H = 67, 5
SLOT, N_SLOTS = 4096, 4
NAN, INF = float("nan"), float("inf")
CLONE_GOOD = dict(size=7.0, hardness=0.5, anti_aliased=True, offset=(1.5, -0.5))
HEAL_GOOD = dict(size=7.0, hardness=0.5, sample_radius=3.0)
POINTS = np.array([(-2.0, 1.0), (3.5, 2.25), (30.0, 4.5), (66.0, 0.0)], np.float32)
CELLS = np.array([(0, 0), (5, 2), (66, 4), (70, 1)], np.int32)
# entry point -> its buffers in call order: name, kind (in / out / opt = an optional input; rgba or mask)
CONTRACT = {
    "pfx_clone_stamp_dev": [("source", "in:rgba"), ("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_clone_stamp": [("source", "in:rgba"), ("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_heal_ring_dev": [("source", "in:rgba"), ("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_heal_ring": [("source", "in:rgba"), ("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_pencil_dev": [("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_pencil": [("preview", "out:rgba"), ("sel", "opt:mask")],
    "pfx_stroke_commit_dev": [("layer", "out:rgba"), ("preview", "in:rgba"), ("sel", "opt:mask")],
}


@pytest.fixture(scope="module")
def arena(gpu):
    rng = np.random.default_rng(23)
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
    is_clone, is_heal, is_pencil, is_commit = "clone" in name, "heal" in name, "pencil" in name, "commit" in name

    def restore():
        arena["host"][:] = arena["pattern"]
        gpu.dev_upload(arena["dev"], arena["pattern"])
        gpu.synchronize()

    def untouched():
        gpu.synchronize()
        return np.array_equal(gpu.dev_download(arena["dev"], arena["pattern"].shape), arena["pattern"]) and np.array_equal(arena["host"], arena["pattern"])

    def call(ptrs=None, tool="good", dims=(W, H), items="good", n=None, color=(0.5, 0.25, 1.0, 1.0), want_dirty=True):
        """ptrs: buffer name -> address (None = NULL); tool None = a NULL descriptor, or a dict; items None = a NULL list, or an array; color None = NULL"""
        p = {b: address(b) for b, _ in bufs}
        p.update(ptrs or {})
        a = {b: C.c_void_p(p[b]) for b, _ in bufs}
        w, h = C.c_uint32(dims[0]), C.c_uint32(dims[1])
        dirty = (C.c_uint32 * 4)(7, 7, 7, 7) if want_dirty else None
        if is_commit:
            return fn(gpu.handle, a["layer"], a["preview"], a["sel"], w, h, C.c_uint8(0), C.c_int(0)), None
        if is_pencil:
            cells = CELLS if isinstance(items, str) else items
            col = None if color is None else (C.c_float * 4)(*color)
            lst = None if cells is None else np.ascontiguousarray(cells, np.int32).ctypes.data_as(C.c_void_p)
            count = (0 if cells is None else len(cells)) if n is None else n
            return fn(gpu.handle, col, a["preview"], a["sel"], w, h, lst, C.c_uint32(count), dirty), dirty
        pts = POINTS if isinstance(items, str) else items
        t = (CLONE_GOOD if is_clone else HEAL_GOOD) if isinstance(tool, str) else tool
        d = None if t is None else C.byref(clone_tool(t) if is_clone else heal_tool(t))
        lst = None if pts is None else np.ascontiguousarray(pts, np.float32).ctypes.data_as(C.c_void_p)
        count = (0 if pts is None else len(pts)) if n is None else n
        return fn(gpu.handle, d, a["source"], a["preview"], a["sel"], w, h, lst, C.c_uint32(count), dirty), dirty

    wrong = []

    def expect(what, result, want):
        if result[0] != want:
            wrong.append(f"{what}: {result[0]}, expected {want}")
        elif want != OK and result[1] is not None and tuple(result[1]) != (7, 7, 7, 7):
            wrong.append(f"{what}: refused, but dirty was written")

    restore()
    expect("the valid call", call(), OK)
    expect("the valid call without sel", call({"sel": None}), OK)
    if not is_commit:
        expect("the valid call without dirty", call(want_dirty=False), OK)
    restore()
    if not is_commit:   # nothing listed: a no-op that writes the empty box
        st, dirty = call(n=0)
        expect("n = 0", (st, None), OK)
        expect("n = 0 with a NULL list", (call(items=None, n=0)[0], None), OK)
        assert tuple(dirty) == (0, 0, 0, 0)
        assert untouched(), "a call with nothing listed wrote to a buffer"
    # ---- refusals ----
    for b, kind in bufs:
        if not kind.startswith("opt"):
            expect(f"{b} = NULL", call({b: None}), ERR_INVALID)
    expect("20000 x 20000", call(dims=(20000, 20000)), ERR_INVALID)
    expect("w = 0", call(dims=(0, H)), ERR_INVALID)
    expect("h = 0", call(dims=(W, 0)), ERR_INVALID)
    if is_clone or is_heal:
        good = CLONE_GOOD if is_clone else HEAL_GOOD
        expect("tool = NULL", call(tool=None), ERR_INVALID)
        expect("points = NULL", call(items=None, n=4), ERR_INVALID)
        fields = ["size", "hardness"] + (["offset_x", "offset_y"] if is_clone else ["sample_radius"])
        for field in fields:
            for bad in (NAN, INF, -INF):
                t = dict(good)
                if field.startswith("offset"):
                    t["offset"] = (bad, 0.0) if field == "offset_x" else (0.0, bad)
                else:
                    t[field] = bad
                expect(f"{field} = {bad}", call(tool=t), ERR_INVALID)
        for k in range(len(POINTS)):
            for bad in (NAN, INF, -INF):
                for axis in (0, 1):
                    pts = POINTS.copy()
                    pts[k, axis] = bad
                    expect(f"point {k}[{axis}] = {bad}", call(items=pts), ERR_INVALID)
    if is_pencil:
        expect("color = NULL", call(color=None), ERR_INVALID)
        expect("cells = NULL", call(items=None, n=4), ERR_INVALID)
        for k in range(4):
            for bad in (NAN, INF, -INF):
                col = [0.5, 0.25, 1.0, 1.0]
                col[k] = bad
                expect(f"color[{k}] = {bad}", call(color=col), ERR_INVALID)
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
