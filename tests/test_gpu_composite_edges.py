"""Parity (GPU): the compositor's document path at its edges — tests/composite_cases.py, every case against the CPU oracle at tolerance 0, through the layer
store (pfx_layer_* + pfx_composite / _preview / _region) and through the device entry points (pfx_flatten_dev, pfx_flatten_preview_dev,
pfx_int_flatten_with_chunk_keys_dev).  What the table reaches is shown on the host by tests/test_composite_cases_host.py.

Every composite also asserts the launch path it was written for through pfx_int_flatten_last_path (pfx_internal.h): live masks, adjustment layers, previews
and rectangles flatten_kernel<true, F>, the zero-opacity twins of group B flatten_kernel<true, false>, the odd opacities of group F flatten_kernel<false, false>,
and the editing sessions of group G all four kernels and the per-chunk start table with its verdict pending and decided.  Refused rectangles raise PfxError and leave
the destination as it was.  A stack's images are uploaded once; the cases change descriptors.

No disagreement with the oracle was found, so no fix is recorded here; three arithmetic-only mutants of k_flatten.hip (adjust_px without its opacity clamp,
preview_apply's lerp without + 0.5, chunk activity from the whole pixel word) each fail this file (profiles/composite_edges.md).

Wall time on an MI355X: the whole file 1.9 s (4 300 composites); the slowest test is the preview on 130 x 70 (738 cases) at 0.31 s, then the raster-only stacks
on 67 x 66 (243 cases) 0.11 s, an editing session 0.09 s, the conceal lattice (46 composites of 256 x 256) 0.06 s.
"""
import ctypes as C
import time

import numpy as np
import pytest

from . import composite_cases as CC
from . import oracle_lib as O
from .dev_buffers import SENTINEL, TAIL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    r = GpuRenderer(0)
    r._lib.pfx_int_flatten_last_path.argtypes = [C.c_void_p]
    r._lib.pfx_int_flatten_last_path.restype = C.c_int
    yield r
    r.tune("dle_kernel", 0)


@pytest.fixture(autouse=True)
def stop_after_a_device_error(gpu):
    """a HIP error behind a test ends the session: nothing more is launched on a device that has reported one"""
    yield
    from paintfe_amd import PfxError
    try:
        gpu.synchronize()
    except PfxError as e:
        pytest.exit(f"the device reported an error after this test: {e}", returncode=3)


def last_path(r):
    return int(r._lib.pfx_int_flatten_last_path(r._h))


def infos(layers):
    """GpuRenderer._infos tuples; a raster layer's store index is its position in the stack"""
    return [(i, L.get("opacity", 1.0), L.get("visible", True), L.get("mode", 0), L.get("kind", 0), tuple(L.get("adj", ()))) for i, L in enumerate(layers)]


class Wants:
    """the oracle's image of a case; cases that differ only in route or rectangle share it"""

    def __init__(self):
        self.full = {}

    def __call__(self, case):
        key = (id(case.layers), id(case.preview), id(case.keys))
        if key not in self.full:
            self.full[key] = CC.Case(case.name, case.w, case.h, case.layers, preview=case.preview, keys=case.keys).want(O.composite)
        if case.rect is None:
            return self.full[key]
        x, y, rw, rh = case.rect
        return self.full[key][y:y + rh, x:x + rw]


class Device:
    """runs cases; keeps what it uploaded (by array identity) until the canvas size changes"""

    def __init__(self, r):
        self.r, self.size, self.resident, self.generation, self.ptrs, self.dst = r, None, {}, 0, {}, 0

    def canvas(self, w, h):
        if self.size == (w, h):
            return
        self.release()
        self.size = (w, h)
        self.r.clear_layers()
        self.dst = self.r.dev_alloc(w * h * 4 + TAIL)
        self.r.dev_upload(self.dst, np.full(w * h * 4 + TAIL, SENTINEL, np.uint8))

    def release(self):
        if self.size is None:
            return
        w, h = self.size
        tail = self.r.dev_download(self.dst + w * h * 4, (TAIL,))
        for p, _ in self.ptrs.values():
            self.r.dev_free(p)
        self.r.dev_free(self.dst)
        self.ptrs, self.resident, self.size = {}, {}, None
        assert (tail == SENTINEL).all(), f"{w}x{h}: a composite wrote behind its destination"

    def ptr(self, array):
        if id(array) not in self.ptrs:
            a = np.ascontiguousarray(array, np.uint8)
            p = self.r.dev_alloc(a.nbytes)
            self.r.dev_upload(p, a)
            self.ptrs[id(array)] = (p, array)   # the array is kept, so its id stays its own
        return self.ptrs[id(array)][0]

    def sync_store(self, layers):
        for i, L in enumerate(layers):
            if CC.is_adj(L) or L.get("pixels") is None:
                continue
            held = self.resident.get(i) or [None, None]
            if held[0] is not L["pixels"]:
                self.generation += 1
                self.r.ensure_layer_texture(i, L["pixels"], self.generation)   # a same-size upload keeps the layer's mask
                held[0] = L["pixels"]
            if held[1] is not L.get("mask"):
                self.r.set_layer_mask(i, L.get("mask"))                         # None: cleared with NULL
                held[1] = L.get("mask")
            self.resident[i] = held

    def run(self, case):
        r, w, h, pv = self.r, case.w, case.h, case.preview
        self.canvas(w, h)
        info = infos(case.layers)
        if case.route == CC.STORE:
            self.sync_store(case.layers)
            if pv is not None:
                return r.composite_preview(w, h, info, pv["pixels"], pv["active_layer"], pv.get("blend_mode", 0), pv.get("is_eraser", False),
                                           pv.get("replaces_layer", False), pv.get("chunk_present"))
            if case.rect is not None:
                return r.composite_dirty_readback(w, h, info, case.rect)
            return r.composite(w, h, info)
        ptrs = [0 if CC.is_adj(L) else self.ptr(L["pixels"]) for L in case.layers]
        masks = [self.ptr(L["mask"]) if L.get("mask") is not None else 0 for L in case.layers]
        if case.route == CC.KEYS:
            arr, n = r._infos(info)
            lp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in ptrs])
            keys = np.ascontiguousarray(case.keys, np.uint8)
            r._check(r._lib.pfx_int_flatten_with_chunk_keys_dev(r._h, lp, arr, C.c_uint32(n), C.c_uint32(w), C.c_uint32(h), C.c_void_p(self.dst), keys.ctypes.data_as(C.c_void_p)))
        elif pv is not None:
            cp = pv.get("chunk_present")
            r.flatten_preview_dev(ptrs, info, w, h, self.dst, self.ptr(pv["pixels"]), pv["active_layer"], pv.get("blend_mode", 0), pv.get("is_eraser", False),
                                  pv.get("replaces_layer", False), chunk_present_ptr=0 if cp is None else self.ptr(cp), mask_ptrs=masks if any(masks) else None)
        else:
            r.flatten_dev(ptrs, info, w, h, self.dst, mask_ptrs=masks if any(masks) else None)
        return r.dev_download(self.dst, (h, w, 4))


def differs(name, got, want):
    bad = (got != want).any(-1)
    if not bad.any():
        return None
    y, x = np.argwhere(bad)[0]
    return f"{name}: {int(bad.sum())} of {bad.size} px differ, first at ({int(x)}, {int(y)}): got {got[y, x].tolist()} want {want[y, x].tolist()}"


def wrong_path(case, path):
    value, mask = case.path()
    if (path & mask) != value or (mask == 0xF0 and (path & 0xF) == CC.K_TEMPLATE):
        return f"{case.name}: launch path {path:#x}, expected {value:#x} under mask {mask:#x}" + (" and a fast kernel" if mask == 0xF0 else "")
    return None


def refused(r, case, failures):
    from paintfe_amd import PfxError
    x, y, rw, rh = case.rect
    dst = np.full(4096, SENTINEL, np.uint8)
    arr, n = r._infos(infos(case.layers))
    before = last_path(r)
    with pytest.raises(PfxError):
        r._check(r._lib.pfx_composite_region(r._h, C.c_uint32(case.w), C.c_uint32(case.h), arr, C.c_uint32(n), C.c_uint32(x), C.c_uint32(y), C.c_uint32(rw),
                                             C.c_uint32(rh), dst.ctypes.data_as(C.c_void_p)))
    if not (dst == SENTINEL).all():
        failures.append(f"{case.name}: a refused call wrote to dst")
    if last_path(r) != before:
        failures.append(f"{case.name}: a refused call launched")


def run_cases(r, cases, what):
    t0 = time.perf_counter()
    dev, wants, failures, paths = Device(r), Wants(), [], set()
    try:
        for case in cases:
            if case.expect == CC.STATUS:
                dev.canvas(case.w, case.h)
                dev.sync_store(case.layers)
                refused(r, case, failures)
                continue
            got = dev.run(case)
            path = last_path(r)
            paths.add(path & 0xFF)
            for f in (differs(case.name, got, wants(case)), wrong_path(case, path)):
                if f:
                    failures.append(f"{case.w}x{case.h} {f}")
    finally:
        dev.release()
    print(f"{what}: {len(cases)} cases, {time.perf_counter() - t0:.2f} s, paths {sorted(hex(p) for p in paths)}")
    assert not failures, f"{what}: {len(failures)} failures\n" + "\n".join(failures[:12])
    return paths


GENERAL_FAST, GENERAL_SLOW = CC.K_TEMPLATE | CC.P_GENERAL | CC.P_FAST, CC.K_TEMPLATE | CC.P_GENERAL


def test_the_seam_reads_minus_one_before_the_first_composite():
    from paintfe_amd import GpuRenderer
    r = GpuRenderer(0)
    try:
        assert last_path(r) == -1
        r.ensure_layer_texture(0, CC.rgba(5, 3, 1), 1)
        r.composite_dirty_readback(5, 3, [(0, 0.0, True, 0)], (1, 1, 2, 1))
        assert last_path(r) == CC.K_TEMPLATE | CC.P_GENERAL | CC.P_REGION      # opacity 0: flatten_kernel<true, false> on a rectangle
        r.composite(5, 3, [(0, 1.0, True, 0)])
        assert last_path(r) & 0xFF == CC.K_STREAM | CC.P_FAST
    finally:
        r.close()


def test_a_conceal_lattice(gpu):
    """every (alpha, conceal) pair under six layer descriptors over three bases, both routes; masks on the bottom, on two, on a hidden layer, an all-255 mask,
    and a mask set and then cleared with NULL"""
    paths = run_cases(gpu, CC.group_a(), "A conceal lattice")
    assert GENERAL_FAST in paths and any(p & 0xF for p in paths)   # the cleared and the hidden mask are back on a fast kernel


@pytest.mark.parametrize("part", ["exposure", "brightness", "mixer", "opacity"])
def test_b_adjustment_rows(gpu, part):
    """every parameter edge in [source, row, raster, Exposure at 0.3], and again with that last opacity at 0: flatten_kernel<true, false>"""
    pick = {"exposure": "exposure ev", "brightness": "brightness ", "mixer": "mixer ", "opacity": " at opacity "}[part]
    cases = [c for row, a, b in CC.group_b_rows() if pick in row.name for c in (a, b)]
    assert cases
    paths = run_cases(gpu, cases, f"B rows {part}")
    assert {GENERAL_FAST, GENERAL_SLOW} <= paths


def test_b_adjustment_positions(gpu):
    paths = run_cases(gpu, CC.group_b_positions(), "B positions")
    assert {GENERAL_FAST, GENERAL_SLOW} <= paths


def test_b_every_mode_above_a_mixer_that_rewrote_alpha(gpu):
    paths = run_cases(gpu, CC.group_b_modes(), "B modes")
    assert paths == {GENERAL_FAST, GENERAL_SLOW}


def test_b_compound_stack_on_every_canvas(gpu):
    paths = run_cases(gpu, CC.group_b_canvases(), "B canvases")
    assert paths == {GENERAL_FAST, GENERAL_SLOW}


@pytest.mark.parametrize("size", CC.C_CANVASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_c_chunk_activity(gpu, size):
    """chunks populated by a visible, a hidden, a fully concealed layer, by coloured pixels of alpha 0, by the preview alone, by caller-supplied keys: an
    inactive chunk stays (0, 0, 0, 0) under an Invert and a mixer, also inside a quad whose other pixels are active"""
    paths = run_cases(gpu, [c for c in CC.group_c() if (c.w, c.h) == size], f"C {size}")
    assert GENERAL_FAST in paths and GENERAL_FAST | CC.P_PREVIEW in paths


@pytest.mark.parametrize("size", CC.D_CANVASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_d_preview(gpu, size):
    paths = run_cases(gpu, CC.group_d(*size), f"D {size}")
    assert paths == {GENERAL_FAST | CC.P_PREVIEW}


@pytest.mark.parametrize("size", CC.E_CANVASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_e_dirty_rectangles(gpu, size):
    paths = run_cases(gpu, CC.group_e(*size), f"E {size}")
    assert paths == {GENERAL_FAST | CC.P_REGION}


@pytest.mark.parametrize("size", CC.F_CANVASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_f_raster_only_off_the_fast_path(gpu, size):
    """NaN, negative, zero, denormal and sub-threshold opacities: flatten_kernel<false, false>; 2^-40 itself and +inf stay on a fast kernel"""
    paths = run_cases(gpu, CC.group_f(*size), f"F {size}")
    assert CC.K_TEMPLATE in paths and all(p == CC.K_TEMPLATE or (p & 0xF and p & CC.P_FAST) for p in paths)


# ---- G: the editing session ------------------------------------------------------------------------------------------------------------------------------------------
def start_table(layers):
    """pfx_flatten.cpp: build_stack's chunk_meta and chunk_start_kernel on the mirror: (some layer above the bottom one may reset a chunk, some chunk does start above
    layer 0).  Normal at opacity >= 1 resets a chunk whose alpha is all 255, Overwrite one without an alpha 0; masked layers never"""
    desc = [L for L in layers if L.get("visible", True) and L.get("pixels") is not None]
    wanted = useful = False
    for L in desc[1:]:
        mode = 0 if L["mode"] > 24 else L["mode"]
        if L.get("mask") is not None or not (mode == CC.OVERWRITE or (mode == CC.NORMAL and L["opacity"] >= 1.0)):
            continue
        wanted = True
        h, w = L["pixels"].shape[:2]
        a, chunks = L["pixels"][..., 3].ravel(), CC.chunk_of_pixels(w, h).ravel()
        hit = np.ones(chunks.max() + 1, bool)
        np.logical_and.at(hit, chunks, (a != 0) if mode == CC.OVERWRITE else (a == 255))
        useful = useful or bool(hit.any())
    return len(desc), wanted, useful


STORE_STEPS = ("upload", "open_hole", "close_hole", "set_mask", "clear_mask", "remove_layer")   # they move the store's epoch (pfx_ctx.cpp); a same-generation upload does not


def apply_step(r, s):
    k = s["kind"]
    if k in ("upload", "upload_same_generation"):
        r.ensure_layer_texture(s["idx"], s["pixels"], s["generation"])
    elif k in ("open_hole", "close_hole"):
        r.update_layer_rect(s["idx"], s["x"], s["y"], s["pixels"])
    elif k in ("set_mask", "clear_mask"):
        r.set_layer_mask(s["idx"], s["mask"])
    elif k == "remove_layer":
        r.remove_layer(s["idx"])
    # every other state step changes descriptors only: the next composite's layer_info carries it


@pytest.mark.parametrize("seed", CC.SESSION_SEEDS)
def test_g_editing_session(gpu, seed):
    """an editing session of 6 stored layers and one of 18 (deep enough for the elimination kernels), compared after every composite.  For raster-only stacks on
    the fast path the kernel follows from the mirror: 16 layers and a reset candidate the class-sorting kernel (the elimination kernel under pfx_tune
    "dle_kernel" 1), otherwise the streaming kernel — with the per-chunk start table while its verdict is pending, and after the repeated composite exactly when
    the mirror says the table skips something"""
    r, failures, seen, table = gpu, [], set(), set()
    t0 = time.perf_counter()
    for n_layers in (6, 18):
        steps, doc = CC.session(seed, n_layers)
        r.clear_layers()
        store_moved = True
        for i, s in enumerate(steps):
            if s["kind"] not in CC.COMPOSITE_STEPS:
                apply_step(r, s)
                store_moved = store_moved or s["kind"] in STORE_STEPS
                continue
            case = CC.Case(f"seed {seed}, {n_layers} layers, step {i} {s['kind']}", doc.w, doc.h, s["layers"], preview=s.get("preview"), rect=s.get("rect"))
            pv = case.preview

            def composite():
                if pv is not None:
                    return r.composite_preview(doc.w, doc.h, s["info"], pv["pixels"], pv["active_layer"], pv["blend_mode"], pv["is_eraser"], pv["replaces_layer"])
                return r.composite_dirty_readback(doc.w, doc.h, s["info"], case.rect) if case.rect else r.composite(doc.w, doc.h, s["info"])

            want = case.want(O.composite)
            got, path = composite(), last_path(r)
            seen.add(path & 0xF)
            failures += [f for f in (differs(case.name, got, want), wrong_path(case, path)) if f]
            if not case.fast_kernel():
                continue
            n_desc, wanted, useful = start_table(s["layers"])
            deep = n_desc >= 16 and wanted
            if (path & 0xF) != (CC.K_SRT if deep else CC.K_STREAM):
                failures.append(f"{case.name}: kernel {path & 0xF} for {n_desc} layers, reset candidate {wanted}")
            if deep:   # the same stack through the elimination kernel
                r.tune("dle_kernel", 1)
                try:
                    got, path2 = composite(), last_path(r)
                finally:
                    r.tune("dle_kernel", 0)
                seen.add(path2 & 0xF)
                failures += [f for f in (differs(case.name + " (elimination kernel)", got, want),) if f]
                if (path2 & 0xF) != CC.K_DLE:
                    failures.append(f"{case.name}: kernel {path2 & 0xF} under dle_kernel 1")
                continue
            used = bool(path & CC.P_CHUNK_START)
            if wanted and store_moved:             # the store's epoch has moved since the last table: this composite builds one and runs with it, verdict pending
                table.add("pending")
                if not used:
                    failures.append(f"{case.name}: a freshly built start table was not used")
            elif s["kind"] == "composite_repeat":  # the composite before it has synchronised: the verdict is in
                table.add("useful" if used else "useless" if wanted else "none")
                if used != useful:
                    failures.append(f"{case.name}: start table used {used}, the mirror says useful {useful}")
            if used and not wanted or (useful and not used):
                failures.append(f"{case.name}: start table used {used}, wanted {wanted}, useful {useful}")
            store_moved = store_moved and not wanted
    print(f"G seed {seed}: {time.perf_counter() - t0:.2f} s, kernels {sorted(seen)}, start table {sorted(table)}")
    assert not failures, f"{len(failures)} failures\n" + "\n".join(failures[:12])
    assert seen == {CC.K_TEMPLATE, CC.K_STREAM, CC.K_DLE, CC.K_SRT}
    assert {"pending", "useful"} <= table, table   # the table in its pending and its decided state
