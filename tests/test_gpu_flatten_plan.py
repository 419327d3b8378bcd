"""Plan gate (GPU): what the compositor launched is what the pure decision says, and it composites the oracle's image.

After every composite the context's last plan (pfx_int_flatten_last_plan, pfx_internal.h) must equal pfx_int_flatten_plan of the case built HERE from the same
inputs — the stack, the canvas, the knobs this file set — and the image must equal the oracle's at tolerance 0.  The rules and the tables of the plan itself:
tests/test_flatten_dispatch_host.py.  Canvases of 67 x 66 and 257 x 130: neither pixel count is a multiple of the 4 x 64 pixels of a wave's smallest tile, both
have more than one 64 x 64 chunk per side: the smallest geometry at which a wrong grid or wave count drops or repeats pixels."""
import ctypes as C

import numpy as np
import pytest

from . import oracle_lib as O
from .test_flatten_dispatch_host import KNOBS, Cands, FlattenCase, FlattenPlan, bind

pytestmark = pytest.mark.gpu

NORMAL, OVERLAY, OVERWRITE, SOFT_LIGHT = 0, 8, 14, 16
MODE_CLASS = [2, 2, 1, 2, 0, 0, 0, 0, 1, 2, 1, 2, 2, 0, 2, 1, 0, 1, 2, 0, 2, 0, 1, 0, 1]   # pfx_flatten.cpp: build_stack (0 heavy, 1 medium, 2 light)
TEMPLATE, STREAM, DLE, SRT = range(4)
CANVASES = [(67, 66), (257, 130)]
DEPTH = 32
TUNE = dict(variant="flatten_variant", units="dle_units", cfg="dle_cfg", sched="dle_sched", fracA="dle_frac_a", fracB="dle_frac_b", kernel="dle_kernel", s1="dle_s1", s2="dle_s2",
            stats="dle_stats")


class Gpu:
    def __init__(self):
        from .backends import GpuBackend
        self.r = GpuBackend(0).r
        self.lib = bind(self.r._lib)
        self.lib.pfx_int_flatten_last_plan.argtypes = [C.c_void_p, C.POINTER(FlattenPlan)]
        self.lib.pfx_int_flatten_last_plan.restype = C.c_int
        self.unorm_ok = int(self.r.selftest_unorm_store() == 0)
        self.knobs, self.min_layers = dict(KNOBS), 16
        self.images, self.bufs = {}, {}

    def tune(self, **knobs):
        for k, v in knobs.items():
            self.r.tune(TUNE[k], v)
        self.knobs.update(knobs)

    def set_min_layers(self, n):
        self.r.tune("dle_min_layers", n)
        self.min_layers = n

    def restore(self):
        self.tune(**KNOBS)
        self.set_min_layers(16)

    def canvas(self, w, h):
        """DEPTH layer images of the canvas and their device copies, one destination and one mask behind them: made once, only descriptors change between cases"""
        if (w, h) not in self.images:
            rng = np.random.default_rng(w * 1000 + h)
            img = rng.integers(0, 256, (DEPTH, h, w, 4), dtype=np.uint8)
            u = rng.random((DEPTH, h, w))
            img[..., 3] = np.where(u < 0.25, 0, np.where(u < 0.5, 255, img[..., 3]))
            img[0, ..., 3] = 255
            bufs = [self.r.dev_alloc(w * h * 4) for _ in range(DEPTH + 2)]
            for k in range(DEPTH):
                self.r.dev_upload(bufs[k], img[k])
            self.images[(w, h)], self.bufs[(w, h)] = img, bufs
        return self.images[(w, h)], self.bufs[(w, h)]

    def free(self):
        for bufs in self.bufs.values():
            for b in bufs:
                self.r.dev_free(b)

    def want_plan(self, w, h, modes, opac, masked=(), has_preview=0, rect=None):
        n = len(modes)
        cands, shallow = Cands(), C.c_int(0)
        self.lib.pfx_int_flatten_cands((C.c_int * n)(*modes), (C.c_float * n)(*opac), (C.c_uint8 * n)(*[int(k in masked) for k in range(n)]), n, self.min_layers, 1,
                                       C.byref(cands), C.byref(shallow))
        assert shallow.value == 0 or cands.n == 0, "no stack of this file is left to the probe"
        c = FlattenCase(n_desc=n, w=w, h=h, general=int(bool(masked)), has_preview=has_preview, fast_div=1, mode_class=min(MODE_CLASS[m] for m in modes),
                        n_cands=cands.n, cand_top=cands.layer[cands.n - 1] if cands.n else 0, unorm_ok=self.unorm_ok, chunk_start=0, **self.knobs)
        if rect:
            c.rw, c.rh = rect[2], rect[3]
        p = FlattenPlan()
        self.lib.pfx_int_flatten_plan(C.byref(c), C.byref(p))
        return p

    def last_plan(self):
        p = FlattenPlan()
        assert self.lib.pfx_int_flatten_last_plan(self.r._h, C.byref(p)) == p.path
        return p

    def flatten(self, w, h, modes, opac, what):
        """one pfx_flatten_dev of the canvas's first len(modes) layers: the plan, then the image"""
        img, bufs = self.canvas(w, h)
        n = len(modes)
        self.r.flatten_dev(bufs[:n], [(k, float(opac[k]), True, int(modes[k])) for k in range(n)], w, h, bufs[DEPTH])
        got, want = self.last_plan(), self.want_plan(w, h, modes, opac)
        assert got.as_tuple() == want.as_tuple(), (what, self.knobs)
        ref = O.flatten_stack(img[:n], np.asarray(modes, np.uint8), np.asarray(opac, np.float32))
        out = self.r.dev_download(bufs[DEPTH], (h, w, 4))
        bad = (out != ref).any(-1)
        assert not bad.any(), f"{what} {self.knobs}: {int(bad.sum())} of {w * h} px differ, first at flat index {int(np.flatnonzero(bad)[0])}"
        return got


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.restore()
    g.free()


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_plain_stacks_by_depth_and_mode_class(gpu, canvas):
    """2, 5, 7, 16 and 17 layers of Normal (light), Overlay (medium) and Soft Light (heavy) below 100 %: the streaming kernel in every shape of the default rule"""
    w, h = canvas
    shapes = set()
    for mode in (NORMAL, OVERLAY, SOFT_LIGHT):
        for n in (2, 5, 7, 16, 17):
            opac = [1.0] + [0.5 + 0.03 * (k % 13) for k in range(1, n)]
            p = gpu.flatten(w, h, [NORMAL] + [mode] * (n - 1), opac, f"{n} layers of mode {mode}")
            assert p.kernel == STREAM
            shapes.add((p.px, p.nb))
    assert shapes == {(2, 2), (4, 2)}


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_overwrite_stacks_under_every_elimination_knob(gpu, canvas):
    """17 and 32 layers with an Overwrite layer at depth 14, the depth threshold off: both elimination kernels, 3 and 2 pixels per lane, equal and shrinking
    streams, default and (clamped) 340-unit streams"""
    w, h = canvas
    kernels = set()
    try:
        gpu.set_min_layers(0)
        for n in (17, 32):
            modes = [NORMAL] + [1 + (5 * k) % 24 for k in range(1, n)]
            modes = [m if m != OVERWRITE else 2 for m in modes]
            modes[14] = OVERWRITE
            opac = [1.0] + [0.7 if k == 14 else 0.4 + 0.04 * (k % 11) for k in range(1, n)]
            for kernel in (0, 1):
                for cfg in (0, 1):
                    for sched in (0, 1):
                        for units in (0, 340):
                            gpu.tune(kernel=kernel, cfg=cfg, sched=sched, units=units)
                            p = gpu.flatten(w, h, modes, opac, f"{n} layers, Overwrite at 14")
                            assert p.kernel == ((SRT if gpu.unorm_ok else DLE) if kernel == 0 else DLE) and p.px == (2 if cfg else 3)
                            kernels.add(p.kernel)
    finally:
        gpu.restore()
    assert DLE in kernels


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_masked_stack_rectangle_and_preview(gpu, canvas):
    """what leaves the fast kernels: a live mask (pfx_flatten_dev), a dirty rectangle (pfx_composite_region) and a tool preview (pfx_flatten_preview_dev)"""
    w, h = canvas
    img, bufs = gpu.canvas(w, h)
    n = 6
    modes, opac = [NORMAL, 1, OVERLAY, SOFT_LIGHT, 3, 9], [1.0, 0.8, 0.6, 1.0, 0.5, 0.9]
    info = [(k, opac[k], True, modes[k]) for k in range(n)]
    layers = [dict(pixels=img[k], mode=modes[k], opacity=opac[k]) for k in range(n)]
    r = gpu.r
    # a masked layer
    mask = np.random.default_rng(w).integers(0, 256, (h, w), dtype=np.uint8)
    r.dev_upload(bufs[DEPTH + 1], mask)
    r.flatten_dev(bufs[:n], info, w, h, bufs[DEPTH], mask_ptrs=[bufs[DEPTH + 1] if k == 2 else 0 for k in range(n)])
    assert gpu.last_plan().as_tuple() == gpu.want_plan(w, h, modes, opac, masked=(2,)).as_tuple()
    assert gpu.last_plan().kernel == TEMPLATE and gpu.last_plan().general == 1
    masked = [dict(L, mask=mask) if k == 2 else L for k, L in enumerate(layers)]
    assert np.array_equal(r.dev_download(bufs[DEPTH], (h, w, 4)), O.composite(masked, w, h))
    # a rectangle that starts off the 4-pixel grid and crosses a chunk edge
    rect = (61, 3, min(w - 61, 70), 62)
    r.clear_layers()
    try:
        for k in range(n):
            r.ensure_layer_texture(k, img[k], generation=1)
        got = r.composite_dirty_readback(w, h, info, rect)
    finally:
        r.clear_layers()
    assert gpu.last_plan().as_tuple() == gpu.want_plan(w, h, modes, opac, rect=rect).as_tuple()
    x, y, rw, rh = rect
    assert np.array_equal(got, O.composite(layers, w, h)[y:y + rh, x:x + rw])
    # a preview over layer 3
    pv = np.random.default_rng(h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    pv[: h // 2, ..., 3] = 0
    r.dev_upload(bufs[DEPTH + 1], pv)
    r.flatten_preview_dev(bufs[:n], info, w, h, bufs[DEPTH], bufs[DEPTH + 1], 3, blend_mode=NORMAL)
    assert gpu.last_plan().as_tuple() == gpu.want_plan(w, h, modes, opac, has_preview=1).as_tuple()
    want = O.composite(layers, w, h, preview=dict(pixels=pv, active_layer=3, blend_mode=NORMAL, is_eraser=False, replaces_layer=False, chunk_present=None))
    assert np.array_equal(r.dev_download(bufs[DEPTH], (h, w, 4)), want)
