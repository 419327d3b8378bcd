"""Visibility gate (GPU) for the class-sorting compositor's memory requests: whatever cache policy its loads and its store carry, a launch reads what the
kernel before it on the stream wrote, and the kernel behind it reads what the launch stored.  Everything at tolerance 0 against tests/oracle_lib, with the
renderer on torch's current stream (as bench.py sets it) and no synchronisation between the calls under test.

Stacks: 16 and 17 layers, S2's alpha distribution (a quarter 0, a quarter 255, the rest 1 .. 254; layer 0 opaque), modes k mod 25 with Overwrite moved to
depth 7 (its own mode 7 goes to depth 14), so depth 7 is the stack's only reset candidate: PFXK_FLATTEN_SRT, a quarter of every unit's pixels early.
Sizes: 191, 192, 193 pixels (one unit of 3 x 64 less one, exactly, plus one), 385 (two units and a pixel) and 8 * 192 + 1 (a wave's stream of units and a
pixel), as single rows and as 64 pixels by that many rows."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  -- before libpfx.so is loaded (see test_gpu_fullsize.py)

from . import oracle_lib as O
from .test_flatten_dispatch_host import KNOBS, Cands, FlattenCase, FlattenPlan, bind

pytestmark = pytest.mark.gpu

OVERWRITE, RESET = 14, 7
SRT = 3
MODE_CLASS = [2, 2, 1, 2, 0, 0, 0, 0, 1, 2, 1, 2, 2, 0, 2, 1, 0, 1, 2, 0, 2, 0, 1, 0, 1]   # pfx_flatten.cpp: build_stack
PIXELS = [191, 192, 193, 385, 8 * 192 + 1]
SHAPES = [(n, 1) for n in PIXELS] + [(64, n) for n in PIXELS]


def stack_modes(n):
    m = [k % 25 for k in range(n)]
    m[RESET], m[14] = OVERWRITE, RESET
    return m


def stack_opacity(n):
    return [1.0] + [0.45 + 0.05 * (k % 11) for k in range(1, n)]


def s2_layers(n, w, h, seed, reset_alpha=None):
    """S2 (bench.py: synth_layer): uniform RGB; alpha a quarter 0, a quarter 255, the rest uniform 1 .. 254; layer 0 opaque"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    u = rng.random((n, h, w))
    img[..., 3] = np.where(u < 0.25, 0, np.where(u < 0.5, 255, rng.integers(1, 255, (n, h, w), dtype=np.uint8)))
    img[0, ..., 3] = 255
    if reset_alpha == "covering":
        img[RESET, ..., 3] = np.maximum(img[RESET, ..., 3], 1)
    elif reset_alpha == "absent":
        img[RESET, ..., 3] = 0
    return img


class Env:
    def __init__(self):
        from paintfe_amd import GpuRenderer
        assert torch.cuda.is_available()
        torch.cuda.set_device(0)
        self.dev = torch.device("cuda", 0)
        self.r = GpuRenderer(0)
        self.r.set_stream(torch.cuda.current_stream().cuda_stream)
        self.lib = bind(self.r._lib)
        self.lib.pfx_int_flatten_last_plan.argtypes = [C.c_void_p, C.POINTER(FlattenPlan)]
        self.lib.pfx_int_flatten_last_plan.restype = C.c_int
        self.unorm_ok = int(self.r.selftest_unorm_store() == 0)

    def upload(self, img):
        return [torch.from_numpy(np.ascontiguousarray(img[k])).to(self.dev) for k in range(img.shape[0])]

    def flatten(self, layers, modes, opac, w, h, dst):
        n = len(modes)
        self.r.flatten_dev([t.data_ptr() for t in layers[:n]], [(k, float(opac[k]), True, int(modes[k])) for k in range(n)], w, h, dst.data_ptr())

    def check_plan(self, n, w, h, stats=0):
        """the recorded plan is the pure decision's for this stack, and that is the class-sorting kernel"""
        modes, opac = stack_modes(n), stack_opacity(n)
        cands, shallow = Cands(), C.c_int(0)
        self.lib.pfx_int_flatten_cands((C.c_int * n)(*modes), (C.c_float * n)(*opac), (C.c_uint8 * n)(), n, 16, 1, C.byref(cands), C.byref(shallow))
        assert cands.n == 1 and cands.layer[0] == RESET and shallow.value == 0
        c = FlattenCase(n_desc=n, w=w, h=h, general=0, has_preview=0, fast_div=1, mode_class=min(MODE_CLASS[m] for m in modes), n_cands=1, cand_top=RESET,
                        unorm_ok=self.unorm_ok, chunk_start=0, **dict(KNOBS, stats=stats))
        want, got = FlattenPlan(), FlattenPlan()
        self.lib.pfx_int_flatten_plan(C.byref(c), C.byref(want))
        assert self.lib.pfx_int_flatten_last_plan(self.r._h, C.byref(got)) == got.path
        assert got.as_tuple() == want.as_tuple()
        assert self.unorm_ok and got.kernel == SRT and got.px == 3


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    torch.cuda.synchronize()
    e.r.tune("dle_stats", 0)
    e.r.close()


def differ(out, ref, what):
    bad = (out != ref).any(-1).ravel()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} px differ, first at flat index {int(np.flatnonzero(bad)[0])}"


@pytest.mark.parametrize("reset_alpha", ["s2", "covering", "absent"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unit_and_stream_edges(env, shape, reset_alpha):
    """s2: every unit deals its early quarter to a leading group.  covering: the reset layer hides everything below it — no early pass in a whole unit, which
    starts at depth 7 on the alpha requested a unit ahead.  absent: the reset layer is transparent — the probes fail, the wave backs off and the look-ahead request
    goes through the resource of zero records."""
    w, h = shape
    for n in (16, 17):
        img = s2_layers(n, w, h, 1000 * n + w + h, reset_alpha)
        modes, opac = stack_modes(n), stack_opacity(n)
        layers = env.upload(img)
        dst = torch.full((h, w, 4), 0xA5, dtype=torch.uint8, device=env.dev)
        env.flatten(layers, modes, opac, w, h, dst)
        env.check_plan(n, w, h)
        torch.cuda.synchronize()
        differ(dst.cpu().numpy(), O.flatten_stack(img, np.asarray(modes, np.uint8), np.asarray(opac, np.float32)), f"{n} layers {w}x{h} {reset_alpha}")


def test_early_groups_run_and_do_not_when_the_reset_layer_covers(env):
    """the kernel's own work counters: S2 alpha splits every unit (one early group each over layers 0 .. 6), a covering reset layer splits none
    (64 whole units: the pixels behind the image's end in a partial unit read as transparent, i.e. as early ones)"""
    w, h, n = 64, 192, 17
    units = w * h // 192
    try:
        env.r.tune("dle_stats", 1)
        for reset_alpha, split in (("s2", True), ("covering", False)):
            img = s2_layers(n, w, h, 5, reset_alpha)
            layers = env.upload(img)
            dst = torch.empty((h, w, 4), dtype=torch.uint8, device=env.dev)
            env.r.flatten_stats(reset=True)
            env.flatten(layers, stack_modes(n), stack_opacity(n), w, h, dst)
            env.check_plan(n, w, h, stats=1)
            s = env.r.flatten_stats(reset=True)
            assert s["nat_units"] == units
            if split:   # 48 early pixels a unit on average, 64 to a group: at most a handful of units need none or two
                assert 0.9 * units <= s["queue_units"] <= units and s["rounds"] >= s["queue_units"] and s["round_layers"] == RESET * s["rounds"]
            else:
                assert s["queue_units"] == 0 and s["rounds"] == 0 and s["nat_layers"] == (n - RESET) * units
            differ(dst.cpu().numpy(), O.flatten_stack(img, np.asarray(stack_modes(n), np.uint8), np.asarray(stack_opacity(n), np.float32)), reset_alpha)
    finally:
        env.r.tune("dle_stats", 0)


@pytest.mark.parametrize("layer", [3, RESET], ids=["below_the_reset_layer", "the_reset_layer"])
def test_write_then_read_without_synchronisation(env, layer):
    """a kernel on the stream rewrites one layer right in front of the composite, twice with different content (an in-place invert, then a device copy of
    fresh pixels); a composite before each rewrite has put the old lines into every cache.  Each result is the oracle's on the NEW content."""
    w, h, n = 193, 67, 17
    modes, opac = stack_modes(n), stack_opacity(n)
    img = s2_layers(n, w, h, 77)
    fresh = s2_layers(n, w, h, 78)[layer]
    layers = env.upload(img)
    fresh_d = torch.from_numpy(np.ascontiguousarray(fresh)).to(env.dev)
    d0, d1, d2 = (torch.empty((h, w, 4), dtype=torch.uint8, device=env.dev) for _ in range(3))
    torch.cuda.synchronize()
    env.flatten(layers, modes, opac, w, h, d0)                                   # the old content is cached
    env.r.adjust_dev(layers[layer].data_ptr(), layers[layer].data_ptr(), w, h, "invert")
    env.flatten(layers, modes, opac, w, h, d1)
    layers[layer].copy_(fresh_d)
    env.flatten(layers, modes, opac, w, h, d2)
    env.check_plan(n, w, h)
    torch.cuda.synchronize()
    m, o = np.asarray(modes, np.uint8), np.asarray(opac, np.float32)
    differ(d0.cpu().numpy(), O.flatten_stack(img, m, o), "before any rewrite")
    inv = img.copy()
    inv[layer] = O.adjust(img[layer], "invert")
    assert np.array_equal(layers[layer].cpu().numpy(), fresh) and not np.array_equal(inv[layer], img[layer])
    differ(d1.cpu().numpy(), O.flatten_stack(inv, m, o), f"layer {layer} inverted in place in front of the composite")
    new = img.copy()
    new[layer] = fresh
    differ(d2.cpu().numpy(), O.flatten_stack(new, m, o), f"layer {layer} overwritten by a device copy in front of the composite")


@pytest.mark.parametrize("shape", [(193, 67), (385, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_gaussian_reads_what_the_composite_stored(env, shape):
    """flatten_dev, then gaussian_blur_dev in exact mode on its result, nothing between them: the oracle's blur of the oracle's composite"""
    w, h = shape
    n, sigma = 17, 3.0
    modes, opac = stack_modes(n), stack_opacity(n)
    img = s2_layers(n, w, h, 300 + w)
    layers = env.upload(img)
    flat = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device=env.dev)
    blur = torch.empty_like(flat)
    torch.cuda.synchronize()
    env.r.set_exact(True)
    try:
        env.flatten(layers, modes, opac, w, h, flat)
        env.r.gaussian_blur_dev(flat.data_ptr(), blur.data_ptr(), w, h, sigma)
        torch.cuda.synchronize()
    finally:
        env.r.set_exact(False)
    env.check_plan(n, w, h)
    ref = O.flatten_stack(img, np.asarray(modes, np.uint8), np.asarray(opac, np.float32))
    differ(flat.cpu().numpy(), ref, "composite")
    differ(blur.cpu().numpy(), O.gaussian_blur(ref, sigma), "exact Gaussian of the composite")


def test_destination_may_be_a_layer(env):
    """pfx_flatten_dev's argument check lets dst BE a layer (a partial overlap is refused): the reset layer, whose alpha the kernel also probes a unit ahead"""
    from paintfe_amd._lib import PfxError, ERR_INVALID
    w, h, n = 385, 40, 17
    modes, opac = stack_modes(n), stack_opacity(n)
    img = s2_layers(n, w, h, 411)
    layers = env.upload(img)
    env.flatten(layers, modes, opac, w, h, layers[RESET])
    env.check_plan(n, w, h)
    torch.cuda.synchronize()
    differ(layers[RESET].cpu().numpy(), O.flatten_stack(img, np.asarray(modes, np.uint8), np.asarray(opac, np.float32)), "dst is layer 7")
    big = torch.zeros((2 * h, w, 4), dtype=torch.uint8, device=env.dev)
    ptrs = [t.data_ptr() for t in layers]
    ptrs[3] = big.data_ptr()
    with pytest.raises(PfxError) as e:
        env.r.flatten_dev(ptrs, [(k, float(opac[k]), True, int(modes[k])) for k in range(n)], w, h, big.data_ptr() + 64)
    assert e.value.status == ERR_INVALID
