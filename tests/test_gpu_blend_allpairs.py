"""Parity gate (GPU): every (accumulator byte, layer byte) pair of every colour channel through the mode functions that round 9 shortened or put on an
unrefined reciprocal (k_blend.h: vivid_light_channel, pin_light_channel, div_raw_rcp), and through their neighbours in the dispatch.

The frame holds 65 536 pixels; pixel i meets accumulator byte b = i & 255 and layer byte t = i >> 8, decorrelated per channel: (b, 255 - b, b ^ 0x55) under
(t, 255 - t, t ^ 0x55).  At 256 px wide that is accumulator byte x under layer byte y; at 193 px wide the same pairs sit across the class-sorting kernel's
192-pixel unit and its one-pixel tail.  The accumulator is set by an Overwrite layer at 100 % right above the bottom layer (Overwrite hands its bytes on
unchanged, alpha included), the layer under test follows it, and the layers above are transparent, so the stored byte is the one the mode function decides.

Three accumulator classes per mode and kernel: an opaque accumulator under an opaque layer at 100 % (the result is trunc(f * 255): a mode function one ulp
off shows wherever f * 255 is an integer); an opaque accumulator under opacities 0.5 and 1 - 2^-24; a general accumulator (alpha 128) under 1.0 and 0.5.  In
the last two the layer's alpha is {0, 1, 127, 255} interleaved lane by lane, in each of its four rotations, so that every pair meets every alpha.
Everything compares with oracle_lib.flatten_stack at tolerance 0.

This file is what certifies a blend mode for div_raw_rcp: a mode's bit is set in PFX_DIV_RAW_MODES only if its cases pass here with the bit set."""
import numpy as np
import pytest

from . import oracle_lib as O

pytestmark = pytest.mark.gpu

NORMAL, OVERWRITE = 0, 14
MODES = [4, 5, 6, 7, 8, 15, 16, 19, 21, 23, 24]   # Reflect, Glow, Color Burn, Color Dodge, Overlay, Hard Light, Soft Light, Divide, Vivid Light, Pin Light, Hard Mix
ALPHAS = np.array([0, 1, 127, 255], np.uint8)
ALMOST_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # 1 - 2^-24
# kernel -> (layers, flatten_variant, masked layer or None), as in test_gpu_blend_writeback.py
KERNELS = {
    "class-sorting-16": (16, 0, None),   # 16 layers with an Overwrite layer above the bottom: flatten_srt_kernel
    "streaming-5": (5, 8, None),         # flatten_variant 8: no elimination kernel, whatever the stack holds
    "general-masked-5": (5, 0, 2),      # a live mask (that conceals nothing) moves the stack to flatten_kernel<GENERAL>
}
# class -> (accumulator alpha, interleaved layer alpha, opacities)
CLASSES = {
    "opaque-under-opaque-100": (255, False, [1.0]),
    "opaque": (255, True, [0.5, ALMOST_ONE]),
    "general": (128, True, [1.0, 0.5]),
}
SHAPES = {256: (256, 256), 193: (193, 340)}   # 340 rows of 193: the first 65 536 pixels carry the pairs, the rest repeat the start
ACC_LAYER, TEST_LAYER = 1, 2


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    g = GpuBackend(0)
    yield g
    g.r.tune("flatten_variant", 0)


def pair_planes(w, h):
    i = np.arange(w * h).reshape(h, w)
    b, t = (i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8)
    return i, b, t


def build_stack(w, h, n, acc_alpha, seed):
    """layer 0: random and opaque; ACC_LAYER: the accumulator bytes; TEST_LAYER: the layer bytes (its alpha is set per composite); above: random colours, alpha 0"""
    rng = np.random.default_rng(seed)
    stack = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    _, b, t = pair_planes(w, h)
    stack[0, ..., 3] = 255
    stack[ACC_LAYER, ..., 0], stack[ACC_LAYER, ..., 1], stack[ACC_LAYER, ..., 2], stack[ACC_LAYER, ..., 3] = b, 255 - b, b ^ 0x55, acc_alpha
    stack[TEST_LAYER, ..., 0], stack[TEST_LAYER, ..., 1], stack[TEST_LAYER, ..., 2], stack[TEST_LAYER, ..., 3] = t, 255 - t, t ^ 0x55, 255
    stack[TEST_LAYER + 1:, ..., 3] = 0
    return stack


def test_the_frame_holds_every_pair_on_every_channel():
    for w, h in SHAPES.values():
        s = build_stack(w, h, 3, 255, 0)
        for c in range(3):
            pairs = s[ACC_LAYER, ..., c].astype(np.uint32).ravel() * 256 + s[TEST_LAYER, ..., c].ravel()
            assert np.unique(pairs).size == 65536


class Frame:
    """a stack resident on the device; composite(modes, opac) runs pfx_flatten_dev and returns (got, ref)"""

    def __init__(self, gpu, stack, variant, masked):
        self.r, self.stack = gpu.r, stack
        self.n, self.h, self.w, _ = stack.shape
        self.bufs = [self.r.dev_alloc(self.w * self.h * 4) for _ in range(self.n + 1)]
        self.mbuf, self.masks = None, None
        for k in range(self.n):
            self.r.dev_upload(self.bufs[k], stack[k])
        if masked is not None:
            self.mbuf = self.r.dev_alloc(self.w * self.h)
            self.r.dev_upload(self.mbuf, np.zeros((self.h, self.w), np.uint8))
            self.masks = [0] * self.n
            self.masks[masked] = self.mbuf
        self.r.tune("flatten_variant", variant)

    def set_layer(self, k, pixels):
        self.stack[k] = pixels
        self.r.dev_upload(self.bufs[k], self.stack[k])

    def composite(self, modes, opac):
        info = [(k, float(opac[k]), True, int(modes[k])) for k in range(self.n)]
        self.r.flatten_dev(self.bufs[:self.n], info, self.w, self.h, self.bufs[self.n], mask_ptrs=self.masks)
        got = self.r.dev_download(self.bufs[self.n], (self.h, self.w, 4))
        ref = O.flatten_stack(self.stack, np.asarray(modes, np.uint8), np.asarray(opac, np.float32))
        return got, ref

    def units_of_the_class_sorting_kernel(self, modes, opac):
        self.r.tune("dle_stats", 1)
        try:
            self.r.flatten_stats(reset=True)
            self.composite(modes, opac)
            return self.r.flatten_stats(reset=True)["nat_units"]
        finally:
            self.r.tune("dle_stats", 0)

    def close(self):
        self.r.tune("flatten_variant", 0)
        for b in self.bufs:
            self.r.dev_free(b)
        if self.mbuf is not None:
            self.r.dev_free(self.mbuf)


@pytest.mark.parametrize("width", list(SHAPES))
@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("mode", MODES)
def test_every_byte_pair_of_every_channel(gpu, mode, kernel, cls, width):
    n, variant, masked = KERNELS[kernel]
    acc_alpha, interleaved, opacities = CLASSES[cls]
    w, h = SHAPES[width]
    f = Frame(gpu, build_stack(w, h, n, acc_alpha, 900 + mode), variant, masked)
    i, _, _ = pair_planes(w, h)
    failures = []
    try:
        modes = [NORMAL, OVERWRITE, mode] + [NORMAL] * (n - 3)
        if kernel == "class-sorting-16" and cls == "general":   # the stack does reach the class-sorting kernel: every unit has its natural pass there
            assert f.units_of_the_class_sorting_kernel(modes, [1.0] * n) > 0
        rotations = range(4) if (interleaved and width == 256) else range(1)
        for rot in rotations:
            if interleaved:   # at 256 px wide (i + (i >> 8)) & 3 is (x + y) & 3: lane by lane along a row, shifted row by row
                px = f.stack[TEST_LAYER].copy()
                px[..., 3] = ALPHAS[(i + (i >> 8) + rot) & 3]
                f.set_layer(TEST_LAYER, px)
            for opacity in opacities:
                opac = [1.0, 1.0, opacity] + [1.0] * (n - 3)
                got, ref = f.composite(modes, opac)
                bad = (got != ref).any(-1)
                if bad.any():
                    y, x = (int(v) for v in np.argwhere(bad)[0])
                    failures.append(f"opacity {opacity!r}, alpha rotation {rot}: {int(bad.sum())} of {w * h} px differ, first at pixel {y * w + x}: "
                                    f"accumulator {f.stack[ACC_LAYER, y, x].tolist()} layer {f.stack[TEST_LAYER, y, x].tolist()} got {got[y, x].tolist()} want {ref[y, x].tolist()}")
    finally:
        f.close()
    assert not failures, f"mode {mode}, {kernel}, {cls}, {w} x {h}:\n" + "\n".join(failures[:8])
