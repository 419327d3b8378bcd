"""Parity gate (GPU): the compositor's masked write-back, raw Overwrite colour channels and unit-opacity composites (k_blend.h: requant_keep,
blend_nx<M_OVERWRITE>, comp_nx<OB, UO>).

The reference's early-out for a transparent layer pixel (canvas_state.rs:1253) is, on the device, four FMAs issued under an EXEC mask instead of
four selects; Overwrite hands the layer pixel's colour channels on without re-quantising them; and a layer whose clamped opacity is exactly 1.0
takes composites that do not multiply by it.  What can go wrong: a lane that must keep its accumulator is written (or the reverse), a NaN of a
discarded lane (0 / 0 under a transparent pixel over a transparent accumulator) reaches a stored value, the wrong composite variant is chosen
for a class of accumulators, or a byte value does not survive Overwrite.

Every case is pfx_flatten_dev against oracle_lib.flatten_stack at tolerance 0 on an n x 1 image of 191, 192, 193 or 385 pixels (one unit of the
class-sorting kernel - 1, exactly, + 1; two units + 1).  The layers under test carry alpha {0, 1, 127, 254, 255} interleaved lane by lane, so
that every wave has written and kept lanes, over accumulators that are transparent, partial and opaque: whole 64-pixel groups of each and mixed
within a group, which puts every count of leading opaque groups on both sides of the unit-opacity variants.  The layers of a stack are uploaded
once; the 25 modes x 6 opacities only change the descriptors."""
import numpy as np
import pytest

from . import oracle_lib as O

pytestmark = pytest.mark.gpu

NORMAL, OVERWRITE = 0, 14
ALPHAS = np.array([0, 1, 127, 254, 255], np.uint8)
OPACITIES = [1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), 0.5, 0.0, 1.5, float(np.float32(2.0) ** -30)]
PIXELS = [191, 192, 193, 385]
# kernel -> (layers, position of a fixed Overwrite layer or None, flatten_variant, masked layer or None)
KERNELS = {
    "class-sorting-16": (16, 5, 0, None),     # 16 layers and a reset candidate: flatten_srt_kernel
    "streaming-5": (5, None, 8, None),        # flatten_variant 8: no elimination kernel, whatever the stack holds
    "streaming-9": (9, None, 8, None),
    "general-masked-5": (5, None, 0, 2),      # a live mask (that conceals nothing) moves the stack to flatten_kernel<GENERAL>
}


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    g = GpuBackend(0)
    yield g
    g.r.tune("flatten_variant", 0)


def base_alpha(npx):
    """the bottom layer's alpha, i.e. the accumulators the layers under test meet: 64-pixel groups that are opaque, transparent, mixed lane by lane, partial,
    mixed, opaque (the class-sorting kernel's unit is three groups)"""
    i = np.arange(npx)
    mixed = np.array([255, 0, 77, 255, 200, 0], np.uint8)[i % 6]
    kinds = [np.full(npx, 255, np.uint8), np.zeros(npx, np.uint8), mixed, np.full(npx, 143, np.uint8), mixed, np.full(npx, 255, np.uint8)]
    return np.choose((i // 64) % 6, kinds).astype(np.uint8)


def build_layers(npx, n, seed):
    """n layers of npx x 1: layer 0 sets the accumulators up; every other layer has random colours and alpha {0, 1, 127, 254, 255} interleaved per lane.  In
    every other run of five pixels the alpha pattern stays put from layer to layer (a pixel that is transparent in every layer keeps a transparent accumulator
    transparent all the way up: den == 0 under a transparent layer pixel, layer after layer); in the runs between it rotates by one per layer"""
    rng = np.random.default_rng(seed)
    stack = rng.integers(0, 256, (n, 1, npx, 4), dtype=np.uint8)
    i = np.arange(npx)
    stack[0, 0, :, 3] = base_alpha(npx)
    for k in range(1, n):
        stack[k, 0, :, 3] = ALPHAS[(i + k * ((i // 5) % 2)) % 5]
    return stack


class Stack:
    """layers resident on the device; composite(modes, opac) runs pfx_flatten_dev and returns (got, ref)"""

    def __init__(self, gpu, stack, variant, masked):
        self.r, self.stack, self.variant = gpu.r, stack, variant
        n, _, npx, _ = stack.shape
        self.n, self.npx = n, npx
        self.bufs = [self.r.dev_alloc(npx * 4) for _ in range(n + 1)]
        self.mbuf, self.masks = None, None
        for k in range(n):
            self.r.dev_upload(self.bufs[k], stack[k])
        if masked is not None:
            self.mbuf = self.r.dev_alloc(npx)
            self.r.dev_upload(self.mbuf, np.zeros((1, npx), np.uint8))
            self.masks = [0] * n
            self.masks[masked] = self.mbuf
        self.r.tune("flatten_variant", variant)

    def composite(self, modes, opac):
        info = [(k, float(opac[k]), True, int(modes[k])) for k in range(self.n)]
        self.r.flatten_dev(self.bufs[:self.n], info, self.npx, 1, self.bufs[self.n], mask_ptrs=self.masks)
        got = self.r.dev_download(self.bufs[self.n], (1, self.npx, 4))
        ref = O.flatten_stack(self.stack, np.asarray(modes, np.uint8), np.asarray(opac, np.float32))
        return got, ref

    def units_of_the_class_sorting_kernel(self, modes, opac):
        """the launch's work counters (pfx_flatten_stats): units whose natural pass flatten_srt_kernel ran"""
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


@pytest.mark.parametrize("npx", PIXELS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_every_mode_and_opacity_over_every_accumulator_class(gpu, kernel, npx):
    """each of the 25 modes at each opacity on every layer above the bottom one (but the class-sorting stack's fixed Overwrite layer, whose holes split its units
    into an early and a natural pass)"""
    n, reset, variant, masked = KERNELS[kernel]
    stack = build_layers(npx, n, 1000 + npx + n)
    if reset is not None:   # the fixed Overwrite layer: alpha zero on every third run of seven pixels
        i = np.arange(npx)
        stack[reset, 0, :, 3] = np.where((i // 7) % 3 == 0, 0, stack[reset, 0, :, 3] | 1)
    s = Stack(gpu, stack, variant, masked)
    failures = []
    try:
        if reset is not None:   # the stack does reach the class-sorting kernel: every unit of the image has a natural pass there
            modes, opac = [NORMAL] + [1] * (n - 1), [1.0] + [0.5] * (n - 1)
            modes[reset], opac[reset] = OVERWRITE, 0.7
            assert s.units_of_the_class_sorting_kernel(modes, opac) == (npx + 191) // 192
        for mode in range(25):
            for opacity in OPACITIES:
                modes = [NORMAL] + [mode] * (n - 1)
                opac = [1.0] + [opacity] * (n - 1)
                if reset is not None:
                    modes[reset], opac[reset] = OVERWRITE, 0.7
                got, ref = s.composite(modes, opac)
                bad = (got != ref).any(-1)
                if bad.any():
                    j = int(np.flatnonzero(bad.ravel())[0])
                    failures.append(f"mode {mode} opacity {opacity!r}: {int(bad.sum())} of {npx} px differ, first at {j}: got {got[0, j].tolist()} want {ref[0, j].tolist()}")
    finally:
        s.close()
    assert not failures, f"{kernel}, {npx} px: {len(failures)} of {25 * len(OPACITIES)} composites differ\n" + "\n".join(failures[:10])


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_overwrite_hands_on_every_byte_value_of_every_colour_channel(gpu, kernel):
    """385 pixels: every value 0 .. 255 on each colour channel of an Overwrite layer under a non-zero alpha (pixels 0 .. 255; behind them alpha 0 is interleaved
    again), at each opacity, with the Overwrite layer on top of the stack (its pixels are the result) and in its middle (they are the accumulators of what follows)"""
    n, reset, variant, masked = KERNELS[kernel]
    npx = 385
    i = np.arange(npx)
    failures = []
    for pos in (n - 1, n // 2):
        stack = build_layers(npx, n, 2000 + n + pos)
        stack[pos, 0, :, 0] = i % 256
        stack[pos, 0, :, 1] = (i + 85) % 256
        stack[pos, 0, :, 2] = (255 - i) % 256
        stack[pos, 0, :, 3] = np.where(i < 256, ALPHAS[1 + i % 4], ALPHAS[i % 5])
        s = Stack(gpu, stack, variant, masked)
        try:
            for opacity in OPACITIES:
                modes = [NORMAL] + [1 + (7 * k) % 13 for k in range(1, n)]      # Multiply .. Xor above and below it
                opac = [1.0] + [0.6 if k % 2 else 1.0 for k in range(1, n)]
                modes[pos], opac[pos] = OVERWRITE, opacity
                got, ref = s.composite(modes, opac)
                bad = (got != ref).any(-1)
                if bad.any():
                    j = int(np.flatnonzero(bad.ravel())[0])
                    failures.append(f"Overwrite at layer {pos} opacity {opacity!r}: {int(bad.sum())} of {npx} px differ, first at {j}: got {got[0, j].tolist()} want {ref[0, j].tolist()}")
        finally:
            s.close()
    assert not failures, f"{kernel}: " + "\n".join(failures[:10])
