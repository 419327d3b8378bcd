"""The streaming walk of the tool kernels (k_tools.h: four pixels per lane, then the n % 4 tail, else pixel by pixel), one table over its seven kernels through
their `_dev` entry points.  Each is held at tolerance 0 to the model that owns it (flood_model, colorkey_model, select_model).

  sizes     n = 1, 3 (no whole quad), 4 (one quad), 5 (a quad and a tail), 1027 (more than one 256-lane block of quads and of pixels, a tail of 3), as w x h with
            w no multiple of 4, so in the shape kernel a lane's four bytes straddle a row end.
  pointers  every buffer at a 16-byte aligned address (the four-per-lane arm), then u8 planes 1 byte and RGBA images 4 bytes further (the pixel-by-pixel arm;
            RGBA stays dword aligned, as the ABI requires).
  optional  the mask, selection or base plane given and NULL.
  wrap      the grid-stride step, once per arm, on the wand mask: one more lane's worth than 8192 blocks of 256 lanes hold, plus a tail."""
import numpy as np
import pytest

from . import colorkey_model as CM
from . import flood_model as FM
from . import select_model as SM
from .dev_buffers import Dev

pytestmark = pytest.mark.gpu

SHAPES = {1: (1, 1), 3: (3, 1), 4: (2, 2), 5: (5, 1), 1027: (13, 79)}   # n: (w, h)
FILL = (10, 220, 90, 128)
TARGET = (200, 60, 30, 180)
KEY = (40, 200, 60)


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


def image(w, h, seed, key_share=2 / 7):
    """RGBA8 noise over a few colours near KEY (that share of the pixels) and TARGET, some pixels transparent; pixel (0, 0) is KEY, opaque"""
    rng = np.random.default_rng(seed)
    palette = np.array([KEY + (255,), (44, 196, 63, 200), TARGET, (198, 64, 28, 90), (0, 0, 0, 0), (250, 250, 250, 255), (90, 90, 200, 17)], np.uint8)
    img = palette[rng.choice(len(palette), (h, w), p=[key_share / 2] * 2 + [(1 - key_share) / 5] * 5)]
    img[..., :3] += rng.integers(0, 3, (h, w, 3), dtype=np.uint8) * (img[..., 3:] != 0)   # values stay below 256
    img[0, 0] = KEY + (255,)
    return img


def plane(w, h, seed, zero_share=0.4):
    """a u8 plane with zeros, 255s and values between; byte (0, 0) is 255"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h, w), dtype=np.uint8)
    p[rng.random((h, w)) < zero_share] = 0
    p[rng.random((h, w)) < 0.2] = 255
    p[0, 0] = 255
    return p


# each row: (d, w, h, plane_offset, rgba_offset, optional given?) -> (got, want, [(input pointer, input array), ...])
def color_to_alpha(gpu, d, w, h, po, ro, given):
    img, mask = image(w, h, 1), plane(w, h, 2)
    d_src, d_dst, d_mask = d.put(img, ro), d.sentinel(img.shape, ro), d.put(mask, po)
    gpu.color_to_alpha_dev(d_src, d_dst, w, h, KEY, mask_ptr=d_mask if given else 0)
    return d.get(d_dst, img.shape), CM.color_to_alpha(img, mask if given else None, target=KEY), [(d_src, img), (d_mask, mask)]


def removal(smoothness, contiguous):
    def run(gpu, d, w, h, po, ro, given):
        img, sel = image(w, h, 3, key_share=0.7), plane(w, h, 4, zero_share=0.15)   # mostly passable: the flood gets far
        d_src, d_dst, d_sel = d.put(img, ro), d.sentinel(img.shape, ro), d.put(sel, po)
        gpu.color_removal_dev(d_src, d_dst, w, h, (0, 0), 12.0, smoothness, contiguous, d_sel if given else 0)
        want = CM.color_removal(img, (0, 0), 12.0, smoothness, contiguous, sel if given else None)
        return d.get(d_dst, img.shape), want, [(d_src, img), (d_sel, sel)]
    return run


def color_distance(mode):
    def run(gpu, d, w, h, po, ro, given):
        img = image(w, h, 5)
        d_src, d_out = d.put(img, ro), d.sentinel((h, w), po)
        gpu.flood_distance_dev(d_src, w, h, (0, 0), TARGET, d_out, mode, 4, True)
        return d.get(d_out, (h, w)), FM.distance_map(img, (0, 0), TARGET, mode, 4, True), [(d_src, img)]
    return run


def wand_mask(gpu, d, w, h, po, ro, given):
    dist, base = plane(w, h, 6), plane(w, h, 7)
    d_dist, d_base, d_out = d.put(dist, po), d.put(base, po), d.sentinel((h, w), po)
    gpu.wand_mask_dev(d_dist, w, h, 100, d_out, True, FM.ADD, d_base if given else 0)
    return d.get(d_out, (h, w)), FM.wand_mask(dist, 100, True, FM.ADD, base if given else None), [(d_dist, dist), (d_base, base)]


def fill_preview(gpu, d, w, h, po, ro, given):
    dist, sel = plane(w, h, 8), plane(w, h, 9)
    d_dist, d_sel, d_out = d.put(dist, po), d.put(sel, po), d.sentinel((h, w, 4), ro)
    gpu.fill_preview_dev(d_dist, w, h, 100, FILL, d_out, d_sel if given else 0)
    return d.get(d_out, (h, w, 4)), FM.fill_preview(dist, 100, FILL, sel if given else None), [(d_dist, dist), (d_sel, sel)]


def shape_combine(gpu, d, w, h, po, ro, given):
    """an ellipse over the canvas's middle, its box clipped by the canvas on two sides"""
    base = plane(w, h, 10)
    d_base, d_out = d.put(base, po), d.sentinel((h, w), po)
    cx, cy, rx, ry = w * 0.6, h * 0.45, w * 0.55 + 0.5, h * 0.4 + 0.5
    gpu.select_ellipse_dev(w, h, cx, cy, rx, ry, d_out, SM.ADD, d_base if given else 0)
    return d.get(d_out, (h, w)), SM.select_ellipse(base if given else None, w, h, cx, cy, rx, ry, SM.ADD), [(d_base, base)]


# kernel: (row, has an optional input)
ROWS = {
    "color_to_alpha": (color_to_alpha, True),
    "passable+rings": (removal(2, True), True),           # passable_kernel, the flood, then the ring kernel writes the image
    "passable+apply_core": (removal(0, False), True),     # passable_kernel's map is the core; apply_core_kernel writes the image
    "color_distance-legacy": (color_distance(FM.LEGACY), False),
    "color_distance-perceptual": (color_distance(FM.PERCEPTUAL), False),
    "wand_mask": (wand_mask, True),
    "fill_preview": (fill_preview, True),
    "shape_combine": (shape_combine, True),
}
CASES = [(name, n, arm, given) for name in ROWS for n in SHAPES for arm in ("vector", "bytes") for given in ((True, False) if ROWS[name][1] else (False,))]


@pytest.mark.parametrize("name,n,arm,given", CASES, ids=[f"{name}-{n}-{arm}-{'given' if given else 'null'}" for name, n, arm, given in CASES])
def test_walk_equals_the_model(gpu, name, n, arm, given):
    w, h = SHAPES[n]
    assert w * h == n and w % 4 != 0
    po, ro = (0, 0) if arm == "vector" else (1, 4)
    with Dev(gpu) as d:
        got, want, inputs = ROWS[name][0](gpu, d, w, h, po, ro, given)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (name, n, arm, given, int((got != want).sum()))
        for ptr, array in inputs:
            assert np.array_equal(d.get(ptr, array.shape), array), "an input was written"


WRAP = 8192 * 256   # lanes of the largest grid
@pytest.mark.parametrize("arm,n,offset", [("vector", WRAP * 4 + 5, 0), ("bytes", WRAP + 5, 1)], ids=["vector", "bytes"])
def test_grid_stride_wraps(gpu, arm, n, offset):
    """every lane of the largest grid has taken its first item when lane 0 comes round for item 8192 * 256; a tail follows"""
    rng = np.random.default_rng(11)
    dist, base = rng.integers(0, 256, (1, n), dtype=np.uint8), rng.integers(0, 256, (1, n), dtype=np.uint8)
    want = FM.wand_mask(dist, 100, True, FM.ADD, base)
    with Dev(gpu) as d:
        d_dist, d_base, d_out = d.put(dist, offset), d.put(base, offset), d.sentinel((1, n), offset)
        gpu.wand_mask_dev(d_dist, n, 1, 100, d_out, True, FM.ADD, d_base)
        got = d.get(d_out, (1, n))
    assert np.array_equal(got, want), (arm, int((got != want).sum()), int(np.flatnonzero(got != want)[:1].sum()))
