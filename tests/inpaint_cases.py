"""Inputs of the content-aware fill tests: the reference's two golden inputs (tests/inpaint.rs:18-63) and the seeded sweeps of the device parity tests.

Instant sweep (canvas 131 x 77): every case must change at least 20 pixels in the model, except the two whose point is that nothing may change
(`outside`: the brush lies wholly off the canvas; `all_in_hole`: every ring candidate lies in the hole), which must change none.
PatchMatch sweep (61 x 45 and 64 x 64, holes of at most about 250 pixels): patch sizes 3, 4, 5, 7, 9, 11 and iterations 3 and 6 are dealt over the hole
shapes and the two kinds of content; `bw_split` reaches the sequential-f32 SSD branch (integer sum >= 2^24), `ring_pixel_island` leaves boundary pixels
unfilled (a one-pixel island gives its four neighbours one valid patch pixel, below min_valid = 2 of patch 3).
PatchMatch edges (`PATCHMATCH_EDGES`): one case per loop of k_inpaint.hip that walks block-sized pieces; each leaves the first turn of exactly the loop it is
named for.  tests/test_inpaint_model_host.py holds every case to the condition that makes it cross its edge, so a later edit of a mask cannot un-cross it.
Second instant canvas (301 x 203, no multiple of 64 or 4): dab lists whose union box is almost the canvas, and a chain of 65 overlapping dabs."""
import functools
import os

import numpy as np

from . import inpaint_model as M

GOLDEN_W = GOLDEN_H = 64
SWEEP_W, SWEEP_H = 131, 77
SWEEP2_W, SWEEP2_H = 301, 203      # the second instant canvas: several 64 x 4 thread blocks in both directions, ragged in both


def load_goldens():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inpaint.npz"))


def _checkerboard():
    y, x = np.mgrid[0:64, 0:64]
    img = np.empty((64, 64, 4), np.uint8)
    even = ((x // 8 + y // 8) % 2 == 0)
    img[even] = (200, 50, 50, 255)
    img[~even] = (50, 50, 200, 255)
    return img


def golden_instant():
    """pattern_with_hole + the golden's call: (src, mask, out, dabs)"""
    img = _checkerboard()
    mask = np.zeros((64, 64), np.uint8)
    mask[24:40, 24:40] = 255
    return img, mask, img.copy(), [(32.0, 32.0, 12.0, 24.0, 0.8)]


def golden_patchmatch():
    """pattern_with_transparent_hole + the golden's call: (src, mask, patch_size, iterations)"""
    img = _checkerboard()
    mask = np.zeros((64, 64), np.uint8)
    mask[24:40, 24:40] = 255
    img[24:40, 24:40] = 0
    return img, mask, 5, 3


# ---------------------------------------------------------------------------------------------------------------- instant sweep

def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return img


def _ramp(w, h):
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = np.minimum((x + y) * 2, 255)
    img[..., 1] = 100
    img[..., 2] = np.minimum(x * 3 // 2, 255)
    img[..., 3] = 255
    return img


def _rect_mask(w, h, x0, y0, x1, y1, value=255):
    m = np.zeros((h, w), np.uint8)
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = value
    return m


def instant_cases():
    """[(name, src, mask, out, dabs, expect)] with expect "changes" (>= 20 pixels) or "nothing" (0 pixels)"""
    W, H = SWEEP_W, SWEEP_H
    cases = []
    # the reference's gradient with a shifted patch (tests/inpaint.rs:70-114), on this canvas
    y, x = np.mgrid[0:H, 0:W]
    grad = np.empty((H, W, 4), np.uint8)
    grad[..., 0] = np.minimum((x + y) * 2, 255)
    grad[..., 1], grad[..., 2], grad[..., 3] = 100, 150, 255
    mask = _rect_mask(W, H, 28, 28, 36, 36)
    grad[28:36, 28:36, 0] = np.minimum(grad[28:36, 28:36, 0].astype(int) + 30, 255)
    cases.append(("gradient_shifted_patch", grad, mask, grad.copy(), [(32.0, 32.0, 10.0, 18.0, 0.5)], "changes"))

    noise = _noise(W, H, 11)
    ramp = _ramp(W, H)
    hole = _rect_mask(W, H, 50, 25, 80, 50)
    clear = np.zeros_like(noise)
    mixed = _noise(W, H, 12)
    mixed[..., 3] = np.random.default_rng(13).choice(np.array([0, 64, 128, 255], np.uint8), (H, W))
    cases.append(("transparent_out_noise", noise, hole, clear, [(64.0, 38.0, 14.0, 24.0, 0.5)], "changes"))
    cases.append(("transparent_out_ramp", ramp, hole, clear, [(64.0, 38.0, 14.0, 24.0, 0.3)], "changes"))
    cases.append(("opaque_out_noise", noise, hole, noise.copy(), [(64.0, 38.0, 14.0, 24.0, 0.8)], "changes"))
    for hd in (0.0, 0.5, 1.0):
        cases.append((f"hardness_{hd}", noise, hole, mixed, [(66.0, 36.0, 13.0, 20.0, hd)], "changes"))
    cases.append(("fractional_centre", noise, hole, mixed, [(63.37, 39.81, 11.25, 17.5, 0.4)], "changes"))
    cases.append(("radius_below_one", noise, _rect_mask(W, H, 0, 0, W, 8), clear,
                  [(float(3 * i) + 0.25, 3.5, 0.2, 12.0, 0.5) for i in range(40)], "changes"))
    edges = {"left": (2.5, 40.0, _rect_mask(W, H, 0, 28, 12, 52)), "right": (128.5, 40.0, _rect_mask(W, H, 119, 28, W, 52)),
             "top": (60.0, 1.5, _rect_mask(W, H, 48, 0, 72, 12)), "bottom": (60.0, 75.5, _rect_mask(W, H, 48, 65, 72, H))}
    for name, (cx, cy, m) in edges.items():
        cases.append((f"clipped_{name}", noise, m, clear, [(cx, cy, 12.0, 20.0, 0.5)], "changes"))
    cases.append(("outside", noise, np.full((H, W), 255, np.uint8), clear, [(-40.0, 30.0, 12.0, 20.0, 0.5), (60.0, 200.0, 12.0, 20.0, 0.5),
                                                                          (400.0, 30.0, 12.0, 20.0, 0.5), (60.0, -13.5, 12.0, 20.0, 0.5)], "nothing"))
    cases.append(("ring_leaves_canvas", noise, _rect_mask(W, H, 0, 0, 20, 20), clear, [(8.0, 8.0, 12.0, 60.0, 0.5)], "changes"))
    cases.append(("all_in_hole", noise, _rect_mask(W, H, 20, 0, 110, H), clear, [(65.0, 38.0, 12.0, 16.0, 0.5)], "nothing"))
    rng = np.random.default_rng(14)
    vals = np.where(hole > 0, rng.choice(np.array([1, 200, 255], np.uint8), (H, W)), 0).astype(np.uint8)
    cases.append(("mask_values_1_200_255", noise, vals, clear, [(64.0, 38.0, 14.0, 24.0, 0.5)], "changes"))
    cases.append(("five_overlapping_dabs", ramp_with_noise(W, H), hole, mixed, FIVE_DABS, "changes"))
    return cases + _instant_cases_second_canvas()


CHAIN_65 = "chain_of_65_overlapping_dabs"


def instant_canvas(name):
    """(w, h) of a case of instant_cases()"""
    return (SWEEP2_W, SWEEP2_H) if name in ("walk_300_dabs", "two_far_corners", CHAIN_65) else (SWEEP_W, SWEEP_H)


def walk_dabs():
    """300 small dabs from the left edge to the right one, zigzagging over the whole height: the union of their pixel boxes is the canvas but for a few pixels;
    five sample radii (the host's ring table), every hardness"""
    radii = (9.0, 12.5, 7.0, 15.0, 10.25)
    return [(1.5 + k * (SWEEP2_W - 3.0) / 299.0, 1.25 + float(k * 37 % (SWEEP2_H - 2)), 2.0 + 0.5 * (k % 4), radii[k % 5], (k % 5) * 0.25) for k in range(300)]


def chain_dabs():
    """65 dabs 3.5 pixels apart with brush radius 9 and sample radius 16: dab k's brush covers most of what dab k - 1 wrote in `out`, and its sample ring reaches
    across the pixels of the dabs before it (the ring reads src, as the reference's does, so the list must equal the single calls in order)"""
    return [(20.0 + 3.5 * k, 100.0 + 6.0 * np.sin(0.4 * k).item(), 9.0, 16.0 if k % 2 else 13.0, (k % 3) * 0.4) for k in range(65)]


def _instant_cases_second_canvas():
    W, H = SWEEP2_W, SWEEP2_H
    y, x = np.mgrid[0:H, 0:W]
    src = ramp_with_noise(W, H, 16)
    squares = np.where((x // 6 + y // 6) % 2 == 0, 255, 0).astype(np.uint8)      # painted-over squares between source squares, all over the canvas
    mixed = _noise(W, H, 17)
    mixed[..., 3] = np.random.default_rng(18).choice(np.array([0, 64, 128, 255], np.uint8), (H, W))
    band = _rect_mask(W, H, 0, 84, W, 118)
    band[(x + y) % 7 == 0] = 0                                                 # source pixels inside the chain's band
    return [("walk_300_dabs", src, squares, mixed, walk_dabs(), "changes"),
            ("two_far_corners", src, squares, np.zeros_like(src), [(5.0, 4.5, 8.0, 14.0, 0.5), (W - 6.0, H - 5.5, 8.0, 14.0, 0.2)], "changes"),
            (CHAIN_65, src, band, mixed, chain_dabs(), "changes")]


FIVE_DABS = [(56.0, 32.0, 9.0, 18.0, 0.5), (61.5, 35.25, 9.0, 24.0, 0.2), (67.0, 38.0, 10.0, 18.0, 0.9), (72.25, 41.0, 8.0, 24.0, 0.5),
             (64.0, 36.0, 12.0, 18.0, 0.0)]


def ramp_with_noise(w, h, seed=15):
    img = _ramp(w, h).astype(int)
    img[..., :3] += np.random.default_rng(seed).integers(-12, 13, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- PatchMatch sweep

def _palette(w, h, seed):
    """3 colours in 5 x 5 blocks: SSD ties occur"""
    colours = np.array([(220, 40, 40, 255), (40, 200, 60, 255), (30, 60, 210, 255)], np.uint8)
    idx = np.random.default_rng(seed).integers(0, 3, ((h + 4) // 5, (w + 4) // 5))
    return colours[np.kron(idx, np.ones((5, 5), int))[:h, :w]]


def _gradnoise(w, h, seed):
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 4), int)
    img[..., 0] = x * 3 + y
    img[..., 1] = 255 - y * 4
    img[..., 2] = (x + y) * 2
    img[..., :3] += np.random.default_rng(seed).integers(-20, 21, (h, w, 3))
    img[..., 3] = 255
    return np.clip(img, 0, 255).astype(np.uint8)


def _hole(shape, w, h):
    m = np.zeros((h, w), np.uint8)
    if shape == "corner":
        m[:12, :16] = 255
    elif shape == "edge":
        m[h - 5:, 10:50] = 255
    elif shape == "two":
        m[8:17, 6:18] = 255
        m[25:35, 40:52] = 255
    elif shape == "L":
        m[10:34, 20:26] = 255
        m[28:34, 26:42] = 255
    elif shape == "ring":
        m[12:30, 18:36] = 255
        m[17:25, 23:31] = 0
    elif shape == "ring_pixel_island":
        m[14:25, 20:31] = 255
        m[19, 25] = 0
    elif shape == "blob":
        rng = np.random.default_rng(21)
        y, x = np.mgrid[0:h, 0:w]
        ang = np.arctan2(y - 22.0, x - 30.0)
        rad = 7.0 + 2.0 * np.sin(3 * ang) + 1.5 * np.cos(5 * ang + 1.0)
        inside = np.hypot(x - 30.0, y - 22.0) < rad
        m[inside] = rng.choice(np.array([1, 200, 255], np.uint8), int(inside.sum()))
    elif shape == "deep":
        m[15:27, 30:42] = 255          # 12 x 12: 6 peels
    elif shape == "small":
        m[30:33, 20:23] = 255
    elif shape in ("antidiag_band", "maindiag_band"):       # three diagonals wide, clipped to 45 columns
        y, x = np.mgrid[0:h, 0:w]
        k = x + y - 88 if shape == "antidiag_band" else x - y - 5
        m[(k >= 0) & (k <= 2) & (x >= 25) & (x < 70)] = 255
    elif shape == "stripe":                                 # 2 x 540: every pixel is a boundary pixel of the first peel
        m[h // 2 - 1:h // 2 + 1, 50:590] = 255
    elif shape == "far_corners":                            # two 3 x 3 holes
        m[3:6, 4:7] = 255
        m[h - 7:h - 4, w - 8:w - 5] = 255
    elif shape == "both_corners":                           # 6 x 6 in the first corner and in the last: the box is the canvas
        m[:6, :6] = 255
        m[h - 6:, w - 6:] = 255
    elif shape == "full_cross":                             # one full row band and one full column band
        m[h // 2 - 1:h // 2 + 2, :] = 255
        m[:, w // 2 - 1:w // 2 + 2] = 255
    elif shape == "one_pixel":
        m[h // 2, w // 2] = 255
    elif shape == "two_pixels":
        m[h // 2, w // 2] = 255
        m[h // 2 - 1, w // 2] = 200
    else:
        raise ValueError(shape)
    return m


PATCHMATCH_SWEEP = [  # (canvas, hole shape, content, patch size, iterations)
    ((61, 45), "corner", "palette", 3, 3), ((61, 45), "edge", "gradnoise", 4, 6), ((61, 45), "two", "palette", 5, 3), ((61, 45), "L", "gradnoise", 7, 6),
    ((61, 45), "ring", "palette", 9, 3), ((61, 45), "blob", "gradnoise", 11, 6), ((61, 45), "deep", "palette", 5, 6), ((61, 45), "deep", "gradnoise", 3, 3),
    ((64, 64), "corner", "gradnoise", 11, 3), ((64, 64), "edge", "palette", 9, 6), ((64, 64), "two", "gradnoise", 7, 3), ((64, 64), "L", "palette", 4, 3),
    ((64, 64), "ring", "gradnoise", 5, 6), ((64, 64), "blob", "palette", 3, 6), ((64, 64), "deep", "gradnoise", 7, 3),
    ((64, 64), "small", "bw_split", 11, 3), ((64, 64), "ring_pixel_island", "palette", 3, 3), ((61, 45), "ring_pixel_island", "gradnoise", 1, 6)]


# What the device code does in block-sized pieces (paintfe_amd/csrc/k_inpaint.hip); the edge cases are sized against these
PM_PASS_WAVES = 16           # pm_pass_kernel: `for (i = lo + wave; i < hi; i += 16u)` — boundary pixels of one anti-diagonal handled per round
PM_BLOCK_THREADS = 1024      # pm_bucket_kernel: `i += 1024u` / `base += 1024u` (boundary pixels and diagonals per turn); pm_scan_kernel: `base += 1024u` (blocks)
PM_COMPACT_ELEMS = 1024      # compact_flags / pm_count_kernel: `blockIdx.x * 1024u` — rectangle elements per compaction block

PATCHMATCH_EDGES = [  # (canvas, hole shape, content, patch size, iterations); the edge each crosses is spelt in EDGE_CONDITIONS
    ((97, 83), "antidiag_band", "gradnoise", 5, 3), ((97, 83), "antidiag_band", "palette", 7, 6),
    ((97, 83), "maindiag_band", "palette", 3, 6), ((97, 83), "maindiag_band", "gradnoise", 9, 3),
    ((640, 24), "stripe", "gradnoise", 5, 3),
    ((600, 520), "far_corners", "palette", 3, 3),
    ((1100, 960), "both_corners", "palette", 7, 3),
    ((70, 50), "full_cross", "gradnoise", 7, 6),
    ((5, 4), "one_pixel", "gradnoise", 11, 3), ((5, 4), "one_pixel", "gradnoise", 7, 6), ((3, 9), "two_pixels", "gradnoise", 7, 3),
    ((10, 9), "one_pixel", "palette", 11, 6), ((8, 7), "two_pixels", "gradnoise", 9, 3)]

# Patch 11 wants min_valid = 121 / 4 = 30 valid patch pixels and a 5 x 4 canvas has 20: every SSD is F32_MAX and the reference leaves the pixel unfilled.  The
# case is kept for what it runs (a query whose 121 slots are all clipped, the unfilled path); the cases after it are the ones that fill.
def _pick(specs, canvas, shape, patch_size=None):
    """the one spec of a list with this canvas and hole shape (and patch size, where two share them)"""
    found = [s for s in specs if s[0] == canvas and s[1] == shape and patch_size in (None, s[3])]
    assert len(found) == 1, (canvas, shape, patch_size, found)
    return found[0]


NEVER_FILLABLE = _pick(PATCHMATCH_EDGES, (5, 4), "one_pixel", 11)

# a huge box and source list, then a small canvas, then a long boundary list: what test_gpu_inpaint.py runs on one context
GEOMETRY_SEQUENCE = [_pick(PATCHMATCH_EDGES, (600, 520), "far_corners"), _pick(PATCHMATCH_SWEEP, (61, 45), "deep", 5), _pick(PATCHMATCH_EDGES, (640, 24), "stripe")]


@functools.lru_cache(maxsize=None)
def patchmatch_expected(spec):
    """the model's (image, counters, peel trace) of a case, computed once per session and shared read-only by the host and the GPU tests"""
    trace = []
    img, k = M.patchmatch(*patchmatch_case(spec), trace=trace)
    img.setflags(write=False)
    return img, k, trace


def patchmatch_case(spec):
    """(src, mask, patch_size, iterations); the hole's pixels in src are garbage the fill must not depend on where the reference does not"""
    (w, h), shape, content, ps, iters = spec
    if content == "palette":
        img = _palette(w, h, 31)
    elif content == "gradnoise":
        img = _gradnoise(w, h, 32)
    else:
        img = np.zeros((h, w, 4), np.uint8)
        img[:, w // 2:, :3] = 255
        img[..., 3] = 255
    m = _hole(shape, w, h)
    img = img.copy()
    img[m > 0] = np.random.default_rng(33).integers(0, 256, (int((m > 0).sum()), 4), dtype=np.uint8)
    return img, m, ps, iters


def patchmatch_id(spec):
    (w, h), shape, content, ps, iters = spec
    return f"{w}x{h}-{shape}-{content}-p{ps}-i{iters}"
