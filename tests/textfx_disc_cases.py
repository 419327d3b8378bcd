"""The disc of the text styles, tap by tap, and planes on which every tap counts (tests/test_textfx_disc_host.py, tests/test_gpu_textfx_disc.py).

`disc_taps` is the reference: the maximum over every (dx, dy) that passes dilate_mask's own f32 test (effects.rs:176-207: int_radius = ceil(radius),
r_sq = radius * radius rounded once, a row is in when dy * dy <= r_sq, a tap when dx * dx + dy * dy <= r_sq), zero outside the image; the minimum is
255 - max(255 - a).  It knows nothing of row spans or window tables: the membership is a boolean matrix and every member is applied on its own, either as one
shifted slice per tap or, on a sparse plane, as one stamp of the matrix per non-zero source pixel.  The five wrong discs of WRONG edit that matrix; the host
tests use them to show that an input would notice such a disc.  Nothing here needs a device."""
import functools

import numpy as np

F = np.float32
PLANE = (200, 140)                                                   # w, h: 140 >= 2 * 64 + 3, so the clear window of every accepted radius fits
INTEGER_RADII = list(range(1, 65))
FRACTIONAL_RADII = [0.5, 1.5, 2.5, 7.3, 8.01, 8.5, 15.9, 31.5, 63.2, 63.99]
SWEEP = sorted(INTEGER_RADII + FRACTIONAL_RADII)                     # every halo 1 .. 64 and both tile shapes
HOST_RADII = [0.5, 1, 2.5, 7.3, 8, 8.01, 31.5, 32, 50, 63.2, 64]     # disc_taps against the model's two forms
SALT_RADII = [1, 2, 5, 8, 9, 16, 17, 33, 50, 64]
SEAM_SIZES = [(67, 5), (131, 70)]                                    # shorter than the halo, odd width | three tiles across, two down
SEAM_RADII = [2, 8, 9, 64]
THIN_SIZES = [(1, 1), (1, 70), (64, 1)]
THIN_RADII = [1, 64]
SMALL_TILE_REACH = 8                                                 # the disc kernel's 64 x 32 tile up to this halo, 64 x 64 above it
BORDER_VALUES = [200, 150, 100, 50, 40, 30, 20, 10]                  # the four corners, then the four mid-edges


def reach_of(radius):
    return int(np.ceil(F(radius)))


# ---- the disc, tap by tap ------------------------------------------------------------------------------------------------------------------------------------------
def disc_member(radius):
    """(2 R + 3, 2 R + 3) bool with R = ceil(radius): [dy + R + 1, dx + R + 1] is True where dilate_mask takes the tap (dx, dy).  The margin of one
    is never a member; it is there for WRONG's extra tap and is the `clear` window"""
    radius = F(radius)
    R = reach_of(radius)
    r_sq = F(radius * radius)
    d = np.arange(-R, R + 1).astype(F)
    sq = (d * d).astype(F)                                           # dx * dx and dy * dy: one f32 product each
    inner = ((sq[None, :] + sq[:, None]).astype(F) <= r_sq) & (sq[:, None] <= r_sq)
    member = np.zeros((2 * R + 3, 2 * R + 3), bool)
    member[1:-1, 1:-1] = inner
    return member


def taps_max(plane, member):
    """out[y, x] = max of plane[y + dy, x + dx] over the members (dx, dy), zero outside the image"""
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape
    m = member.shape[0] // 2
    ys, xs = np.nonzero(plane)
    dys, dxs = np.nonzero(member)
    if len(ys) <= len(dys):                                          # a source at s reaches the outputs s - tap: the matrix turned by 180 degrees, stamped at s
        stamp = np.ascontiguousarray(member[::-1, ::-1]).astype(np.uint8)
        out = np.zeros((h + 2 * m, w + 2 * m), np.uint8)
        for y, x in zip(ys, xs):
            win = out[y:y + 2 * m + 1, x:x + 2 * m + 1]
            np.maximum(win, stamp * plane[y, x], out=win)
        return np.ascontiguousarray(out[m:m + h, m:m + w])
    padded = np.pad(plane, m)
    out = np.zeros((h, w), np.uint8)
    for dy, dx in zip(dys - m, dxs - m):
        np.maximum(out, padded[m + dy:m + dy + h, m + dx:m + dx + w], out=out)
    return out


def disc_taps(plane, radius, take_min=False, wrong=None):
    """the disc's maximum (take_min: minimum) of a u8 plane; `wrong`: a function of WRONG applied to the membership first (None from it: nothing to drop at
    this radius, and None is returned)"""
    member = disc_member(radius)
    if wrong is not None:
        member = wrong(member)
        if member is None:
            return None
    plane = np.asarray(plane, np.uint8)
    return 255 - taps_max(255 - plane, member) if take_min else taps_max(plane, member)


# ---- five wrong discs ------------------------------------------------------------------------------------------------------------------------------------------------
def _row_ends(member):
    """[(row index, first column, last column)] of the rows that hold a tap"""
    ends = []
    for i in range(member.shape[0]):
        cols = np.nonzero(member[i])[0]
        if len(cols):
            ends.append((i, int(cols[0]), int(cols[-1])))
    return ends


def drop_right_of_row_0(member):
    out, m = member.copy(), member.shape[0] // 2
    out[m, np.nonzero(member[m])[0][-1]] = False
    return out


def drop_right_of_every_row(member):
    out = member.copy()
    for i, _, last in _row_ends(member):
        out[i, last] = False
    return out


def drop_last_row(member):
    """the disc's last row: dy = +ceil(r) at an integer radius, the largest dy that passes dy * dy <= r_sq otherwise"""
    out = member.copy()
    out[_row_ends(member)[-1][0]] = False
    return out


def drop_both_ends_of_long_rows(member):
    """rows of 16 taps and more, the ones the kernel reads from its 16- and 64-column tables; None where the disc has none (ceil(r) < 8)"""
    out, any_row = member.copy(), False
    for i, first, last in _row_ends(member):
        if last - first + 1 >= 16:
            out[i, first] = out[i, last] = False
            any_row = True
    return out if any_row else None


def extra_right_of_rim_rows(member):
    """one tap more right of the rows |dy| = ceil(r) - 1 (at ceil(r) = 1 that is the row dy = 0)"""
    out, m = member.copy(), member.shape[0] // 2
    R = m - 1
    for i in {m - (R - 1), m + (R - 1)}:
        out[i, np.nonzero(member[i])[0][-1] + 1] = True
    return out


WRONG = {"rightmost tap of the dy = 0 row dropped": drop_right_of_row_0,
         "rightmost tap of every row dropped": drop_right_of_every_row,
         "last disc row dropped": drop_last_row,
         "both end taps of every row of length >= 16 dropped": drop_both_ends_of_long_rows,
         "one extra tap right of the rows |dy| = ceil r - 1": extra_right_of_rim_rows}
NEVER_SKIPPED = ["rightmost tap of every row dropped", "last disc row dropped"]


# ---- what build_disc makes of a row ----------------------------------------------------------------------------------------------------------------------------------
def span_word(length):
    """(level, reads) of a span of `length` columns by build_disc's rule: the largest window of 4^level columns, level <= 3, that fits the span, and
    ceil(length / window) reads of it"""
    level = 0
    while level < 3 and 4 ** (level + 1) <= length:
        level += 1
    return level, -(-length // 4 ** level)


def row_lengths(radius):
    return [last - first + 1 for _, first, last in _row_ends(disc_member(radius))]


# ---- planes ----------------------------------------------------------------------------------------------------------------------------------------------------------
def clear_centres(radius):
    """(x, y) of the lone pixel: around the corners of the 64 x 32 tiles at the small halos, around the corner (64, 64) of both tile shapes above"""
    return [(63, 31), (64, 32), (63, 63), (64, 64)] if reach_of(radius) <= SMALL_TILE_REACH else [(66, 66)]


def border_pixels(w, h):
    at = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2), (w - 1, h // 2), (w // 2, h - 1)]
    return list(zip(at, BORDER_VALUES))


@functools.lru_cache(maxsize=None)
def clear(radius, k=0):
    """one pixel of 255 at clear_centres(radius)[k] alone in its (2 ceil(r) + 3)^2 window, and eight lower values on the border"""
    w, h = PLANE
    plane = np.zeros((h, w), np.uint8)
    for (x, y), v in border_pixels(w, h):
        plane[y, x] = v
    x, y = clear_centres(radius)[k]
    plane[y, x] = 255
    plane.setflags(write=False)
    return plane


def holes(radius, k=0):
    return 255 - clear(radius, k)


@functools.lru_cache(maxsize=None)
def salt(size=PLANE, seed=3):
    """about 3 % of the pixels non-zero, with random values: overlapping discs of different heights"""
    w, h = size
    rng = np.random.default_rng(seed + 1000 * w + h)
    plane = np.where(rng.random((h, w)) < 0.03, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    plane.setflags(write=False)
    return plane


def pepper(size=PLANE, seed=3):
    return 255 - salt(size, seed)


@functools.lru_cache(maxsize=None)
def noise(size, seed=5):
    """every pixel random: for the images of one row or one column, where 3 % would be nothing"""
    w, h = size
    plane = np.random.default_rng(seed + 1000 * w + h).integers(0, 256, (h, w), dtype=np.uint8)
    plane.setflags(write=False)
    return plane


def source(kind, radius, take_min, k=0, size=PLANE):
    """the plane of a kind: "clear" (holes for the minimum) | "salt" (its complement for the minimum) | "noise" (the same plane for both)"""
    if kind == "clear":
        return holes(radius, k) if take_min else clear(radius, k)
    if kind == "salt":
        return pepper(size) if take_min else salt(size)
    return noise(size)


@functools.lru_cache(maxsize=None)
def expected(kind, radius, take_min, k=0, size=PLANE):
    """disc_taps of source(...), shared and read only"""
    plane = source(kind, radius, take_min, k, size)
    out = disc_taps(plane, radius, take_min)
    out.setflags(write=False)
    return out
