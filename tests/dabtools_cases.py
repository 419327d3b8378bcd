"""Inputs of the dab-list tools' tests (clone stamp, heal ring, pencil), shared by tests/test_dabtools_model_host.py (no GPU: the model against a scalar
transcription, the branches each case reaches, the fragile-pixel cap) and tests/test_gpu_dabtools.py (the kernels against the model).  The expected images are
computed once per case and cached; callers do not modify them.

Canvases sit at the chunk grid's edges: 131 x 70 is 3 x 2 chunks, ragged right and bottom; 64 x 64 exactly one; 65 x 1 and 1 x 130 one pixel into a second
chunk; 1 x 1.  A stroke is a first circle left of the canvas, two or three line segments from the line helper's model (fractional centres, one pixel apart, so
neighbouring dabs overlap almost entirely; one segment leaves the canvas and the helper drops its tail), single circles beyond the other three edges, and a
dab at (64, 64) whose box straddles four chunks where the canvas has them."""
import functools

import numpy as np

from . import dabtools_model as M

CANVASES = [(131, 70), (64, 64), (65, 1), (1, 130), (1, 1)]
BIG = CANVASES[0]
# size, hardness, anti_aliased, offset: every size 1 / 2 / 7 / 41, hardness 0 / 0.5 / 1, both edge modes and every offset (the last two leave the canvas) occur
CLONE_BIG = [(1, 0.0, True, (0, 0)), (2, 0.5, False, (17.5, -9.5)), (7, 1.0, True, (17.5, -9.5)), (7, 0.0, False, (200, 0)), (41, 0.5, True, (-200, 0)),
             (41, 1.0, False, (0, 0)), (41, 0.0, True, (17.5, -9.5)), (2, 1.0, True, (-200, 0)), (1, 0.5, False, (200, 0)), (7, 0.5, True, (0, 0))]
CLONE_SMALL = [(7, 0.5, True, (0, 0)), (41, 1.0, False, (17.5, -9.5)), (2, 0.0, True, (0, 0))]
# size, hardness, sample_radius.  The reference's angle seed x * 1619 + y * 3929 is far below 2^32 on canvases this small, so every pixel's angle offset is
# below 1e-3 rad and the ring's 24 angles sit that close to multiples of 15 degrees: cos / sin of the four axis samples are +-1 or a few ulps off.  A
# half-integer radius (6.5; 0.75 * 30 = 22.5) then puts x +- radius on or within a few f32 spacings of a rounding tie, and one ulp of cos decides which way
# it goes.  Under the model's definition such a pixel is fragile whichever stroke covers it: at 30 that is every pixel of every canvas here, at 6.5 the
# pixels whose seed is below about 3e5 (most of 131 x 70, all of 65 x 1), at 1 only pixel (0, 0) (angle offset exactly 0: cos 60 degrees * 1 is the tie),
# which is already 1.5 % of a 65 x 1 canvas.  So the heal cases come in two zones:
#   free   the fragile pixels the stroke covers are capped at 1 % (test_dabtools_model_host.py): sample_radius 1 under the full stroke where the canvas is
#          large enough, and strokes confined to where the seed is large or away from (0, 0) — the bottom right of 131 x 70 for 6.5, where the ring still
#          leaves the canvas at the right and bottom edges; the lower part of 1 x 130; the right part of 65 x 1;
#   tie    the full stroke where no stroke can stay under the cap — 30 everywhere, with the ring leaving the canvas near every edge; 6.5 over the whole
#          canvas; the one-pixel-wide canvases from their first pixel: compared like any other case (exactly where not fragile, alpha alone where fragile),
#          the fraction reported, no cap.
HEAL_FULL = {BIG: [(1, 0.0, 1.0), (41, 1.0, 1.0), (7, 0.5, 1.0), (2, 0.5, 1.0)], (64, 64): [(7, 0.5, 1.0), (41, 1.0, 1.0), (2, 0.0, 1.0)], (1, 1): [(7, 0.5, 1.0), (41, 1.0, 30.0)]}
HEAL_CORNER = {BIG: [(2, 0.5, 6.5), (7, 1.0, 6.5), (7, 0.0, 6.5), (1, 0.0, 6.5)], (1, 130): [(7, 0.5, 6.5), (41, 1.0, 1.0), (2, 0.0, 1.0)],
               (65, 1): [(7, 0.5, 1.0), (41, 1.0, 1.0), (2, 0.0, 1.0)]}
HEAL_TIE = {BIG: [(41, 0.0, 6.5), (41, 0.5, 30.0), (7, 1.0, 30.0), (2, 0.5, 6.5), (2, 1.0, 30.0), (1, 0.0, 30.0)], (64, 64): [(7, 0.5, 6.5), (41, 1.0, 30.0)],
            (65, 1): [(7, 0.5, 6.5), (41, 1.0, 30.0), (2, 0.0, 1.0)], (1, 130): [(7, 0.5, 1.0), (41, 1.0, 30.0), (2, 1.0, 30.0)]}


def source(w, h, seed=1):
    """the layer: random colours, alpha random with an alpha-0 and an alpha-255 region"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    img[..., 3][(xs + 2 * ys) % 11 < 3] = 0
    img[..., 3][(3 * xs + ys) % 13 < 5] = 255
    return img


def selection(w, h):
    """a selection with holes: mostly 255, some 0, a few low values (any non-zero byte passes)"""
    rng = np.random.default_rng(31 * w + h)
    sel = np.full((h, w), 255, np.uint8)
    r = rng.random((h, w))
    sel[r < 0.25] = 0
    sel[(r >= 0.25) & (r < 0.3)] = 1
    sel[(r >= 0.3) & (r < 0.35)] = 128
    return sel


@functools.lru_cache(maxsize=None)
def segments(w, h):
    """the stroke as a list of pieces, each an (n, 2) f32 array: the first circle, the line segments, the circles beyond the edges"""
    a, b, c, d = (-2.5, h * 0.3 + 0.25), (w * 0.45 + 0.3, h * 0.55 + 0.25), (w + 3.0, h * 0.2), (w * 0.3 + 0.6, h * 0.9 - 0.1)
    pieces = [np.array([a], M.F), M.line_points(a, b, w, h), M.line_points(b, c, w, h), M.line_points(b, d, w, h),
              np.array([(w + 2.5, h * 0.5), (w * 0.5, -2.5), (w * 0.5 + 0.5, h + 2.5)], M.F)]
    if w > 64 and h > 64:
        pieces.append(np.array([(64.0, 64.0)], M.F))
    return [p for p in pieces if len(p)]


@functools.lru_cache(maxsize=None)
def corner_segments(w, h):
    """the same kind of stroke confined to the large-seed corner: 131 x 70's bottom right, 1 x 130's lower part"""
    if (w, h) == BIG:
        a, b, c, d = (133.5, 60.25), (126.3, 66.2), (104.7, 60.4), (120.2, 74.0)
    elif (w, h) == (65, 1):
        a, b, c, d = (68.5, 0.25), (60.3, 0.2), (30.7, 0.4), (45.2, 3.0)
    else:
        a, b, c, d = (3.5, 100.25), (0.3, 92.5), (0.6, 120.4), (0.2, 134.0)
    return [p for p in (np.array([a], M.F), M.line_points(a, b, w, h), M.line_points(b, c, w, h), M.line_points(c, d, w, h)) if len(p)]


def points(w, h, stroke="full"):
    return np.concatenate(segments(w, h) if stroke == "full" else corner_segments(w, h))


def segments_of(case):
    return segments(case["w"], case["h"]) if case.get("stroke", "full") == "full" else corner_segments(case["w"], case["h"])


def points_of(case):
    return points(case["w"], case["h"], case.get("stroke", "full"))


def _names():
    clone, heal = {}, {}
    for (w, h) in CANVASES:
        big = (w, h) == BIG
        for s in (CLONE_BIG if big else CLONE_SMALL):
            for sel in (False, True):
                for seeded in ((False, True) if big else (True,)):
                    name = f"{w}x{h}-size{s[0]}-hard{s[1]}-{'aa' if s[2] else 'hard-edge'}-off{s[3][0]},{s[3][1]}{'-sel' if sel else ''}{'-seeded' if seeded else ''}"
                    clone[name] = dict(w=w, h=h, tool=dict(size=s[0], hardness=s[1], anti_aliased=s[2], offset=s[3]), sel=sel, seeded=seeded)
        for table, stroke, zone in ((HEAL_FULL, "full", "free"), (HEAL_CORNER, "corner", "free"), (HEAL_TIE, "full", "tie")):
            for s in table.get((w, h), []):
                for sel in (False, True):
                    for seeded in ((False, True) if big else (True,)):
                        name = f"{w}x{h}-{stroke}-size{s[0]}-hard{s[1]}-ring{s[2]}{'-sel' if sel else ''}{'-seeded' if seeded else ''}"
                        heal[name] = dict(w=w, h=h, tool=dict(size=s[0], hardness=s[1], sample_radius=s[2]), sel=sel, seeded=seeded, stroke=stroke, zone=zone)
    return clone, heal


CLONE, HEAL = _names()
CLONE_NAMES, HEAL_NAMES = sorted(CLONE), sorted(HEAL)


def selection_of(case):
    return selection(case["w"], case["h"]) if case["sel"] else None


def seeded_preview(w, h, alpha):
    """a non-empty preview for a stroke that writes `alpha` onto an empty one: random colours everywhere; alpha one below, equal to and one above the
    stroke's, by position"""
    rng = np.random.default_rng(5 * w + 3 * h)
    pv = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    pv[..., 3] = np.clip(alpha.astype(np.int32) + (xs + ys) % 3 - 1, 0, 255).astype(np.uint8)
    return pv


@functools.lru_cache(maxsize=None)
def ring(w, h, sample_radius, flavour):
    """one Ring per layer, sample radius and flavour, shared by every case on it (it only caches)"""
    return M.Ring(source(w, h), sample_radius, flavour)


@functools.lru_cache(maxsize=None)
def clone_preview(name):
    c = CLONE[name]
    w, h = c["w"], c["h"]
    empty = np.zeros((h, w, 4), np.uint8)
    if not c["seeded"]:
        return empty
    return seeded_preview(w, h, M.clone_stroke(c["tool"], source(w, h), empty, selection_of(c), points(w, h))[0][..., 3])


@functools.lru_cache(maxsize=None)
def clone_expected(name):
    """(the preview after the stroke, the dirty box, the branch counts)"""
    c = CLONE[name]
    stats = M.new_stats()
    out, dirty = M.clone_stroke(c["tool"], source(c["w"], c["h"]), clone_preview(name), selection_of(c), points(c["w"], c["h"]), stats)
    return out, dirty, stats


@functools.lru_cache(maxsize=None)
def heal_preview(name):
    c = HEAL[name]
    w, h = c["w"], c["h"]
    empty = np.zeros((h, w, 4), np.uint8)
    if not c["seeded"]:
        return empty
    return seeded_preview(w, h, M.heal_stroke(c["tool"], ring(w, h, c["tool"]["sample_radius"], "device"), empty, selection_of(c), points_of(c))[0][..., 3])


@functools.lru_cache(maxsize=None)
def heal_expected(name, flavour="device"):
    """(the preview after the stroke, the dirty box, the branch counts, the fragile mask, the in-canvas sample count per pixel)"""
    c = HEAL[name]
    w, h = c["w"], c["h"]
    r = ring(w, h, c["tool"]["sample_radius"], flavour)
    stats = M.new_stats()
    out, dirty = M.heal_stroke(c["tool"], r, heal_preview(name), selection_of(c), points_of(c), stats)
    return out, dirty, stats, r.fragile.copy(), r.count.copy()


# ---- pencil: colour, the segments' end points (start, end), selection; every canvas -------------------------------------------------------------------------------
def pencil_lines(w, h):
    """steep, shallow, reversed, one leaving the canvas, one of a single cell"""
    return [((1.5, 0.5), (w * 0.2 + 2.0, h - 0.5)), ((0.5, h * 0.5), (w - 0.5, h * 0.6)), ((w - 1.5, h - 1.5), (2.5, 1.5)), ((w * 0.5, h * 0.5), (w + 6.5, -4.5)),
            ((w * 0.25, h * 0.25), (w * 0.25 + 0.2, h * 0.25 + 0.2))]


PENCIL_COLORS = {"opaque": (0.2, 0.4, 0.6, 1.0), "half": (1.0, 0.0, 0.999, 0.5), "tie": (0.3, 0.3, 0.3, 128.0 / 255.0)}


def _pencil_names():
    out = {}
    for (w, h) in CANVASES:
        for cname in PENCIL_COLORS:
            for sel in (False, True):
                out[f"{w}x{h}-{cname}{'-sel' if sel else ''}"] = dict(w=w, h=h, color=PENCIL_COLORS[cname], sel=sel)
    return out


PENCIL = _pencil_names()
PENCIL_NAMES = sorted(PENCIL)


@functools.lru_cache(maxsize=None)
def pencil_cell_lists(w, h):
    return [M.line_cells(a, b, w, h) for a, b in pencil_lines(w, h)]


def pencil_preview(w, h):
    """alphas 127, 128, 129 by position under random colours: one below, equal to and one above the `tie` colour's byte, and both sides of `half`"""
    rng = np.random.default_rng(9 * w + h)
    pv = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    pv[..., 3] = (127 + (xs + 2 * ys) % 3).astype(np.uint8)
    return pv


@functools.lru_cache(maxsize=None)
def pencil_expected(name):
    c = PENCIL[name]
    cells = np.concatenate(pencil_cell_lists(c["w"], c["h"]))
    stats = M.new_stats()
    out, dirty = M.pencil_cells(c["color"], pencil_preview(c["w"], c["h"]), selection_of(c), cells, stats)
    return out, dirty, stats
