"""The dab-list tools' CPU model (tests/dabtools_model.py) held to what it restates, without a GPU:

* against an independent scalar transcription of clone_stamp_circle / heal_circle / draw_pixel_and_get_bounds (ref: src/ui/panels/tools/behavior/raster/
  clone_heal.rs) — pixel by pixel, dab by dab, nothing cached, nothing hoisted — which proves that evaluating a pixel's colour once equals the serial loop;
* against hand-derived answers for the corners the issue names;
* the library's two line helpers against the model, through ctypes;
* the cases of tests/dabtools_cases.py reach the branches they are built for, the two libm flavours agree at every pixel that is not fragile, and the
  fragile pixels stay under the cap where the cases are built to (the counts are in profiles/dab_tools.md)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from . import dabtools_cases as DC
from . import dabtools_model as M
from .shape_model import Libm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID = 0, -1


# ---- the scalar transcription -----------------------------------------------------------------------------------------------------------------------------------------
def rs_round(v):
    v = float(v)
    return math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)       # exact on the f64 image of an f32: half away from zero


def rs_u8(v):
    v = float(v)
    return 0 if v != v else int(max(0.0, min(255.0, math.trunc(v))))


def rs_clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def scalar_brush_alpha(dist, radius, hardness, aa):
    if radius <= 0:
        return F(0)
    safe = rs_clamp(F(hardness), F(0), F(1))
    t = rs_clamp(dist / radius, F(0), F(1))
    falloff = t * t * (F(3) - F(2) * t)
    material = F(1) + (safe - F(1)) * falloff
    if aa:
        e0, e1 = radius + F(0.5), radius - F(0.5)
        if dist <= e1:
            cov = F(1)
        elif dist >= e0:
            cov = F(0)
        else:
            x = rs_clamp((dist - e0) / (e1 - e0), F(0), F(1))
            cov = x * x * (F(3) - F(2) * x)
    else:
        cov = F(1) if dist <= radius else F(0)
    return material * cov


def scalar_clone_circle(tool, src, pv, sel, cx, cy):
    h, w = pv.shape[:2]
    cx, cy, radius = F(cx), F(cy), F(tool["size"]) / F(2)
    x0, x1, y0, y1 = M.dab_box(cx, cy, radius, w, h)
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            if sel is not None and sel[y, x] == 0:
                continue
            dx, dy = F(x) - cx, F(y) - cy
            dist = np.sqrt(dx * dx + dy * dy)
            if dist > radius:
                continue
            geom = scalar_brush_alpha(dist, radius, tool["hardness"], tool["anti_aliased"])
            if geom < F(0.01):
                continue
            sx, sy = rs_round(F(x) + F(tool["offset"][0])), rs_round(F(y) + F(tool["offset"][1]))
            if sx < 0 or sx >= w or sy < 0 or sy >= h:
                continue
            sp = [F(v) / F(255) for v in src[sy, sx]]
            alpha = geom * sp[3]
            if alpha >= F(pv[y, x, 3]) / F(255):
                pv[y, x] = [rs_u8(sp[0] * F(255)), rs_u8(sp[1] * F(255)), rs_u8(sp[2] * F(255)), rs_u8(alpha * F(255))]


def scalar_heal_circle(tool, src, pv, sel, cx, cy, libm):
    h, w = pv.shape[:2]
    cx, cy, radius, sr = F(cx), F(cy), F(tool["size"]) / F(2), F(tool["sample_radius"])
    x0, x1, y0, y1 = M.dab_box(cx, cy, radius, w, h)
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            if sel is not None and sel[y, x] == 0:
                continue
            dx, dy = F(x) - cx, F(y) - cy
            dist = np.sqrt(dx * dx + dy * dy)
            if dist > radius:
                continue
            t = rs_clamp(dist / radius, F(0), F(1))
            hard_t = rs_clamp(F(tool["hardness"]) * F(0.9) + F(0.1), F(0), F(1))
            if t < hard_t:
                geom = F(1)
            else:
                s = (t - hard_t) / (F(1) - hard_t + F(1e-6))
                geom = F(1) - s * s * (F(3) - F(2) * s)
            if geom < F(0.01):
                continue
            seed = (x * 1619 + y * 3929) & 0xFFFFFFFF
            angle_offset = F(np.uint32(seed)) / F(4294967296.0) * M.TAU
            sums, count = [F(0), F(0), F(0)], F(0)
            for i in range(24):
                angle = angle_offset + (F(i) / F(24)) * M.TAU
                c, s_ = libm.cos(np.array([angle], F))[0], libm.sin(np.array([angle], F))[0]
                for rr in (sr * F(0.75), sr):
                    sx, sy = rs_round(F(x) + c * rr), rs_round(F(y) + s_ * rr)
                    if sx < 0 or sx >= w or sy < 0 or sy >= h:
                        continue
                    for k in range(3):
                        sums[k] = sums[k] + F(src[sy, sx, k])
                    count = count + F(1)
            if count < F(1):
                continue
            if geom >= F(pv[y, x, 3]) / F(255):
                pv[y, x] = [rs_u8(sums[0] / count), rs_u8(sums[1] / count), rs_u8(sums[2] / count), rs_u8(geom * F(255))]


TINY_W, TINY_H = 13, 9
TINY_POINTS = [(-1.5, 3.25), (2.3, 3.9), (3.1, 4.4), (3.9, 4.9), (11.6, 7.7), (12.4, 8.2), (6.0, -1.0), (6.5, 4.5), (6.5, 4.5)]


def tiny_inputs(seeded):
    src, sel = DC.source(TINY_W, TINY_H, seed=3), DC.selection(TINY_W, TINY_H)
    pv = np.zeros((TINY_H, TINY_W, 4), np.uint8)
    if seeded:
        rng = np.random.default_rng(4)
        pv = rng.integers(0, 256, pv.shape, dtype=np.uint8)
        pv[..., 3] = rng.choice(np.array([0, 1, 100, 128, 200, 254, 255], np.uint8), pv.shape[:2])
    return src, sel, pv


@pytest.mark.parametrize("seeded", [False, True], ids=["empty", "seeded"])
@pytest.mark.parametrize("use_sel", [False, True], ids=["no-sel", "sel"])
@pytest.mark.parametrize("size,hardness,aa,offset", [(5, 0.5, True, (2.5, -1.5)), (3, 0.0, False, (-0.5, 0.5)), (9, 1.0, True, (0, 0)), (1, 0.3, False, (20, 0))])
def test_clone_model_equals_the_scalar_loop(size, hardness, aa, offset, use_sel, seeded):
    tool = dict(size=size, hardness=hardness, anti_aliased=aa, offset=offset)
    src, sel, pv = tiny_inputs(seeded)
    sel = sel if use_sel else None
    want = pv.copy()
    for cx, cy in TINY_POINTS:
        scalar_clone_circle(tool, src, want, sel, cx, cy)
    got, _ = M.clone_stroke(tool, src, pv, sel, TINY_POINTS)
    assert np.array_equal(got, want)
    assert offset[0] == 20 or not np.array_equal(got, pv)


@pytest.mark.parametrize("flavour", ["glibc", "device"])
@pytest.mark.parametrize("seeded", [False, True], ids=["empty", "seeded"])
@pytest.mark.parametrize("use_sel", [False, True], ids=["no-sel", "sel"])
@pytest.mark.parametrize("size,hardness,sr", [(5, 0.5, 2.0), (3, 0.0, 6.5), (9, 1.0, 1.0), (4, 0.3, 30.0)])
def test_heal_model_equals_the_scalar_loop(size, hardness, sr, use_sel, seeded, flavour):
    """the model evaluates a pixel's ring once and caches it; the scalar loop evaluates it at every visit of every dab"""
    tool = dict(size=size, hardness=hardness, sample_radius=sr)
    src, sel, pv = tiny_inputs(seeded)
    sel = sel if use_sel else None
    want, libm = pv.copy(), Libm(flavour)
    for cx, cy in TINY_POINTS:
        scalar_heal_circle(tool, src, want, sel, cx, cy, libm)
    got, _ = M.heal_stroke(tool, M.Ring(src, sr, flavour), pv, sel, TINY_POINTS)
    assert np.array_equal(got, want)
    assert sr == 30.0 or not np.array_equal(got, pv)


# ---- hand-derived answers ----------------------------------------------------------------------------------------------------------------------------------------------
def one_pixel_canvas(w=9, h=1):
    src = np.zeros((h, w, 4), np.uint8)
    for x in range(w):
        src[0, x] = (10 * x + 1, 10 * x + 2, 10 * x + 3, 255)
    return src


def test_clone_half_pixel_offsets_round_away_from_zero():
    """size 1 at (4, 0) touches pixel 4 alone (dist 0, alpha 1).  Offset +0.5: round(4.5) = 5; offset -0.5: round(3.5) = 4, not 3 — away from zero on the SUM,
    which is positive; offset -4.5: round(-0.5) = -1, off the canvas (toward zero it would have been pixel 0)"""
    src = one_pixel_canvas()
    empty = np.zeros_like(src)
    for off, want in ((0.5, 5), (-0.5, 4), (1.5, 6), (-1.5, 3)):
        out, dirty = M.clone_stroke(dict(size=1, hardness=1.0, anti_aliased=False, offset=(off, 0)), src, empty, None, [(4.0, 0.0)])
        assert tuple(out[0, 4]) == tuple(src[0, want]), off
        assert not out[0, [0, 1, 2, 3, 5, 6, 7, 8]].any() and dirty == (2, 0, 6, 1)   # the box is 3 ..= 4: (3.5 as u32, 4.5 as u32); the rect 3 - 1 .. 4 + 2
    out, _ = M.clone_stroke(dict(size=1, hardness=1.0, anti_aliased=False, offset=(-4.5, 0)), src, empty, None, [(4.0, 0.0)])
    assert not out.any()
    stats = M.new_stats()
    M.clone_stroke(dict(size=1, hardness=1.0, anti_aliased=False, offset=(-4.5, 0)), src, empty, None, [(4.0, 0.0)], stats)
    assert stats["off_canvas"] == 1 and stats["wrote"] == 0


def test_clone_tie_replaces_and_one_below_keeps():
    """source alpha 128 under a full-strength dab: alpha = 128 / 255, byte (128 / 255 * 255) as u8 = 128.  A preview alpha of 128 ties and is replaced; 129 keeps"""
    src = one_pixel_canvas()
    src[..., 3] = 128
    pv = np.zeros_like(src)
    pv[0, 4] = (9, 9, 9, 128)
    pv[0, 5] = (9, 9, 9, 129)
    tool = dict(size=1, hardness=1.0, anti_aliased=False, offset=(0, 0))
    out, _ = M.clone_stroke(tool, src, pv, None, [(4.0, 0.0), (5.0, 0.0)])
    assert tuple(out[0, 4]) == (41, 42, 43, 128) and tuple(out[0, 5]) == (9, 9, 9, 129)


def test_clone_source_alpha_zero_writes_rgb_under_alpha_zero():
    src = one_pixel_canvas()
    src[..., 3] = 0
    out, _ = M.clone_stroke(dict(size=1, hardness=1.0, anti_aliased=False, offset=(0, 0)), src, np.zeros_like(src), None, [(4.0, 0.0)])
    assert tuple(out[0, 4]) == (41, 42, 43, 0)                    # 0 >= 0 / 255: written
    pv = np.zeros_like(src)
    pv[0, 4] = (9, 9, 9, 1)
    out, _ = M.clone_stroke(dict(size=1, hardness=1.0, anti_aliased=False, offset=(0, 0)), src, pv, None, [(4.0, 0.0)])
    assert tuple(out[0, 4]) == (9, 9, 9, 1)                       # 0 < 1 / 255: kept


def test_heal_ring_off_the_canvas_skips_the_pixel():
    """a 1 x 1 canvas with sample_radius 1: both radii round every sample of pixel (0, 0) to a neighbour (cos and sin are never both below 0.5 / 0.75 in
    magnitude... at 0.75 the sample is (round(0.75 c), round(0.75 s)), (0, 0) only if |c|, |s| < 2 / 3, which no angle satisfies), so count < 1"""
    src = np.full((1, 1, 4), 200, np.uint8)
    pv = np.zeros_like(src)
    stats = M.new_stats()
    out, dirty = M.heal_stroke(dict(size=3, hardness=1.0, sample_radius=1.0), M.Ring(src, 1.0), pv, None, [(0.0, 0.0)], stats)
    assert not out.any() and stats["empty_ring"] == 1 and stats["wrote"] == 0 and dirty == (0, 0, 1, 1)


def test_heal_flat_layer_gives_its_colour_and_ties_replace():
    """a layer of one colour: any non-empty ring averages to that colour; hardness 1 gives geom 1 -> alpha byte 255, which ties a preview alpha of 255"""
    src = np.zeros((7, 7, 4), np.uint8)
    src[...] = (50, 100, 150, 7)
    pv = np.zeros_like(src)
    pv[3, 3] = (1, 2, 3, 255)
    out, _ = M.heal_stroke(dict(size=1, hardness=1.0, sample_radius=2.0), M.Ring(src, 2.0), pv, None, [(3.0, 3.0)])
    assert tuple(out[3, 3]) == (50, 100, 150, 255)
    assert int((out != pv).any(axis=-1).sum()) == 1


def test_pencil_ties_replace_and_the_box_follows_the_reference():
    pv = np.zeros((3, 5, 4), np.uint8)
    pv[1, 1], pv[1, 2] = (9, 9, 9, 128), (9, 9, 9, 129)
    color = (1.0, 0.5, 0.25, 128.0 / 255.0)
    sel = np.full((3, 5), 255, np.uint8)
    sel[1, 3] = 0
    out, dirty = M.pencil_cells(color, pv, sel, [(1, 1), (2, 1), (3, 1), (9, 9), (1, 1)])
    assert tuple(out[1, 1]) == (255, 127, 63, 128) and tuple(out[1, 2]) == (9, 9, 9, 129) and not out[1, 3].any()
    assert dirty == (0, 0, 4, 3)                                   # cells 1 and 2; the masked cell 3 returns Rect::NOTHING
    assert M.cells_box([(1, 1), (2, 1), (3, 1), (9, 9)], 5, 3) == (0, 0, 5, 3)


def test_dirty_of_a_dab_left_of_the_canvas_still_names_column_zero():
    src = one_pixel_canvas()
    out, dirty = M.clone_stroke(dict(size=3, hardness=1.0, anti_aliased=False, offset=(0, 0)), src, np.zeros_like(src), None, [(-5.0, 0.0)])
    assert M.dab_box(-5.0, 0.0, 1.5, 9, 1) == (0, 0, 0, 0) and not out.any() and dirty == (0, 0, 2, 1)
    assert M.clone_stroke(dict(size=3, hardness=1.0, anti_aliased=False, offset=(0, 0)), src, np.zeros_like(src), None, [])[1] == (0, 0, 0, 0)


# ---- the library's host functions -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from paintfe_amd import _lib
    return _lib.load()


CTX_ENTRY_POINTS = ["pfx_clone_stamp_dev", "pfx_heal_ring_dev", "pfx_pencil_dev", "pfx_clone_stamp", "pfx_heal_ring", "pfx_pencil", "pfx_stroke_commit_dev"]
HOST_ENTRY_POINTS = ["pfx_stroke_line_points", "pfx_pencil_line_cells"]


def test_the_abi_declares_and_exports_every_entry_point(lib):
    header = open(os.path.join(ROOT, "include", "pfx.h")).read()
    null, zero = C.c_void_p(None), C.c_uint32(0)
    for name in CTX_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*pfx_ctx\s*\*\s*ctx\b" % name, header), name
        getattr(lib, name).restype = C.c_int
    for name in HOST_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(lib, name), name
    assert lib.pfx_abi_version() == 1
    for name in ("pfx_clone_stamp_dev", "pfx_heal_ring_dev", "pfx_clone_stamp", "pfx_heal_ring"):       # a NULL context is an error, not a fault
        assert getattr(lib, name)(null, None, null, null, null, zero, zero, null, zero, null) != OK
    assert lib.pfx_pencil_dev(null, None, null, null, zero, zero, null, zero, null) != OK and lib.pfx_pencil(null, None, null, null, zero, zero, null, zero, null) != OK
    assert lib.pfx_stroke_commit_dev(null, null, null, null, zero, zero, 0, 0) != OK


def test_the_binding_lays_the_structs_out_as_the_header_does():
    from paintfe_amd import _lib
    assert C.sizeof(_lib.CloneStampTool) == 20 and _lib.CloneStampTool.anti_aliased.offset == 8 and _lib.CloneStampTool.offset_y.offset == 16
    assert C.sizeof(_lib.HealRingTool) == 12 and _lib.HealRingTool.sample_radius.offset == 8


LINES = {
    "diagonal": ((1.5, 2.25), (40.75, 30.5)), "below-a-tenth": ((5.0, 5.0), (5.05, 5.05)), "just-a-tenth": ((5.0, 5.0), (5.1, 5.0)),
    "leaves-midway": ((20.5, 10.5), (80.0, -30.0)), "enters": ((-10.0, -10.0), (10.0, 10.0)), "outside": ((-9.0, 3.0), (-2.0, 50.0)),
    "start-outside-and-short": ((-3.0, 5.0), (-3.01, 5.0)), "reversed": ((40.75, 30.5), (1.5, 2.25)), "steep": ((3.2, 0.1), (5.9, 39.7)),
    "shallow": ((0.4, 7.7), (49.6, 9.2)), "one-cell": ((7.3, 7.3), (7.6, 7.9)), "along-the-edge": ((49.999, 0.0), (49.999, 39.999)),
    "steep-reversed": ((5.9, 39.7), (3.2, 0.1)), "far": ((-300.5, 20.0), (400.0, 21.0)),
}


@pytest.mark.parametrize("name", sorted(LINES))
def test_line_helpers_equal_the_model(lib, name):
    from paintfe_amd import pencil_line_cells, stroke_line_points
    a, b = LINES[name]
    w, h = 50, 40
    want = M.line_points(a, b, w, h)
    got = stroke_line_points(a, b, w, h)
    assert got.dtype == np.float32 and np.array_equal(got, want), name
    cells = M.line_cells(a, b, w, h)
    assert np.array_equal(pencil_line_cells(a, b, w, h), cells)
    if name == "below-a-tenth" or name == "start-outside-and-short":
        assert len(want) == 1 and tuple(want[0]) == (F(a[0]), F(a[1]))              # the start alone, tested against nothing
    if name == "leaves-midway":
        assert 0 < len(want) < math.ceil(math.hypot(b[0] - a[0], b[1] - a[1])) + 1 and 0 < len(cells)
    if name == "outside":
        assert len(want) == 0 and len(cells) == 0


def test_line_helpers_report_the_count_and_refuse_bad_input(lib):
    n = C.c_uint32(77)
    f = lambda v: C.c_float(v)
    buf = np.full((3, 2), -1.0, np.float32)
    want = M.line_points((1.5, 2.25), (9.0, 2.25), 50, 40)
    st = lib.pfx_stroke_line_points(f(1.5), f(2.25), f(9.0), f(2.25), 50, 40, buf.ctypes.data_as(C.c_void_p), 3, C.byref(n))
    assert st == OK and n.value == len(want) > 3 and np.array_equal(buf, want[:3])          # cut at the capacity, the count in full
    cells = np.full((2, 2), -1, np.int32)
    st = lib.pfx_pencil_line_cells(f(1.5), f(2.25), f(9.0), f(2.25), 50, 40, cells.ctypes.data_as(C.c_void_p), 2, C.byref(n))
    assert st == OK and n.value == 9 and np.array_equal(cells, [[1, 2], [2, 2]])
    for fn in (lib.pfx_stroke_line_points, lib.pfx_pencil_line_cells):
        assert fn(f(1), f(1), f(2), f(2), 50, 40, None, 0, None) == ERR_INVALID
        assert fn(f(1), f(1), f(2), f(2), 50, 40, None, 4, C.byref(n)) == ERR_INVALID
        assert fn(f(1), f(1), f(2), f(2), 0, 40, None, 0, C.byref(n)) == ERR_INVALID
        for k in range(4):
            for bad in (float("nan"), float("inf"), -float("inf")):
                v = [1.0, 1.0, 2.0, 2.0]
                v[k] = bad
                assert fn(*[f(t) for t in v], 50, 40, None, 0, C.byref(n)) == ERR_INVALID
        assert fn(f(-3e38), f(0), f(3e38), f(0), 50, 40, None, 0, C.byref(n)) == ERR_INVALID   # an overflowing distance / a walk without end


# ---- the cases reach what they are built for ---------------------------------------------------------------------------------------------------------------------------
def covered(stats):
    return 0 if stats["covered"] is None else int(stats["covered"].sum())


@pytest.mark.parametrize("name", DC.CLONE_NAMES)
def test_clone_cases_reach_their_branches(name):
    c = DC.CLONE[name]
    out, dirty, s = DC.clone_expected(name)
    big, off_canvas = (c["w"], c["h"]) == DC.BIG, abs(c["tool"]["offset"][0]) == 200
    assert s["far"] > 0 or c["tool"]["size"] == 1 or c["w"] * c["h"] == 1
    assert (s["sel"] > 0) == c["sel"]
    if off_canvas:
        assert s["off_canvas"] > 0 and s["wrote"] == 0 and np.array_equal(out, DC.clone_preview(name))
    elif big:
        assert s["wrote"] > 0 and s["alpha0"] > 0 and not np.array_equal(out, DC.clone_preview(name))
        if c["tool"]["offset"][0] == 17.5:
            assert s["off_canvas"] > 0                     # part of the stroke clones from beyond the right edge / above the top
        if c["seeded"]:
            assert s["tie"] > 0 and s["kept"] > 0
        if c["tool"]["size"] >= 7 and c["tool"]["hardness"] < 1.0 and c["tool"]["anti_aliased"]:
            assert s["kept"] > 0                           # a later, fainter dab loses against an earlier one
    if big:
        assert dirty[0] == 0 and dirty[2] == c["w"] and dirty[3] == c["h"]   # the stroke starts left of the canvas, leaves it on the right and below


@pytest.mark.parametrize("name", DC.HEAL_NAMES)
def test_heal_cases_reach_their_branches_and_the_flavours_agree(name):
    c = DC.HEAL[name]
    out, dirty, s, fragile, count = DC.heal_expected(name, "device")
    out_g, dirty_g, s_g, fragile_g, count_g = DC.heal_expected(name, "glibc")
    assert dirty == dirty_g
    assert (s["sel"] > 0) == c["sel"] or c["w"] * c["h"] == 1
    if c["w"] * c["h"] == 1:
        assert s["empty_ring"] > 0 or c["sel"]              # the ring of a one-pixel canvas never lands on it
    else:
        assert s["wrote"] > 0 and not np.array_equal(out, DC.heal_preview(name))
        if c["seeded"] and c["tool"]["size"] >= 7:
            assert s["tie"] > 0
            assert s["kept"] > 0 or c["tool"]["hardness"] == 1.0
    # where no sample can move, the two flavours pick the same samples and write the same bytes; alpha never depends on the flavour where a ring is not empty
    same = ~(fragile | fragile_g)
    assert np.array_equal(out[same], out_g[same])
    differing = int((out != out_g).any(axis=-1).sum())
    sure = same | (np.minimum(count, count_g) >= 2)
    assert np.array_equal(out[sure][:, 3], out_g[sure][:, 3])
    n_cov, n_frag = covered(s), int((fragile & s["covered"]).sum()) if s["covered"] is not None else 0
    print(f"{name}: zone {c['zone']}, covered {n_cov}, fragile among them {n_frag}, pixels where glibc and device differ {differing}")
    if c["zone"] == "free":
        assert n_frag * 100 <= n_cov, (n_frag, n_cov)       # the cap: a condition on the inputs, see tests/dabtools_cases.py


@pytest.mark.parametrize("name", DC.PENCIL_NAMES)
def test_pencil_cases_reach_their_branches(name):
    c = DC.PENCIL[name]
    out, dirty, s = DC.pencil_expected(name)
    w, h = c["w"], c["h"]
    assert s["wrote"] > 0 or (c["sel"] and w * h == 1)
    assert (s["sel"] > 0) == c["sel"] or w * h <= 130
    if w * h > 1 and not c["sel"]:
        assert s["kept"] > 0 or c["color"][3] == 1.0
        assert s["tie"] > 0 or c["color"][3] == 0.5                    # `tie` meets its own byte; a cell listed twice ties with what it wrote
        assert dirty == M.cells_box(np.concatenate(DC.pencil_cell_lists(w, h)), w, h)
