"""The line / curve tool's CPU model (tests/linetool_model.py) held to what it restates, without a GPU:

* against an independent scalar transcription of rasterize_bezier, draw_bezier_circle_with_hardness, compute_line_alpha and draw_filled_triangle (ref:
  src/ui/panels/tools/behavior/raster/bezier_math.rs, brush_render.rs:85-133) — primitive after primitive, pixel by pixel, the alpha byte carried;
* the fact the kernel rests on — (pa * 255.0) as u8 >= s for the f32 values just above s / 255.0, all 256 bytes — and that the maximum form equals the serial
  form on every case of tests/linetool_cases.py;
* pfx_line_bounds and pfx_line_plan of the library against the model, bit for bit, through ctypes;
* the cases reach the branches they are named for; the header declares what the library exports."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from . import linetool_cases as LC
from . import linetool_model as M

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID = 0, -1


# ---- the scalar transcription -----------------------------------------------------------------------------------------------------------------------------------------
def rs_u32(v):
    v = float(v)
    return 0 if (v != v or v <= 0.0) else (0xFFFFFFFF if v >= 4294967296.0 else int(v))


def rs_u8(v):
    v = float(v)
    return 0 if v != v else int(max(0.0, min(255.0, math.trunc(v))))


def rs_fmax(a, b):      # f32::max: a NaN operand yields the other
    return b if a != a else (a if b != b else (a if a > b else b))


def rs_fmin(a, b):
    return b if a != a else (a if b != b else (a if a < b else b))


def rs_clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def rs_rem(a, b):       # `%` on f32: fmodf, exact; NaN for an infinite a or a zero b
    try:
        return F(math.fmod(float(a), float(b)))
    except ValueError:
        return F(np.nan)


def scalar_line_alpha(dist, radius, forced_hardness, anti_alias):
    if not anti_alias:
        return F(1) if dist < radius else F(0)
    safe = rs_clamp(F(forced_hardness), F(0), F(0.99))
    if radius < F(1.5):
        eff, fade = radius + F(1), F(1)
    elif radius < F(3):
        aa_extend = F(1.5)
        eff, fade = radius + aa_extend, aa_extend + (radius * (F(1) - safe))
    else:
        eff, fade = radius, rs_fmax(radius * (F(1) - safe), F(2))
    solid = eff - fade
    if dist <= solid:
        return F(1)
    if dist >= eff:
        return F(0)
    t = (dist - solid) / fade
    x = F(1) - rs_clamp(t, F(0), F(1))
    return x * x * (F(3) - F(2) * x)


def scalar_circle(pv, sel, cx, cy, color, radius, anti_alias):
    h, w = pv.shape[:2]
    pad = (F(1.5) if radius < F(1.5) else rs_fmax(radius * (F(1) - F(0.95)), F(2)) + F(2)) if anti_alias else F(1)
    outer = radius + pad
    min_x, max_x = rs_u32(rs_fmax(cx - outer, F(0))), min(rs_u32(np.ceil(cx + outer)), w - 1)
    min_y, max_y = rs_u32(rs_fmax(cy - outer, F(0))), min(rs_u32(np.ceil(cy + outer)), h - 1)
    for y in range(min_y, max_y + 1):
        for x in range(min_x, max_x + 1):
            if sel is not None and sel[y, x] == 0:
                continue
            dx, dy = F(x) - cx, F(y) - cy
            dist = np.sqrt(dx * dx + dy * dy)
            alpha = scalar_line_alpha(dist, radius, 0.95, anti_alias)
            if alpha <= 0:
                continue
            pixel_alpha = alpha * color[3]
            if pixel_alpha > F(pv[y, x, 3]) / F(255):
                pv[y, x] = [rs_u8(color[0] * F(255)), rs_u8(color[1] * F(255)), rs_u8(color[2] * F(255)), rs_u8(pixel_alpha * F(255))]


def scalar_triangle(pv, sel, a, b, c, color):
    h, w = pv.shape[:2]
    fade = F(1)
    min_x = rs_u32(rs_fmax(np.floor(rs_fmin(rs_fmin(a[0], b[0]), c[0]) - fade), F(0)))
    max_x = min(rs_u32(np.ceil(rs_fmax(rs_fmax(a[0], b[0]), c[0]) + fade)), max(w - 1, 0))
    min_y = rs_u32(rs_fmax(np.floor(rs_fmin(rs_fmin(a[1], b[1]), c[1]) - fade), F(0)))
    max_y = min(rs_u32(np.ceil(rs_fmax(rs_fmax(a[1], b[1]), c[1]) + fade)), max(h - 1, 0))

    def edge_dist(v0, v1, px, py):
        ex, ey = v1[0] - v0[0], v1[1] - v0[1]
        ln = rs_fmax(np.sqrt(ex * ex + ey * ey), F(0.001))
        return (ex * (py - v0[1]) - ey * (px - v0[0])) / ln

    ex, ey = b[0] - a[0], b[1] - a[1]
    cross = ex * (c[1] - a[1]) - ey * (c[0] - a[0])
    sign = F(1) if cross >= 0 else F(-1)
    for y in range(min_y, max_y + 1):
        for x in range(min_x, max_x + 1):
            if sel is not None and sel[y, x] == 0:
                continue
            px, py = F(x) + F(0.5), F(y) + F(0.5)
            d0, d1, d2 = edge_dist(a, b, px, py) * sign, edge_dist(b, c, px, py) * sign, edge_dist(c, a, px, py) * sign
            min_dist = rs_fmin(rs_fmin(d0, d1), d2)
            if min_dist < -fade:
                continue
            if min_dist >= fade:
                alpha = color[3]
            else:
                t = rs_clamp((min_dist + fade) / (F(2) * fade), F(0), F(1))
                alpha = t * t * (F(3) - F(2) * t) * color[3]
            if alpha <= 0:
                continue
            if alpha > F(pv[y, x, 3]) / F(255):
                pv[y, x] = [rs_u8(color[0] * F(255)), rs_u8(color[1] * F(255)), rs_u8(color[2] * F(255)), rs_u8(alpha * F(255))]


def scalar_rasterize(tool, preview, sel, last_bounds):
    pv = preview.copy()
    h, w = pv.shape[:2]
    size = F(tool["size"])
    color = [F(c) / F(255) for c in tool["color"]]
    if last_bounds is None:
        pv[:] = 0
    else:
        b = [F(v) for v in last_bounds]
        min_x, max_x = rs_u32(rs_fmax(np.floor(b[0]), F(0))), rs_u32(rs_fmin(np.ceil(b[2]), F(w)))
        min_y, max_y = rs_u32(rs_fmax(np.floor(b[1]), F(0))), rs_u32(rs_fmin(np.ceil(b[3]), F(h)))
        for cy in range(min_y // 64, min(-(-max_y // 64), -(-h // 64))):
            for cx in range(min_x // 64, min(-(-max_x // 64), -(-w // 64))):
                pv[cy * 64:cy * 64 + 64, cx * 64:cx * 64 + 64] = 0
    p = [(F(x), F(y)) for x, y in tool["p"]]
    length = lambda u, v: M.vec2_length(u[0] - v[0], u[1] - v[1])
    spacing = rs_fmax(size * F(0.1), F(0.5))
    total = (length(p[1], p[0]) + length(p[2], p[1]) + length(p[3], p[2])) + length(p[3], p[0])
    raw = float(np.ceil(total / spacing))
    steps = min(max(0 if raw != raw else int(min(raw, 1e18)), 20), 5000)
    on, off = {0: (F(0), F(0)), 1: (size * F(0.5), size * F(1.5)), 2: (size * F(2), size * F(1.5))}[tool["pattern"]]
    cycle = on + off
    cumulative, last_pos, line_points = F(0), None, []
    for i in range(steps + 1):
        t = F(i) / F(steps)
        t2 = t * t
        t3 = t2 * t
        mt = F(1) - t
        mt2 = mt * mt
        mt3 = mt2 * mt
        pos = (mt3 * p[0][0] + F(3) * mt2 * t * p[1][0] + F(3) * mt * t2 * p[2][0] + t3 * p[3][0],
               mt3 * p[0][1] + F(3) * mt2 * t * p[1][1] + F(3) * mt * t2 * p[2][1] + t3 * p[3][1])
        if last_pos is not None:
            cumulative = cumulative + length(pos, last_pos)
        last_pos = pos
        fx, fy = pos
        if fx >= 0 and fy >= 0 and rs_u32(fx) < w and rs_u32(fy) < h:
            should_draw = True if tool["pattern"] == 0 else bool(rs_rem(cumulative, cycle) < on)
            if should_draw:
                if sel is not None and sel[rs_u32(fy), rs_u32(fx)] == 0:
                    continue
                line_points.append((fx, fy, i == 0, i == steps))
    for fx, fy, is_start, is_end in line_points:
        if tool["cap_style"] == 1 and (is_start or is_end):
            continue
        scalar_circle(pv, sel, fx, fy, color, size / F(2), bool(tool["anti_alias"]))
    if tool["end_shape"] == 1:
        arrow_length, half = rs_fmax(size * F(3), F(8)), rs_fmax(size * F(1.5), F(4))
        tip_advance = size + size / F(2)
        if tool["arrow_side"] in (0, 2):
            tx, ty = F(3) * (p[3][0] - p[2][0]), F(3) * (p[3][1] - p[2][1])
            ln = rs_fmax(np.sqrt(tx * tx + ty * ty), F(0.001))
            dx, dy = tx / ln, ty / ln
            tip = (p[3][0] + dx * tip_advance, p[3][1] + dy * tip_advance)
            base = (tip[0] - dx * arrow_length, tip[1] - dy * arrow_length)
            px, py = -dy, dx
            scalar_triangle(pv, sel, tip, (base[0] + px * half, base[1] + py * half), (base[0] - px * half, base[1] - py * half), color)
        if tool["arrow_side"] in (1, 2):
            tx, ty = F(3) * (p[1][0] - p[0][0]), F(3) * (p[1][1] - p[0][1])
            ln = rs_fmax(np.sqrt(tx * tx + ty * ty), F(0.001))
            dx, dy = tx / ln, ty / ln
            tip = (p[0][0] - dx * tip_advance, p[0][1] - dy * tip_advance)
            base = (tip[0] + dx * arrow_length, tip[1] + dy * arrow_length)
            px, py = -dy, dx
            scalar_triangle(pv, sel, tip, (base[0] + px * half, base[1] + py * half), (base[0] - px * half, base[1] - py * half), color)
    return pv


TINY_W, TINY_H = 70, 66      # 2 x 2 chunks, the last column 6 wide and the last row 2 tall
TINY_CURVE = [(5.5, 60.2), (20.0, 70.0), (40.0, 50.0), (66.3, 62.8)]
# size, aa, pattern, cap, end_shape, arrow_side, colour, selection, preview, last_bounds
TINY = [
    (1, True, 0, 0, 0, 0, LC.RED, False, "empty", None), (1, False, 0, 1, 1, 2, LC.GREEN, True, "seeded", (0.0, 0.0, 0.0, 0.0)),
    (2.9, True, 2, 0, 1, 0, LC.GREEN, True, "seeded", (10.5, 3.0, 63.5, 20.0)), (2.9, False, 1, 1, 0, 0, LC.RED, False, "seeded", (60.0, 60.0, 80.0, 90.0)),
    (4, True, 0, 0, 1, 1, (7, 248, 77, 1), False, "seeded", (0.0, 0.0, 0.0, 0.0)), (4, False, 2, 0, 1, 2, LC.RED, True, "empty", None),
    (5.9, True, 1, 1, 1, 2, LC.GREEN, False, "seeded", (0.0, 64.0, 64.0, 66.0)), (5.9, False, 0, 0, 0, 0, LC.GREEN, True, "seeded", (0.0, 0.0, 0.0, 0.0)),
    (12, True, 0, 1, 1, 0, LC.GREEN, True, "seeded", (0.0, 0.0, 0.0, 0.0)), (12, False, 2, 0, 0, 0, LC.RED, False, "empty", None),
]


@pytest.mark.parametrize("size,aa,pattern,cap,end_shape,side,color,use_sel,preview,last", TINY, ids=[f"size{t[0]}-{'aa' if t[1] else 'hard'}" for t in TINY])
def test_model_equals_the_scalar_loop_in_both_forms(size, aa, pattern, cap, end_shape, side, color, use_sel, preview, last):
    tool = LC.tool(TINY_CURVE, size, color, pattern, cap, end_shape, side, aa)
    pv = LC.seeded_preview(TINY_W, TINY_H) if preview == "seeded" else np.zeros((TINY_H, TINY_W, 4), np.uint8)
    sel = LC.selection(TINY_W, TINY_H) if use_sel else None
    with np.errstate(all="ignore"):
        want = scalar_rasterize(tool, pv, sel, last)
    serial, _, st = M.render(tool, pv, sel, last)
    by_max, _, _ = M.render(tool, pv, sel, last, "max")
    assert st["writes"] > 0 and not np.array_equal(want, pv)
    assert np.array_equal(serial, want), int((serial != want).any(axis=-1).sum())
    assert np.array_equal(by_max, want), int((by_max != want).any(axis=-1).sum())


def test_scalar_loop_on_points_far_outside_the_canvas():
    """the saturating casts and NaN rules decide what is drawn: here the curve passes through the canvas between far control points, and an overflowing one
    draws nothing"""
    far = LC.tool([(-3000.0, 20.0), (-10.0, 900.0), (80.0, -700.0), (2500.0, 40.0)], 4, LC.RED, 0, 0, 1, 2, True)
    huge = LC.tool([(-3e38, 20.0), (3e38, 3e38), (-3e38, -3e38), (3e38, 40.0)], 4, LC.RED, 1, 0, 1, 2, True)
    pv = np.zeros((TINY_H, TINY_W, 4), np.uint8)
    for tool, draws in ((far, True), (huge, False)):
        with np.errstate(all="ignore"):
            want = scalar_rasterize(tool, pv, None, None)
        got, _, st = M.render(tool, pv, None, None)
        assert np.array_equal(got, want) and np.array_equal(M.render(tool, pv, None, None, "max")[0], want)
        assert bool(want.any()) == draws and st["off_canvas"] > 0


# ---- what the kernel rests on ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_write_never_lowers_the_alpha_byte():
    """for every byte s and the first four f32 values pa above s / 255.0: (pa * 255.0) as u8 >= s — so the byte a pixel carries never goes down, and the serial
    walk equals the maximum"""
    for s in range(256):
        pa = F(s) / F(255)
        for _ in range(4):
            pa = np.nextafter(pa, F(np.inf), dtype=F)
            assert pa > F(s) / F(255) and int(M.trunc_u8(pa * F(255))) >= s, (s, pa)
        assert int(M.trunc_u8((F(s) / F(255)) * F(255))) == s     # and the round trip of a colour byte gives the byte back, for every byte
    assert LC.LOSSY_BYTES == []                                   # the model finds no byte c with ((c / 255.0) * 255.0) as u8 != c: the colour cases use 7


@pytest.mark.parametrize("name", LC.NAMES)
def test_maximum_form_equals_the_serial_form(name):
    serial, b, st = LC.expected(name)
    by_max, b2, _ = LC.expected(name, None, "max")
    assert np.array_equal(serial, by_max) and np.array_equal(b, b2)
    other = not LC.CASES[name]["sel"]                              # the GPU test runs every case with and without the selection
    assert np.array_equal(LC.expected(name, other)[0], LC.expected(name, other, "max")[0])


# ---- the library's host functions -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from paintfe_amd import _lib
    return _lib.load()


def c_tool(t):
    from paintfe_amd import line_tool
    return line_tool(t["p"], t["size"], t["color"], t["pattern"], t["cap_style"], t["end_shape"], t["arrow_side"], t["anti_alias"])


CTX_ENTRY_POINTS = ["pfx_line_render_dev", "pfx_line_render", "pfx_stroke_commit_mask_dev", "pfx_stroke_commit_mask"]
HOST_ENTRY_POINTS = ["pfx_line_bounds", "pfx_line_plan"]


def test_the_abi_declares_and_exports_every_entry_point(lib):
    header = open(os.path.join(ROOT, "include", "pfx.h")).read()
    null, zero = C.c_void_p(None), C.c_uint32(0)
    for name in CTX_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*pfx_ctx\s*\*\s*ctx\b" % name, header), name
        getattr(lib, name).restype = C.c_int
    for name in HOST_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+pfx_line_tool\s*\*" % name, header) and hasattr(lib, name), name
    assert lib.pfx_abi_version() == 1
    for name in ("pfx_line_render_dev", "pfx_line_render"):          # a NULL context is an error, not a fault
        assert getattr(lib, name)(null, None, null, null, zero, zero, None, None) != OK
    assert lib.pfx_stroke_commit_mask_dev(null, null, null, null, zero, zero, 0) != OK and lib.pfx_stroke_commit_mask(null, null, null, null, zero, zero, 0) != OK
    assert lib.pfx_line_bounds(None, zero, zero, None) == ERR_INVALID and lib.pfx_line_plan(None, zero, zero, null, zero, None, None, None) == ERR_INVALID


def test_the_binding_lays_the_struct_out_as_the_header_does():
    from paintfe_amd import _lib
    T = _lib.LineTool
    assert C.sizeof(T) == 60 and T.size.offset == 32 and T.color.offset == 36 and T.pattern.offset == 40 and T.anti_alias.offset == 56


HOSTILE = {
    "far": LC.tool([(-3000.0, 20.0), (-10.0, 900.0), (80.0, -700.0), (2500.0, 40.0)], 4, end_shape=1, arrow_side=2),
    "overflowing": LC.tool([(-3e38, 20.0), (3e38, 3e38), (-3e38, -3e38), (3e38, 40.0)], 4, pattern=1, end_shape=1, arrow_side=2),
    "size0-dashed": LC.tool(LC.SWEEP, 0.0, pattern=2, end_shape=1, arrow_side=2),
    "negative-size": LC.tool(LC.SWEEP, -5.0, end_shape=1, arrow_side=1),
    "huge-size": LC.tool(LC.SWEEP, 1e30, pattern=1, end_shape=1, arrow_side=2),
}


def same_floats(a, b):
    """the same bit patterns, except that any NaN equals any NaN (an overflowing head: the sign and payload of a NaN are nobody's contract)"""
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def plans_agree(lib, tool, w, h):
    from paintfe_amd import line_bounds, line_plan
    want_dots, want_tris, info = M.plan(tool, w, h)
    dots, tris = line_plan(c_tool(tool), w, h)
    assert dots.shape == want_dots.shape and np.array_equal(dots.view(np.uint32), want_dots.view(np.uint32))          # bit patterns
    assert same_floats(tris, want_tris) and same_floats(line_bounds(c_tool(tool), w, h), M.bounds(tool, w, h))
    return info


@pytest.mark.parametrize("name", LC.NAMES)
def test_bounds_and_plan_equal_the_model(lib, name):
    c = LC.CASES[name]
    plans_agree(lib, c["tool"], c["w"], c["h"])


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_bounds_and_plan_equal_the_model_on_hostile_floats(lib, name):
    info = plans_agree(lib, HOSTILE[name], LC.W, LC.H)
    if name == "overflowing":
        assert info["steps"] == 5000 and info["off_canvas"] >= 4990
    if name == "size0-dashed":
        assert info["pattern_off"] > 0 and len(M.plan(HOSTILE[name], LC.W, LC.H)[0]) == 0        # a cycle of 0: fmodf gives NaN, which compares false


def test_plan_reports_the_count_and_refuses_bad_input(lib):
    c = LC.CASES["arrow-both-size4"]
    t, w, h = c_tool(c["tool"]), c["w"], c["h"]
    want, want_tris, _ = M.plan(c["tool"], w, h)
    n, nt = C.c_uint32(0), C.c_uint32(9)
    small = np.full((10, 2), -7.0, F)
    tri = (C.c_float * 12)()
    assert lib.pfx_line_plan(C.byref(t), w, h, small.ctypes.data_as(C.c_void_p), 4, C.byref(n), tri, C.byref(nt)) == OK
    assert n.value == len(want) and nt.value == 2 and np.array_equal(small[:4], want[:4]) and (small[4:] == -7.0).all()
    assert lib.pfx_line_plan(C.byref(t), w, h, None, 0, C.byref(n), None, None) == OK and n.value == len(want)
    assert lib.pfx_line_plan(C.byref(t), w, h, None, 4, C.byref(n), None, None) == ERR_INVALID
    assert lib.pfx_line_plan(C.byref(t), w, h, None, 0, None, None, None) == ERR_INVALID
    assert lib.pfx_line_plan(C.byref(t), 0, h, None, 0, C.byref(n), None, None) == ERR_INVALID
    assert lib.pfx_line_plan(C.byref(t), 20000, 20000, None, 0, C.byref(n), None, None) == ERR_INVALID
    out = (C.c_float * 4)()
    assert lib.pfx_line_bounds(C.byref(t), w, 0, out) == ERR_INVALID and lib.pfx_line_bounds(C.byref(t), w, h, None) == ERR_INVALID
    for field, bad in [("size", float("nan")), ("size", float("inf")), ("pattern", 3), ("pattern", -1), ("cap_style", 2), ("end_shape", 2), ("arrow_side", 3)]:
        broken = c_tool(c["tool"])
        setattr(broken, field, bad)
        assert lib.pfx_line_plan(C.byref(broken), w, h, None, 0, C.byref(n), None, None) == ERR_INVALID, field
        assert lib.pfx_line_bounds(C.byref(broken), w, h, out) == ERR_INVALID, field
    for k in range(8):
        for bad in (float("nan"), float("inf"), float("-inf")):
            broken = c_tool(c["tool"])
            broken.p[k] = bad
            assert lib.pfx_line_plan(C.byref(broken), w, h, None, 0, C.byref(n), None, None) == ERR_INVALID
            assert lib.pfx_line_bounds(C.byref(broken), w, h, out) == ERR_INVALID


# ---- the cases reach their branches ---------------------------------------------------------------------------------------------------------------------------------------
def chunk_entries(name):
    c = LC.CASES[name]
    dots, _, _ = M.plan(c["tool"], c["w"], c["h"])
    radius = F(c["tool"]["size"]) / F(2)
    total = 0
    for fx, fy in dots:
        x0, x1, y0, y1 = M.dot_box(fx, fy, radius, bool(c["tool"]["anti_alias"]), c["w"], c["h"])
        total += (x1 // 64 - x0 // 64 + 1) * (y1 // 64 - y0 // 64 + 1)
    return total, len(dots)


def test_the_piece_case_needs_at_least_three_pieces():
    entries, n = chunk_entries(LC.PIECE_CASE)
    assert n == 5001 and entries >= 3 * LC.PIECE_LIMIT          # a piece holds at most PIECE_LIMIT entries


@pytest.mark.parametrize("name", LC.NAMES)
def test_cases_reach_their_branches(name):
    c = LC.CASES[name]
    tool, w, h = c["tool"], c["w"], c["h"]
    out, _, st = LC.expected(name)
    dots, tris, _ = M.plan(tool, w, h)
    radius = F(tool["size"]) / F(2)
    assert st["writes"] > 0
    if name.startswith("cross"):
        regime = 0 if radius < F(1.5) else (1 if radius < F(3) else 2)
        assert regime == {1: 0, 2.9: 0, 4: 1, 5.9: 1, 12: 2}[tool["size"]]
        assert st["px_solid"] > 0 and (st["px_fade"] > 0) == bool(tool["anti_alias"])
        cells = {(M.as_u32(x), M.as_u32(y)) for x, y in dots}
        assert {63, 64} <= {y for _, y in cells} and {127, 128} <= {x for x, _ in cells}
        assert {(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (2, 2)} <= st["dot_chunks"]
    if name.startswith("sweep"):
        assert {cx for cx, _ in st["dot_chunks"]} == {0, 1, 2, 3} and {cy for _, cy in st["dot_chunks"]} == {0, 1, 2}
    if name.startswith("outside"):
        assert st["off_canvas"] > 0 and st["clipped_low"] > 0 and st["clipped_high"] > 0 and st["steps"] < 5000
    if name.startswith("degenerate"):
        assert st["raw_steps"] == 0 and st["steps"] == 20 and st["n_listed"] == 21 and st["length"] < 0.01
    if name.startswith("cap5000"):
        assert st["raw_steps"] > 5000 and st["steps"] == 5000 and st["n_listed"] == 5001
    if name.startswith(("dotted", "dashed")):
        cycle = float(tool["size"]) * (2.0 if tool["pattern"] == 1 else 3.5)
        assert st["pattern_off"] > 0 and st["n_listed"] > 0 and float(st["length"]) / cycle >= 3
        assert (st["flat_dropped"] >= 1) == (tool["cap_style"] == 1)
    if name == "solid-size4-flat":
        assert st["flat_dropped"] == 2
    if name.startswith("arrow"):
        signs = [float(M.tri_sign(t)) for t in tris]
        assert signs == {0: [1.0], 1: [-1.0], 2: [1.0, -1.0]}[tool["arrow_side"]] or name == "arrow-zero-tangent-size4"
    if name in ("arrow-end-size4", "arrow-start-size4", "arrow-both-size4", "arrow-both-size1-hard"):
        assert st["tri_full"] > 0 and st["tri_fade"] > 0 and st["tri_skipped"] > 0
    if name == "arrow-partly-off-size12":
        assert tris[0][:, 0].max() > w and tris[0][:, 1].max() > h and st["tri_full"] > 0       # hangs over the right and the bottom edge
    if name == "arrow-wholly-off-size4":
        assert tris[0][:, 0].max() < -1 and st["tri_full"] == st["tri_fade"] == 0 and st["tri_skipped"] > 0    # the saturated box is column 0; every pixel is skipped
    if name == "arrow-zero-tangent-size4":
        assert (tris[0] == tris[0][0]).all() and float(M.tri_sign(tris[0])) == 1.0              # direction 0 / 0.001: the head collapses onto p0, the cross product is 0
    if name == "arrow-beyond-the-dots-size12":
        assert st["tri_chunks"] - st["dot_chunks"]
    if name.startswith("sel") or c["sel"]:
        sel = LC.selection(w, h)
        assert st["sel_dropped"] > 0 and st["px_sel_skipped"] > 0
        if c["preview"] == "empty":
            assert not out[sel == 0].any() and out[sel != 0].any()
    if name == "sel-arrow-size12":
        x0, x1, y0, y1 = M.tri_box(tris[0], w, h)
        box_sel, box_out = LC.selection(w, h)[y0:y1 + 1, x0:x1 + 1], out[y0:y1 + 1, x0:x1 + 1, 3]
        assert (box_sel == 0).any() and (box_out[box_sel == 0] == 0).all() and (box_out[box_sel != 0] == 255).any()
    if name.startswith("colour"):
        a = tool["color"][3]
        assert out[..., 3].max() == a and {tuple(px) for px in out[out[..., 3] > 0][:, :3]} == {(7, 248, 77)}
    if name.startswith("seeded-strict"):
        pv = LC.seeded_preview(w, h)
        changed = (out != pv).any(axis=-1)
        assert st["ties"] > 0 and changed.any() and pv[changed][:, 3].max() <= 127 and (out[changed][:, :3] == LC.GREEN[:3]).all()
        best = LC.expected(name, None, "max")[0]
        assert np.array_equal(best, out)
        # where the line is at full strength over the band of equal alpha, nothing was written
        plain = M.render(tool, np.zeros_like(pv), LC.selection_of(c), None)[0]
        full = plain[..., 3] == 128
        assert (full & (pv[..., 3] == 128)).any() and not changed[full & (pv[..., 3] >= 128)].any() and changed[full & (pv[..., 3] == 127)].all()
    if name.startswith("seeded-clear"):
        pv = LC.seeded_preview(w, h)
        cleared = np.zeros((h, w), bool)
        if c["last"] == "all":
            cleared[:] = True
        else:
            cx0, cx1, cy0, cy1 = M.clear_chunks(c["last"], w, h)
            assert (cx0, cx1, cy0, cy1) == {"seeded-clear-part-size4": (1, 3, 0, 1), "seeded-clear-edge-size4": (2, 4, 1, 3), "seeded-clear-away-from-the-line": (2, 4, 1, 3)}[name]
            cleared[cy0 * 64:cy1 * 64, cx0 * 64:cx1 * 64] = True
        line = (out[..., :3] == LC.GREEN[:3]).all(axis=-1)            # a faint rim pixel is written with alpha byte 0
        assert not out[cleared & ~line].any()                                    # exactly the reference's chunks are empty but for the line
        assert np.array_equal(out[~cleared & ~line], pv[~cleared & ~line])        # the stale rest survives
        assert (cleared & line).any() or name == "seeded-clear-away-from-the-line"
        if name == "seeded-clear-away-from-the-line":
            chunks = {(cx, cy) for cx in range(2, 4) for cy in range(1, 3)}
            assert not chunks & (st["dot_chunks"] | st["tri_chunks"])             # chunks of the launch that are only cleared
        if name == "seeded-clear-part-size4":
            assert (~cleared & line).any() and pv[70, 80, 3] and np.array_equal(out[70, 80], pv[70, 80])


def test_two_frame_drag_clears_by_chunks():
    pv0 = np.zeros((LC.H, LC.W, 4), np.uint8)
    f1, b1, _ = M.render(LC.DRAG[0], pv0, None, None)
    f2, _, _ = M.render(LC.DRAG[1], f1, None, b1)
    fresh, _, _ = M.render(LC.DRAG[1], pv0, None, None)
    cx0, cx1, cy0, cy1 = M.clear_chunks(b1, LC.W, LC.H)
    assert (cx0, cx1, cy0, cy1) == (0, 3, 0, 2)
    assert np.array_equal(f2, fresh)                    # frame 1 lay inside its own bounds' chunks: nothing stale is left
    with np.errstate(all="ignore"):
        assert np.array_equal(scalar_rasterize(LC.DRAG[1], scalar_rasterize(LC.DRAG[0], pv0, None, None), None, b1), f2)


def test_commit_mask_model_over_all_pairs():
    old, pv = LC.commit_inputs()
    for reveal in (False, True):
        got = M.commit_mask(old, pv, None, reveal)
        for o, s in [(0, 0), (255, 255), (255, 1), (1, 255), (200, 100), (100, 200), (3, 254), (254, 3)]:
            want = (o * (255 - s)) // 255 if reveal else o + ((255 - o) * s) // 255
            assert got[o, s] == (want if s else o)
        assert (got <= old).all() if reveal else (got >= old).all()
    sel = LC.selection(256, 256)
    got = M.commit_mask(old, pv, sel, False)
    assert np.array_equal(got[sel == 0], old[sel == 0]) and not np.array_equal(got, old)
