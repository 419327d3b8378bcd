"""The case table of the line / curve tool, shared by tests/test_linetool_model_host.py (which asserts that every case reaches the branch it is named for)
and tests/test_gpu_linetool.py.  Canvases are 200 x 136 unless stated: 4 x 3 chunks, the last column and the last row of chunks 8 pixels wide and tall."""
import functools

import numpy as np

from . import linetool_model as M

F = np.float32
W, H = 200, 136
WIDE = (1344, 70)   # 21 x 2 chunks: the 5000-step cap at size 1

# curves
CROSS = [(2.0, 63.4), (120.0, 63.6), (140.0, 64.0), (126.5, 134.0)]        # along row 63 / 64, then down column 127 / 128: every interior chunk border but x = 192
SWEEP = [(6.5, 8.25), (150.0, -20.0), (60.0, 150.0), (196.5, 120.75)]      # crosses x = 64, 128, 192 and y = 64, 128
OUTSIDE = [(-30.0, -20.0), (260.0, 10.0), (-50.0, 150.0), (230.0, 160.0)]  # control points outside on every side
POINT = [(100.3, 70.7)] * 4
LONG = [(2.0, 35.0), (450.0, 5.0), (900.0, 65.0), (1341.0, 35.0)]
TO_THE_RIGHT = [(20.0, 40.0), (50.0, 30.0), (80.0, 50.0), (110.0, 40.0)]   # ends at x = 110 heading right: a size-12 head reaches chunk column 2, the dots do not
NEAR_EDGE = [(120.0, 100.0), (150.0, 90.0), (170.0, 120.0), (196.0, 130.0)]   # the end head hangs over the right and bottom edges
LEAVES = [(60.0, 60.0), (30.0, 40.0), (0.0, 30.0), (-40.0, 20.0)]          # ends far left of the canvas: the end head is wholly off it
ZERO_TANGENT = [(70.0, 50.0), (70.0, 50.0), (100.0, 80.0), (140.0, 60.0)]  # p1 == p0: the start tangent's 0.001 floor

RED, GREEN = (200, 30, 40, 255), (10, 220, 90, 128)


def tool(p, size, color=RED, pattern=0, cap_style=0, end_shape=0, arrow_side=0, anti_alias=True):
    return dict(p=p, size=size, color=color, pattern=pattern, cap_style=cap_style, end_shape=end_shape, arrow_side=arrow_side, anti_alias=anti_alias)


def case(t, w=W, h=H, preview="empty", last="all", sel=False):
    """preview: "empty" or "seeded"; last: "all" (no previous bounds: clear everything), "none" (bounds that clear no chunk), or four floats"""
    return dict(tool=t, w=w, h=h, preview=preview, last=last, sel=sel)


CASES = {}
for size in (1, 2.9, 4, 5.9, 12):
    for aa in (True, False):
        CASES[f"cross-size{size}-{'aa' if aa else 'hard'}"] = case(tool(CROSS, size, anti_alias=aa))
CASES["sweep-size4"] = case(tool(SWEEP, 4))
CASES["outside-size5.9"] = case(tool(OUTSIDE, 5.9))
CASES["outside-size12-hard"] = case(tool(OUTSIDE, 12, anti_alias=False))
CASES["degenerate-size4"] = case(tool(POINT, 4))
CASES["cap5000-size1"] = case(tool(LONG, 1), *WIDE)
for pattern, pname in ((1, "dotted"), (2, "dashed")):
    for size in (2, 12):
        for cap, cname in ((0, "round"), (1, "flat")):
            CASES[f"{pname}-size{size}-{cname}"] = case(tool(SWEEP, size, pattern=pattern, cap_style=cap))
CASES["solid-size4-flat"] = case(tool(SWEEP, 4, cap_style=1))
for side, sname in ((0, "end"), (1, "start"), (2, "both")):
    CASES[f"arrow-{sname}-size4"] = case(tool(SWEEP, 4, end_shape=1, arrow_side=side))
CASES["arrow-both-size1-hard"] = case(tool(SWEEP, 1, end_shape=1, arrow_side=2, anti_alias=False))
CASES["arrow-partly-off-size12"] = case(tool(NEAR_EDGE, 12, end_shape=1, arrow_side=0))
CASES["arrow-wholly-off-size4"] = case(tool(LEAVES, 4, end_shape=1, arrow_side=0))
CASES["arrow-zero-tangent-size4"] = case(tool(ZERO_TANGENT, 4, end_shape=1, arrow_side=1))
CASES["arrow-beyond-the-dots-size12"] = case(tool(TO_THE_RIGHT, 12, end_shape=1, arrow_side=0))
CASES["sel-dots-size4"] = case(tool(SWEEP, 4), sel=True)
CASES["sel-dots-size12-dashed"] = case(tool(SWEEP, 12, pattern=2), sel=True)
CASES["sel-arrow-size12"] = case(tool(TO_THE_RIGHT, 12, end_shape=1, arrow_side=2), sel=True)
CASES["sel-cross-size1"] = case(tool(CROSS, 1), sel=True)
# ((c / 255.0) * 255.0) as u8 for every byte c: the model finds which bytes do not come back — none (tests/test_linetool_model_host.py asserts the list), so the
# colour cases take byte 7
LOSSY_BYTES = [c for c in range(256) if M.color_bytes((c, c, c))[0] != c]
LOSSY = LOSSY_BYTES[0] if LOSSY_BYTES else 7
for a in (255, 128, 1):
    CASES[f"colour-alpha{a}-size5.9"] = case(tool(SWEEP, 5.9, color=(LOSSY, 255 - LOSSY, 77, a)))
CASES["seeded-strict-size12"] = case(tool(SWEEP, 12, color=GREEN), preview="seeded", last="none")
CASES["seeded-strict-size1-arrow"] = case(tool(SWEEP, 1, color=GREEN, end_shape=1, arrow_side=2), preview="seeded", last="none", sel=True)
CASES["seeded-clear-all-size4"] = case(tool(CROSS, 4, color=GREEN), preview="seeded")
CASES["seeded-clear-part-size4"] = case(tool(CROSS, 4, color=GREEN), preview="seeded", last=(70.5, 10.25, 130.0, 63.75))    # chunks x 1 .. 2, y 0: not a rectangle of pixels
CASES["seeded-clear-edge-size4"] = case(tool(CROSS, 4, color=GREEN), preview="seeded", last=(128.0, 64.0, 250.0, 500.0))   # min on a chunk border, max beyond the canvas
CASES["seeded-clear-away-from-the-line"] = case(tool(TO_THE_RIGHT, 4, color=GREEN, end_shape=1), preview="seeded", last=(150.0, 90.0, 199.0, 135.5), sel=True)
NAMES = sorted(CASES)
PIECE_CASE, PIECE_LIMIT = "cap5000-size1", 1500   # chunk-list entries per launch: 5001 dots, so at least four pieces (asserted on the host)


@functools.lru_cache(maxsize=None)
def selection(w, h):
    """zero blocks of 5 x 3 pixels on a 11 x 7 lattice, plus a zero band: dot centres fall into zero cells while their neighbours paint around them"""
    sel = np.full((h, w), 255, np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    sel[((xs % 11) < 5) & ((ys % 7) < 3)] = 0
    sel[:, 116:124] = 0                   # under part of TO_THE_RIGHT's end head
    sel[(xs + ys) % 13 == 0] = 1          # any non-zero byte selects
    sel.setflags(write=False)
    return sel


@functools.lru_cache(maxsize=None)
def seeded_preview(w, h):
    """another colour everywhere, alpha in vertical bands of 9: below, equal to and above GREEN's 128, and 0"""
    pv = np.zeros((h, w, 4), np.uint8)
    pv[..., 0], pv[..., 1], pv[..., 2] = 90, 60, 200
    pv[..., 3] = np.array([100, 128, 200, 0, 127, 129], np.uint8)[(np.arange(w) // 9) % 6][None, :]
    pv.setflags(write=False)
    return pv


def preview_of(c):
    return seeded_preview(c["w"], c["h"]) if c["preview"] == "seeded" else np.zeros((c["h"], c["w"], 4), np.uint8)


def last_of(c):
    return None if c["last"] == "all" else ((0.0, 0.0, 0.0, 0.0) if c["last"] == "none" else c["last"])


def selection_of(c, use_sel=None):
    return selection(c["w"], c["h"]) if (c["sel"] if use_sel is None else use_sel) else None


@functools.lru_cache(maxsize=None)
def expected(name, use_sel=None, form="serial"):
    """(preview, bounds, stats) of the model for the case; use_sel overrides the case's own choice"""
    c = CASES[name]
    out, b, st = M.render(c["tool"], preview_of(c), selection_of(c, use_sel), last_of(c), form)
    out.setflags(write=False)
    return out, b, st


# a two-frame drag: frame 2 uses frame 1's bounds, whose chunks hold all of frame 1; the end point moves to another chunk row
DRAG = [tool([(20.0, 20.0), (60.0, 20.0), (90.0, 40.0), (140.0, 50.0)], 5.9, color=GREEN, end_shape=1, arrow_side=0),
        tool([(20.0, 20.0), (60.0, 20.0), (90.0, 40.0), (100.0, 110.0)], 5.9, color=GREEN, end_shape=1, arrow_side=0)]


def commit_inputs():
    """old and s over all 256 x 256 pairs in one 256 x 256 image"""
    old = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    pv = np.zeros((256, 256, 4), np.uint8)
    pv[..., 3] = np.arange(256, dtype=np.uint8)[None, :]
    pv[..., :3] = 33
    return np.ascontiguousarray(old), pv
