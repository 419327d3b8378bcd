"""Which median kernel and which box-blur kernels run for a call: the two host-side decisions (pfx_stencil.cpp), exported as the test seams
pfx_int_median_path and pfx_int_box_plan (pfx_internal.h), against tables written out here from the rules.  No device: both are pure functions.

Median, r = max(radius, 1), the first rule that matches:
  * r beyond PFX_MEDIAN_MAX_RADIUS: unsupported;
  * max(bits_min, 2) <= r <= 8, unless r = 3 and pfx_tune "median_xlane" has bit 2: the bit-plane select, the column-pair kernel when "median_pair" is on and r <= 7;
  * r = 1: the 3x3 network;
  * r = 3, xlane bit 2, not "median_single": the 7x7 cross-lane network;
  * r = 2, xlane & 3 != 0, not single: the 5x5 cross-lane network, two rows per lane when xlane & 3 == 2;
  * 2 <= r <= 4, not single: the shared-column networks;  r in {2, 3}: the single-window networks;
  * r beyond PFXK_MEDIAN_TILE_MAX_RADIUS: the sliding histogram;  otherwise the value search, one pixel per lane under "median_search1", else four.
Box blur, fused_ok = not in place and not "box_two_pass":
  * fused_ok, r <= the tile kernel's limit, "box_strip" != 2: the tile kernel;
  * fused_ok, box_strip != 0, r <= the strip walk's limit, r beyond the tile limit or box_strip = 2, w * h < 2^29: the strip walk;
  * otherwise two passes: the horizontal one on prefix sums when "box_prefix_from" > 0, r >= it, "box_px" = 0 and r within the prefix kernel's LDS limit;
  * columns per lane: box_px 4 / 8 as given, any other non-zero value 16; 0: 8 below "box_px_switch", else 16;
  * rows per lane: box_py 16 / 32 / 64 as given, any other non-zero value 128; 0: 16 below "box_py_switch", 64 below twice that, else 128.

The limits are queried or read from the headers, so the tables are written per radius CLASS."""
import ctypes as C
import itertools
import os
import re

import pytest

from paintfe_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pfx_kernels.h: PFX_MEDIAN_*
MEDIAN = {"U": -1, "N": 0, "X": 1, "R": 2, "7": 3, "H": 4, "G": 5, "P": 6, "b": 7, "4": 8, "1": 9, "I": 10}
# unsupported, 3x3 net, cross-lane, cross-lane two rows, cross-lane 7x7, shared columns, single-window net, bits pair, bits, search4, search1, histogram.
# In the tables: B = "P" with median_pair, else "b";  S = "1" with median_search1, else "4"
M_COLS = ("1", "2", "3", "4", "5-7", "8", "search", "hist", "beyond")
# (bits_min values, xlane values, single values) -> a letter per radius class
M_TABLE = [
    ((9,), (0,), (0,), "NHHHSSSIU"),            # no bit-plane select: the networks and the search alone
    ((9,), (1, 3), (0,), "NXHHSSSIU"),          # xlane & 3 = 3 is not 2: one row per lane
    ((9,), (2,), (0,), "NRHHSSSIU"),
    ((9,), (5,), (0,), "NX7HSSSIU"),
    ((9,), (0, 1, 2, 3, 5), (1,), "NGGSSSSIU"),   # single: radius 4 has no single-window network and takes the search
    ((3,), (0,), (0,), "NHBBBbSIU"),            # the default bits_min
    ((3,), (1, 3), (0,), "NXBBBbSIU"),
    ((3,), (2,), (0,), "NRBBBbSIU"),
    ((3,), (5,), (0,), "NX7BBbSIU"),            # xlane bit 2 keeps radius 3 off the bit planes ...
    ((3,), (0, 1, 2, 3), (1,), "NGBBBbSIU"),
    ((3,), (5,), (1,), "NGGBBbSIU"),            # ... single or not
    ((1, 2), (0, 1, 2, 3), (0, 1), "NBBBBbSIU"),   # bits_min below 2 means 2: radius 1 stays on the 3x3 network
    ((1, 2), (5,), (0,), "NB7BBbSIU"),
    ((1, 2), (5,), (1,), "NBGBBbSIU"),
]
M_DEFAULTS = dict(bits_min=3, xlane=1, single=0, search1=0, pair=1)                                   # pfx_stencil.cpp, pfx_internal.h
B_DEFAULTS = dict(strip=2, two_pass=0, prefix_from=72, px_force=0, py_force=0, px_switch=12, py_switch=20)

TILE, STRIP, TWO_PASS = range(3)   # pfx_kernels.h: PFX_BOX_*
SLIDING, PREFIX = range(2)
BOX = {"T": TILE, "S": STRIP, "P": TWO_PASS}
# (fused_ok, box_strip, w * h below 2^29) -> kind per radius class: within the tile limit | within the strip limit | beyond
B_KIND = {
    (1, 0, 1): "TPP", (1, 0, 0): "TPP",
    (1, 1, 1): "TSP", (1, 1, 0): "TPP",
    (1, 2, 1): "SSP", (1, 2, 0): "PPP",
    (0, 0, 1): "PPP", (0, 0, 0): "PPP", (0, 1, 1): "PPP", (0, 1, 0): "PPP", (0, 2, 1): "PPP", (0, 2, 0): "PPP",
}
B_RADII = (1, 4, 5, 19, 20, 39, 40, 60, 61, 71, 72, 700, 2039)
# px_switch 12, py_switch 20: radius -> (columns, rows) per lane by radius
B_LANE_RUNS = {1: (8, 16), 4: (8, 16), 5: (8, 16), 19: (16, 16), 20: (16, 64), 39: (16, 64), 40: (16, 128), 60: (16, 128), 61: (16, 128), 71: (16, 128),
               72: (16, 128), 700: (16, 128), 2039: (16, 128)}
B_SIZES = ((1 << 15, (1 << 14) - 1), (1 << 15, 1 << 14))   # w * h = 2^29 - 2^15 and 2^29


class MedianCase(C.Structure):   # pfx_internal.h: pfx_median_case
    _fields_ = [(n, C.c_int) for n in ("radius", "bits_min", "xlane", "single", "search1", "pair")]


class BoxCase(C.Structure):   # pfx_internal.h: pfx_box_case
    _fields_ = [("radius", C.c_int), ("in_place", C.c_int), ("w", C.c_uint32), ("h", C.c_uint32)] + \
               [(n, C.c_int) for n in ("strip", "two_pass", "prefix_from", "px_force", "py_force", "px_switch", "py_switch")]


class BoxPlan(C.Structure):   # pfx_kernels.h: pfx_box_plan
    _fields_ = [(n, C.c_int) for n in ("kind", "h_kind", "px", "py")]


def _define(header, name):
    text = open(os.path.join(ROOT, *header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


MEDIAN_MAX = _define(("include", "pfx.h"), "PFX_MEDIAN_MAX_RADIUS")
MEDIAN_TILE_MAX = _define(("paintfe_amd", "csrc", "pfx_kernels.h"), "PFXK_MEDIAN_TILE_MAX_RADIUS")


@pytest.fixture(scope="module")
def lib():
    L = _lib.load()
    L.pfx_int_median_path.argtypes = [C.POINTER(MedianCase)]
    L.pfx_int_median_path.restype = C.c_int
    L.pfx_int_box_plan.argtypes = [C.POINTER(BoxCase), C.POINTER(BoxPlan)]
    L.pfx_int_box_plan.restype = C.c_int
    for f in ("pfxk_box_tile_max_radius", "pfxk_box_strip_max_radius", "pfxk_box_prefix_max_radius"):
        getattr(L, f).argtypes = []
        getattr(L, f).restype = C.c_int
    return L


def median_path(lib, radius, **knobs):
    k = dict(M_DEFAULTS, **knobs)
    c = MedianCase(radius, k["bits_min"], k["xlane"], k["single"], k["search1"], k["pair"])
    return lib.pfx_int_median_path(C.byref(c))


def box_plan(lib, radius, in_place=0, w=256, h=256, **knobs):
    k = dict(B_DEFAULTS, **knobs)
    c = BoxCase(radius, in_place, w, h, k["strip"], k["two_pass"], k["prefix_from"], k["px_force"], k["py_force"], k["px_switch"], k["py_switch"])
    p = BoxPlan(-1, -1, -1, -1)
    kind = lib.pfx_int_box_plan(C.byref(c), C.byref(p))
    assert kind == p.kind
    return p


def median_column(radius):
    if radius > MEDIAN_MAX:
        return "beyond"
    if radius > MEDIAN_TILE_MAX:
        return "hist"
    return {1: "1", 2: "2", 3: "3", 4: "4", 5: "5-7", 6: "5-7", 7: "5-7", 8: "8"}.get(radius, "search")


def test_limits_are_sane(lib):
    assert 8 < MEDIAN_TILE_MAX < MEDIAN_MAX
    assert 1 <= lib.pfxk_box_tile_max_radius() < lib.pfxk_box_strip_max_radius() < lib.pfxk_box_prefix_max_radius()


def test_median_path_table(lib):
    radii = sorted({1, 2, 3, 4, 5, 7, 8, 9, MEDIAN_TILE_MAX, MEDIAN_TILE_MAX + 1, MEDIAN_MAX, MEDIAN_MAX + 1})
    seen, cells = set(), set()
    for bits_mins, xlanes, singles, row in M_TABLE:
        for bits_min, xlane, single, search1, pair, radius in itertools.product(bits_mins, xlanes, singles, (0, 1), (0, 1), radii):
            letter = row[M_COLS.index(median_column(radius))]
            letter = {"B": "P" if pair else "b", "S": "1" if search1 else "4"}.get(letter, letter)
            got = median_path(lib, radius, bits_min=bits_min, xlane=xlane, single=single, search1=search1, pair=pair)
            assert got == MEDIAN[letter], (radius, bits_min, xlane, single, search1, pair, got, letter)
            seen.add(got)
            cells.add((bits_min, xlane, single))
    assert cells == set(itertools.product((1, 2, 3, 9), (0, 1, 2, 3, 5), (0, 1))), "the table covers every knob combination"
    assert seen == set(MEDIAN.values()), "every path is reached"


def test_median_defaults_give_the_shipped_routes(lib):
    shipped = {1: "N", 2: "X", 8: "b"}
    shipped.update({r: "P" for r in range(3, 8)})
    shipped.update({r: "4" for r in range(9, MEDIAN_TILE_MAX + 1)})
    shipped.update({r: "I" for r in range(MEDIAN_TILE_MAX + 1, MEDIAN_MAX + 1)})
    shipped[MEDIAN_MAX + 1] = "U"
    for radius, letter in shipped.items():
        assert median_path(lib, radius) == MEDIAN[letter], radius


def box_column(lib, radius):
    return 0 if radius <= lib.pfxk_box_tile_max_radius() else (1 if radius <= lib.pfxk_box_strip_max_radius() else 2)


@pytest.mark.parametrize("strip", [0, 1, 2])
@pytest.mark.parametrize("two_pass", [0, 1])
@pytest.mark.parametrize("in_place", [0, 1])
def test_box_plan_table(lib, in_place, two_pass, strip):
    kinds, h_kinds, pxs, pys = set(), set(), set(), set()
    for (w, h), prefix_from, px_force, py_force, radius in itertools.product(B_SIZES, (0, 1, 72), (0, 4, 8, 16), (0, 16, 32, 64, 128), B_RADII):
        small = int(w * h < 1 << 29)
        p = box_plan(lib, radius, in_place, w, h, strip=strip, two_pass=two_pass, prefix_from=prefix_from, px_force=px_force, py_force=py_force)
        what = (radius, in_place, w, h, strip, two_pass, prefix_from, px_force, py_force)
        kind = BOX[B_KIND[(int(not in_place and not two_pass), strip, small)][box_column(lib, radius)]]
        assert p.kind == kind, what
        prefix = kind == TWO_PASS and px_force == 0 and {0: False, 1: True, 72: radius >= 72}[prefix_from]   # every radius here is within the prefix limit
        assert p.h_kind == (PREFIX if prefix else SLIDING), what
        assert p.px == (px_force or B_LANE_RUNS[radius][0]), what
        assert p.py == (py_force or B_LANE_RUNS[radius][1]), what
        kinds.add(p.kind), h_kinds.add(p.h_kind), pxs.add(p.px), pys.add(p.py)
    assert h_kinds == ({SLIDING, PREFIX} if TWO_PASS in kinds else {SLIDING})
    assert pxs == {4, 8, 16} and pys == {16, 32, 64, 128}
    want = {"T", "S", "P"} if (not in_place and not two_pass and strip == 1) else None
    if want:
        assert kinds == {BOX[k] for k in want}, "every kind is reached"


def test_box_lane_runs_follow_their_switches_and_odd_forces_saturate(lib):
    for radius in (11, 12, 23, 24, 47, 48):
        p = box_plan(lib, radius, strip=0, px_switch=24, py_switch=12)
        assert (p.px, p.py) == (8 if radius < 24 else 16, 16 if radius < 12 else (64 if radius < 24 else 128)), radius
    p = box_plan(lib, 9, strip=0, px_force=5, py_force=100)
    assert (p.kind, p.h_kind, p.px, p.py) == (TWO_PASS, SLIDING, 16, 128)


def test_box_prefix_pass_stops_at_its_lds_limit(lib):
    limit = lib.pfxk_box_prefix_max_radius()
    assert box_plan(lib, limit, prefix_from=1).h_kind == PREFIX
    assert box_plan(lib, limit + 1, prefix_from=1).h_kind == SLIDING
    assert box_plan(lib, limit, prefix_from=0).h_kind == SLIDING


def test_box_defaults_give_the_shipped_routes(lib):
    strip_max = lib.pfxk_box_strip_max_radius()
    for radius in range(1, strip_max + 1):
        assert box_plan(lib, radius).kind == STRIP, radius
        assert box_plan(lib, radius, in_place=1).kind == TWO_PASS, radius
    for radius in (strip_max + 1, 71, 72, 700, 2039):
        p = box_plan(lib, radius)
        assert (p.kind, p.h_kind) == (TWO_PASS, PREFIX if radius >= 72 else SLIDING), radius
