"""No device: the tables of tests/gauss_valu_cases.py are held to the rules they restate, and shown to be able to see what they are for.

  * pfxk_gauss_v_tile (the one tile decision of the VALU Gaussian's vertical pass, k_gauss.hip) against a table written out here from the rules,
    at every switch point from both sides and under every forced value of the "gauss_v_cfg" knob;
  * the LDS bytes of both passes at every radius 1 .. 850 stay within 160 KiB (what a workgroup can be granted);
  * a numpy float32 restatement of the reference (separate multiply and add, ascending taps, clamp to edge, H then V, round half away) equals
    the oracle byte for byte on every (radius, shape) row, and on each radius's tall and wide row four mutants of it (first / last / centre tap
    dropped, far edge clamped at n - 2) each change at least 8 bytes: a kernel wrong in one of these ways cannot pass the GPU tests' rows.
    A descending-order mutant changes next to nothing on these inputs; its count is printed (run with -s), not asserted: the rows do not
    claim to see the summation order."""
import numpy as np
import pytest

from . import gauss_model as G
from . import gauss_valu_cases as V
from . import oracle_lib as O

# ---- the tile decision, written out from launch_v's rules -----------------------------------------------------------------------------------
# knob low byte 0: by radius
AUTO = [  # (first radius, last radius, config)
    (1, 110, 0),      # default: 8 columns x 128 rows
    (111, 160, 1),    # 16 x 256
    (161, 240, 4),    # 8 x 512
    (241, 340, 3),    # 8 x 256
    (341, 380, 0),    # 8 x 128 again
    (381, 850, 2),    # 4 x 256, LDS row stride 5
]
# knob low byte k: forced up to radius 340; launch_v ignores the knob above
FORCED = {k: [(1, 340, k), (341, 380, 0), (381, 850, 2)] for k in (1, 2, 3, 4)}
FORCED.update({k: [(1, 380, 0), (381, 850, 2)] for k in (5, 6, 255)})   # a byte that names no shape: config 0, at every radius the knob governs
TILES = {0: (8, 128, 10), 1: (16, 256, 16), 2: (4, 256, 5), 3: (8, 256, 10), 4: (8, 512, 10)}   # config -> columns, rows, LDS row stride (float4)


def lds_of(cfg, r):
    tx, rows, rs = TILES[cfg]
    return (rows + 2 * r + 4) * rs * 16


def check_ranges(ranges, knob):
    assert ranges[0][0] == 1 and ranges[-1][1] == V.MAX_RADIUS and all(a[1] + 1 == b[0] for a, b in zip(ranges, ranges[1:])), "the table has a gap"
    for lo, hi, cfg in ranges:
        for r in sorted({lo, lo + 1, (lo + hi) // 2, hi - 1, hi} & set(range(lo, hi + 1))):
            got = V.v_tile(r, knob)
            assert got == (cfg, TILES[cfg][0], TILES[cfg][1], lds_of(cfg, r)), (knob, r, got, cfg)


def test_limits_match_the_tables():
    assert V.max_radius() == V.MAX_RADIUS
    assert V.V_TILES == tuple(TILES[k] for k in range(5))
    assert max(V.RADII) == V.MAX_RADIUS


def test_tile_decision_by_radius():
    check_ranges(AUTO, 0)
    check_ranges(AUTO, 0x200)   # the bits above the low byte belong to development tools: not a shape
    for a, b in ((110, 111), (160, 161), (240, 241), (340, 341), (380, 381)):
        assert V.v_tile(a)[0] != V.v_tile(b)[0], (a, b)
        assert a in V.RADII and b in V.RADII, "the radius table misses a side of a switch point"


@pytest.mark.parametrize("knob", sorted(FORCED))
def test_tile_decision_under_a_forced_knob(knob):
    check_ranges(FORCED[knob], knob)
    check_ranges(FORCED[knob], knob | 0x4000)
    for r in (341, 380, 381, 850):
        assert V.v_tile(r, knob) == V.v_tile(r, 0), f"the knob reaches radius {r}"


def test_output_pointers_are_optional():
    import ctypes as C
    lib = V._lib()
    assert lib.pfxk_gauss_v_tile(200, 0, None, None, None) == 4
    rows = C.c_int(0)
    assert lib.pfxk_gauss_v_tile(200, 3, None, C.byref(rows), None) == 3 and rows.value == 256


def test_forced_rows_fit_and_the_refusal_row_does_not():
    for r, knobs in V.FORCED.items():
        for k in knobs:
            cfg, tx, rows, lds = V.v_tile(r, k)
            assert lds <= V.LDS_LIMIT, (r, k, lds)
            if k:
                assert cfg == k
    assert V.v_tile(254, 1)[3] > V.LDS_LIMIT, "254 leaves config 1 out because it does not fit"
    assert V.v_tile(254, 4)[3] == V.LDS_LIMIT and V.v_tile(255, 4)[3] > V.LDS_LIMIT, "254 is the 8 x 512 tile's last radius"
    r, k = V.REFUSED
    cfg, tx, rows, lds = V.v_tile(r, k)
    assert cfg == k and lds == (260 + 600) * 256 and lds > V.LDS_LIMIT


def test_lds_stays_within_a_workgroups_share_at_every_radius():
    for r in range(1, V.MAX_RADIUS + 1):
        cfg, tx, rows, lds = V.v_tile(r, 0)
        assert 0 < lds <= V.LDS_LIMIT, f"vertical pass, radius {r}: config {cfg} asks for {lds} B"
        assert lds == lds_of(cfg, r)
        e = 1024 + 2 * r + 12   # launch_h: the staged row segment, one pad slot per 4 entries, one entry of slack
        hb = V.h_lds_bytes(r)
        assert hb == (e + e // 4 + 1) * 16 and hb <= V.LDS_LIMIT, f"horizontal pass, radius {r}: {hb} B"


# ---- the rows: the restatement equals the oracle, and the long rows see the mutants -------------------------------------------------------------

def changed(a, b):
    return int((a != b).sum())


@pytest.mark.parametrize("radius", V.RADII)
def test_restatement_equals_the_oracle_and_the_rows_see_the_mutants(radius):
    sigma = G.sigma_for_radius(radius)
    taps = O.gaussian_kernel(sigma)
    assert len(taps) == 2 * radius + 1
    rows = V.shapes(radius)
    assert len(set(rows)) == len(rows)
    for (w, h) in rows:
        img = V.image(w, h, radius)
        want = V.oracle(w, h, radius)
        hx = V.one_pass(img, taps, 1)
        got = V.round_half_away(V.one_pass(hx, taps, 0))
        assert np.array_equal(got, want), f"r={radius} {w}x{h}: the restatement differs from the oracle in {changed(got, want)} bytes"
        tall, wide = (w, h) == V.tall_shape(radius), (w, h) == V.wide_shape(radius)
        if not (tall or wide):
            continue
        assert len(np.unique(want)) >= 32, f"r={radius} {w}x{h}: the result sits on {len(np.unique(want))} byte values"

        def mutant(**kw):   # in the pass along the long axis; the other pass is the reference's
            if tall:
                return V.round_half_away(V.one_pass(hx, taps, 0, **kw))
            return V.round_half_away(V.one_pass(V.one_pass(img, taps, 1, **kw), taps, 0))

        for name, kw in V.mutants(radius, h if tall else w).items():
            n = changed(mutant(**kw), want)
            print(f"gauss_valu_cases: r={radius} {w}x{h} {name}: {n} bytes change")
            assert n >= 8, f"r={radius} {w}x{h}: the mutant '{name}' changes {n} bytes: this row's image cannot see it"
        print(f"gauss_valu_cases: r={radius} {w}x{h} descending taps: {changed(mutant(descending=True), want)} bytes change (not asserted)")
