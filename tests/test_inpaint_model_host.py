"""The content-aware fill CPU model (tests/inpaint_model.py) against the reference's two inpaint goldens, the sweeps' counters, and
pfx_inpaint_ring_offsets against the model (no GPU).

* The model reproduces `inpaint/instant_brush_center` and `inpaint/patchmatch_checkerboard` at tolerance 0.  The instant golden is weak — on its input the
  routine changes no pixel — which is why every sweep case is held to a counter: at least 20 changed pixels, or exactly 0 where the case says "nothing".
* The PatchMatch sweep reaches what it is named for: every patch size and both iteration counts, a hole at least 4 peels deep, the sequential-f32 SSD branch
  (integer sum >= 2^24), boundary pixels left unfilled.
* The integer SSD of the model equals its line-by-line f32 form.
* pfx_inpaint_ring_offsets equals the model's 64 floats bit for bit."""
import ctypes as C

import numpy as np
import pytest

from paintfe_amd import _lib, inpaint_ring_offsets

from . import inpaint_cases as IC
from . import inpaint_model as M


@pytest.fixture(scope="module")
def goldens():
    return IC.load_goldens()


def test_model_reproduces_the_instant_golden(goldens):
    src, mask, out, dabs = IC.golden_instant()
    img, changed = M.instant_list(src, mask, out, dabs)
    assert np.array_equal(img, goldens["inpaint/instant_brush_center"])
    assert changed == 0      # the golden's weakness, on record


def test_model_reproduces_the_patchmatch_golden(goldens):
    src, mask, ps, iters = IC.golden_patchmatch()
    img, k = M.patchmatch(src, mask, ps, iters)
    assert np.array_equal(img, goldens["inpaint/patchmatch_checkerboard"])
    assert k["peels"] == 8 and k["unfilled"] == 0 and k["big_sums"] == 0


@pytest.mark.parametrize("case", IC.instant_cases(), ids=lambda c: c[0])
def test_instant_sweep_cases_change_pixels(case):
    name, src, mask, out, dabs, expect = case
    img, changed = M.instant_list(src, mask, out, dabs)
    print(name, "pixels changed:", changed)
    assert src.shape == IC.instant_canvas(name)[::-1] + (4,)
    if expect == "nothing":
        assert changed == 0 and np.array_equal(img, out)
    else:
        assert changed >= 20
    assert np.array_equal(img[mask == 0], out[mask == 0])      # only painted-over pixels are touched


def test_instant_sweep_holds_what_it_is_named_for():
    cases = {c[0]: c for c in IC.instant_cases()}
    assert {0.0, 0.5, 1.0} <= {d[4] for c in cases.values() for d in c[4]}
    assert any(d[0] != int(d[0]) and d[1] != int(d[1]) for d in cases["fractional_centre"][4])
    assert set(np.unique(cases["mask_values_1_200_255"][2])) == {0, 1, 200, 255}
    assert not cases["transparent_out_noise"][3].any()
    five = cases["five_overlapping_dabs"][4]
    assert len(five) == 5 and len({d[3] for d in five}) == 2


def test_second_instant_canvas_holds_what_it_is_named_for():
    cases = {c[0]: c for c in IC.instant_cases()}
    W, H = IC.SWEEP2_W, IC.SWEEP2_H
    assert W % 64 and W % 4 and H % 4 and W > 4 * 64 and H > 4 * 4 and {IC.instant_canvas(n) for n in cases} == {(IC.SWEEP_W, IC.SWEEP_H), (W, H)}

    def boxes(dabs):   # the dabs' pixel loop bounds (inpaint.rs:93-96) through the model's own conversions
        out = []
        for cx, cy, r, _, _ in dabs:
            cx, cy, r = M.f32(cx), M.f32(cy), max(M.f32(r), M.f32(1.0))
            out.append((M.as_u32(max(cx - r, M.f32(0.0))), M.as_u32(max(cy - r, M.f32(0.0))), min(M.as_u32(np.ceil(cx + r)), W - 1), min(M.as_u32(np.ceil(cy + r)), H - 1)))
        return np.array(out)

    walk = boxes(cases["walk_300_dabs"][4])
    assert len(walk) == 300 and len({d[3] for d in cases["walk_300_dabs"][4]}) == 5
    assert walk[:, 0].min() == 0 and walk[:, 1].min() == 0 and walk[:, 2].max() == W - 1 and walk[:, 3].max() >= H - 3      # the union box is almost the canvas
    far = boxes(cases["two_far_corners"][4])
    union = (far[:, 2].max() - far[:, 0].min() + 1) * (far[:, 3].max() - far[:, 1].min() + 1)
    own = ((far[:, 2] - far[:, 0] + 1) * (far[:, 3] - far[:, 1] + 1)).sum()
    assert len(far) == 2 and union >= 0.95 * W * H and own < 0.02 * union      # almost every thread of the launch has no dab
    name, src, mask, out, dabs, _ = cases[IC.CHAIN_65]
    chain = boxes(dabs)
    assert len(dabs) == 65
    for a, b, d in zip(chain, chain[1:], dabs[1:]):      # dab k's pixel box overlaps dab k - 1's, and its sample ring (radius > the spacing) reaches back over it
        assert b[0] <= a[2] and b[1] <= a[3] and a[1] <= b[3] and d[3] > 3.5 + d[2]
    step_by_step = out
    written = np.zeros(mask.shape, bool)
    rewritten = 0
    for d in dabs:
        nxt, _ = M.instant(src, mask, step_by_step, *d)
        touched = (nxt != step_by_step).any(-1)
        rewritten += int((touched & written).sum())
        written |= touched
        step_by_step = nxt
    assert rewritten >= 20                                                      # later dabs change pixels earlier dabs wrote
    assert not np.array_equal(step_by_step, M.instant_list(src, mask, out, dabs[::-1])[0])      # so the order matters


EDGE_CONDITIONS = {      # hole shape -> (what must hold, spelt for the failure message; a function of the mask and the model's first peel)
    "antidiag_band": ("more than 2 rounds of 16 waves on one anti-diagonal of the first peel",
                      lambda mask, first, box: np.bincount([x + y for x, y in first]).max() > 2 * IC.PM_PASS_WAVES),
    "maindiag_band": ("diagonals of one or two pixels between empty diagonals inside the box",
                      lambda mask, first, box: np.bincount([x + y for x, y in first]).max() <= 2 and
                      (np.bincount([x + y - box[0] - box[1] for x, y in first], minlength=box[2] + box[3] - 1) == 0).sum() >= 20),
    "stripe": ("a first peel of more than 1024 boundary pixels", lambda mask, first, box: len(first) > IC.PM_BLOCK_THREADS),
    "far_corners": ("more than 1024 diagonals in the box, hundreds of compaction blocks",
                    lambda mask, first, box: box[2] + box[3] - 1 > IC.PM_BLOCK_THREADS and -(-box[2] * box[3] // IC.PM_COMPACT_ELEMS) >= 200),
    # the peels' own compaction (over the box) takes the second turn of pm_scan_kernel, and boundary pixels get their list offsets from it: box element
    # (y - y0) * bw + (x - x0) lies in a block at or past 1024, so a lost carry drops them onto the first hole's list entries
    "both_corners": ("more than 1024 compaction blocks over the box and over the canvas, first-peel boundary pixels in a block at or past 1024",
                     lambda mask, first, box: -(-box[2] * box[3] // IC.PM_COMPACT_ELEMS) > IC.PM_BLOCK_THREADS and
                     -(-mask.size // IC.PM_COMPACT_ELEMS) > IC.PM_BLOCK_THREADS and
                     0 < sum(((y - box[1]) * box[2] + (x - box[0])) // IC.PM_COMPACT_ELEMS >= IC.PM_BLOCK_THREADS for x, y in first) < len(first)),
    "full_cross": ("the box is the canvas", lambda mask, first, box: box == (0, 0, mask.shape[1], mask.shape[0])),
    "one_pixel": ("the patch is larger than the canvas", None),
    "two_pixels": ("the patch is larger than the canvas", None),
}


@pytest.mark.parametrize("spec", IC.PATCHMATCH_EDGES, ids=IC.patchmatch_id)
def test_patchmatch_edge_cases_cross_their_edges(spec):
    (w, h), shape, content, ps, iters = spec
    src, mask, _, _ = IC.patchmatch_case(spec)
    img, k, trace = IC.patchmatch_expected(spec)
    hole = mask > 0
    ys, xs = np.nonzero(hole)
    box = (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))      # x0, y0, bw, bh
    first = trace[0]
    diag = int(np.bincount([x + y for x, y in first]).max())
    print(IC.patchmatch_id(spec), k, "hole", int(hole.sum()), "first peel", len(first), "largest diagonal", diag, "bw + bh - 1 =", box[2] + box[3] - 1,
          "box blocks", -(-box[2] * box[3] // IC.PM_COMPACT_ELEMS), "canvas blocks", -(-w * h // IC.PM_COMPACT_ELEMS))
    what, holds = EDGE_CONDITIONS[shape]
    if shape in ("one_pixel", "two_pixels"):
        assert max(ps, 3) > min(w, h), what      # no patch of the canvas is whole: every query and every candidate is clipped
    else:
        assert holds(mask, first, box), what
    assert k["peels"] >= 1 and len(trace) == k["peels"] and sum(len(t) for t in trace) == int(hole.sum())
    changed = int((img[hole] != src[hole]).any(-1).sum())
    assert np.array_equal(img[~hole], src[~hole])
    if spec == IC.NEVER_FILLABLE:
        assert changed == 0 and k["unfilled"] == 1      # min_valid 30 on a canvas of 20 pixels: see inpaint_cases.NEVER_FILLABLE
    else:
        assert changed >= 1


def test_patchmatch_edges_hold_what_they_are_named_for():
    specs = IC.PATCHMATCH_EDGES
    assert {s[3] for s in specs} >= {3, 5, 7, 9, 11} and {s[4] for s in specs} == {3, 6}
    band = [s for s in specs if s[1] == "antidiag_band"]
    assert {s[3] for s in band} == {5, 7} and {s[4] for s in band} == {3, 6}      # forward and backward passes alike: 2 passes and 4
    assert len({IC.patchmatch_id(s) for s in specs} | {IC.patchmatch_id(s) for s in IC.PATCHMATCH_SWEEP}) == len(specs) + len(IC.PATCHMATCH_SWEEP)
    tiny = [s for s in specs if s[1] in ("one_pixel", "two_pixels")]
    assert {s[0] for s in tiny} >= {(5, 4), (3, 9)} and {s[3] for s in tiny} >= {7, 11}
    assert any(s[3] ** 2 > 64 and s != IC.NEVER_FILLABLE for s in tiny)      # a fill through the second half of the wave's 2 x 64 patch slots
    a, b, c = IC.GEOMETRY_SEQUENCE
    assert a[1] == "far_corners" and b in IC.PATCHMATCH_SWEEP and c[1] == "stripe"
    assert (IC.PM_PASS_WAVES, IC.PM_BLOCK_THREADS, IC.PM_COMPACT_ELEMS) == (16, 1024, 1024)


def test_the_peel_trace_changes_nothing():
    spec = IC.PATCHMATCH_SWEEP[2]
    plain_img, plain_k = M.patchmatch(*IC.patchmatch_case(spec))
    trace = []
    img, k = M.patchmatch(*IC.patchmatch_case(spec), trace=trace)
    assert np.array_equal(img, plain_img) and k == plain_k and len(trace) == k["peels"]


def test_patchmatch_sweep_holds_what_it_is_named_for():
    specs = IC.PATCHMATCH_SWEEP
    assert {s[3] for s in specs} >= {3, 4, 5, 7, 9, 11} and {s[4] for s in specs} == {3, 6}
    assert {s[0] for s in specs} == {(61, 45), (64, 64)} and {s[2] for s in specs} >= {"palette", "gradnoise", "bw_split"}
    assert {s[1] for s in specs} >= {"corner", "edge", "two", "L", "ring", "blob", "deep"}
    for s in specs:
        _, mask, _, _ = IC.patchmatch_case(s)
        assert 0 < int((mask > 0).sum()) <= 260
    assert set(np.unique(IC.patchmatch_case(specs[5])[1])) == {0, 1, 200, 255}


@pytest.fixture(scope="module")
def sweep_counters():
    return {IC.patchmatch_id(s): M.patchmatch(*IC.patchmatch_case(s))[1] for s in IC.PATCHMATCH_SWEEP if s[1] in ("deep", "small", "ring_pixel_island")}


def test_patchmatch_sweep_counters(sweep_counters):
    for name, k in sweep_counters.items():
        print(name, k)
    assert all(k["peels"] >= 4 for n, k in sweep_counters.items() if "-deep-" in n)
    assert sweep_counters["64x64-small-bw_split-p11-i3"]["big_sums"] > 0
    assert sweep_counters["64x64-ring_pixel_island-palette-p3-i3"]["unfilled"] > 0
    assert sweep_counters["61x45-ring_pixel_island-gradnoise-p1-i6"]["unfilled"] > 0


def test_integer_ssd_equals_the_sequential_f32_ssd():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 40, 4), dtype=np.uint8)
    bw = np.zeros((40, 40, 4), np.uint8)
    bw[:, 20:, :3] = 255
    mask = (rng.random((40, 40)) < 0.15).astype(np.uint8) * 255
    k = M._Counters()
    for image in (img, bw):
        for _ in range(150):
            ax, ay, bx, by = (int(v) for v in rng.integers(0, 40, 4))
            half = int(rng.integers(1, 6))
            mv = max((2 * half + 1) ** 2, 4) // 4
            a, b = M._ssd(image, mask, ax, ay, bx, by, half, mv, k), M.ssd_sequential(image, mask, ax, ay, bx, by, half, mv)
            assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)
    assert k.big_sums > 0


@pytest.mark.parametrize("radius", [24.0, 18.0, 0.5, 1000.0])
def test_ring_offsets_match_the_model(radius):
    assert np.array_equal(inpaint_ring_offsets(radius).view(np.uint32), M.ring_offsets(radius).view(np.uint32))


def test_ring_offsets_null_out_is_a_no_op():
    fn = _lib.load().pfx_inpaint_ring_offsets
    fn.restype = None
    fn(C.c_float(24.0), C.c_void_p(None))
