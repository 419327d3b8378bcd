"""Parity (GPU): the brush engine at its edges — every row of tests/brush_cases.py against the CPU oracle at tolerance 0, under each `brush_binning`
setting the row names, so that the binned kernel, the bounding-box kernel and the oracle give one image.  What the table reaches is shown on the host by
tests/test_brush_cases_host.py.

Non-finite centres are ordinary rows: the stamp prologue (pfx_brush_stamps_ex_dev) gives a NaN / inf centre the pixel box the reference's casts give it
(brush_render.rs:208-215, 584-587) and launches over the union of the stamps' boxes, so a NaN stamp paints column / row 0 whether it is first, in the
middle or last and whichever kernel runs.  Before that the bounding-box launch took its box from min / max over the centres — which skip a NaN that is
not first, so the stamp painted nothing — refused a NaN first stamp, and only the binned kernel did what the reference does.

brush_alpha_dev's prepared reciprocal (k_common.h:rdiv): the denominators are the radius, which is >= sqrt(0.001) > 2^-5 (the radius^2 skip) and < 2^24
(only the anti-aliased path divides, and it is taken only while radius + 0.5 > radius), and edge1 - edge0 = -1; the numerators are a distance, 0 or
>= 2^-75 (the square root of the smallest subnormal) and <= radius + 0.5 < 2^24, and dist - edge0 in (-1, 0).  k_common.h argues for denominators in
[2^-48, 2^20] and numerators 0 or in [2^-100, 2^20]; the brush's reach above 2^20 is inside neither, so test_brush_division_range re-checks the brush's own
range against `/` on the device, and the radius family shows the quotient's use in pixels.

Wall time on an MI355X: the whole file 2.6 s together with tests/test_gpu_resample_edges.py; the slowest families are size (324 rows, 0.47 s) and line
(324 rows on both kernels, 0.45 s).
"""
import ctypes as C
import time

import numpy as np
import pytest

from . import brush_cases as BC

pytestmark = pytest.mark.gpu

BBOX, BINNED = 1, 2


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    g = GpuBackend(0)
    g.r._lib.pfx_int_brush_last.argtypes = [C.c_void_p]
    g.r._lib.pfx_int_brush_last.restype = C.c_int
    return g


@pytest.fixture(scope="module")
def oracle():
    from .backends import OracleBackend
    return OracleBackend()


def brush_path(gpu):
    return gpu.r._lib.pfx_int_brush_last(gpu.r._h)


def same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = (got != ref).any(-1)
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} pixels differ, first at x={x} y={y}: device {got[y, x].tolist()} oracle {ref[y, x].tolist()}")


def run_row(gpu, oracle, row):
    ref = BC.run(oracle, row)
    for binning in row.binning:
        gpu.r.tune("brush_binning", binning)
        try:
            got = BC.run(gpu, row)
            path = brush_path(gpu)
        finally:
            gpu.r.tune("brush_binning", 1)
        same(got, ref, f"{row} binning={binning}")
        if row.family == "count":   # a row written for one kernel has to run on it
            n = len(row.points)
            assert path == (BINNED if n > 64 and binning else BBOX), f"{row} binning={binning}: ran path {path}"
    return len(row.binning)


@pytest.mark.parametrize("family", BC.FAMILIES)
def test_brush_edges_vs_oracle(gpu, oracle, family):
    t0 = time.perf_counter()
    rows = BC.rows(family)
    assert rows
    n = sum(run_row(gpu, oracle, row) for row in rows)
    print(f"{family}: {len(rows)} rows, {n} device runs, {time.perf_counter() - t0:.2f} s")


def test_brush_path_getter_tells_the_kernels_apart(gpu):
    """64 stamps: the bounding-box kernel; 65: the binned one, or the bounding-box kernel under brush_binning = 0; a brush below the radius skip and a
    stroke off the right / bottom edge launch nothing"""
    row = next(r for r in BC.rows("count") if r.name == "65-eraser")
    tgt = BC.target(row.target, *row.size)
    brush = gpu.r.make_brush(**row.brush)
    gpu.r.brush_stamps(tgt, brush, row.points[:64])
    assert brush_path(gpu) == BBOX
    gpu.r.brush_stamps(tgt, brush, row.points)
    assert brush_path(gpu) == BINNED
    gpu.r.tune("brush_binning", 0)
    try:
        gpu.r.brush_stamps(tgt, brush, row.points)
        assert brush_path(gpu) == BBOX
    finally:
        gpu.r.tune("brush_binning", 1)
    gpu.r.brush_stamps(tgt, gpu.r.make_brush(**dict(row.brush, size=0.06)), row.points)
    assert brush_path(gpu) == 0
    gpu.r.brush_stamps(tgt, brush, row.points[:3] + np.float32(1000.0))
    assert brush_path(gpu) == 0
    gpu.r.brush_stamps(tgt, brush, row.points[:3] - np.float32(1000.0))   # the reference's casts give a stamp off the left / top edge the box of column / row 0
    assert brush_path(gpu) == BBOX


def test_nan_stamp_is_one_behaviour_in_every_place_and_on_both_kernels(gpu, oracle):
    """the issue's three stamps (50, 50), (NaN, 10), (90, 60) at size 17.5, the NaN in each place, alone and in front of 70 more stamps: always the
    reference's column 0"""
    w, h = 120, 90
    brush = dict(size=17.5, hardness=0.6, anti_aliased=True, color=(0.9, 0.3, 0.1, 0.8), flow=0.85)
    tgt = np.zeros((h, w, 4), np.uint8)
    fin = [(50.0, 50.0), (90.0, 60.0)]
    nan = (float("nan"), 10.0)
    plain = oracle.brush_stamps(tgt, brush, fin)
    for pts in ([nan] + fin, [fin[0], nan, fin[1]], fin + [nan]):
        for tail in (0, 70):
            p = np.concatenate([np.array(pts, np.float32), BC.stroke(tail, w, h, seed=5)]) if tail else np.array(pts, np.float32)
            ref = oracle.brush_stamps(tgt, brush, p)
            if not tail:
                assert (ref[:, 0] != plain[:, 0]).any() and np.array_equal(ref[:, 1:], plain[:, 1:])
            for binning in (1, 0):
                gpu.r.tune("brush_binning", binning)
                try:
                    same(gpu.brush_stamps(tgt, brush, p), ref, f"NaN at {pts.index(nan)} of {len(p)} binning={binning}")
                finally:
                    gpu.r.tune("brush_binning", 1)


def test_brush_division_range(gpu):
    """k_common.h:rdiv against the compiler's IEEE divide over the operands brush_alpha_dev produces (see the module docstring): numerators with
    exponents -75 .. 24, denominators -5 .. 24, 2^28 random pairs"""
    t0 = time.perf_counter()
    bad = gpu.r.selftest_division_range(seed=0xB2054, n_millions=268, num_exp=(-75, 24), den_exp=(-5, 24))
    print(f"division self-test, brush range: {bad} mismatches, {time.perf_counter() - t0:.2f} s")
    assert bad == 0
