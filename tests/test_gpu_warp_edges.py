"""Parity (GPU): the warp kernels (k_warp.hip) at their edges — the tables of tests/warp_cases.py through the device-resident entry points, against the CPU
oracle.  What the tables reach is shown on the host by tests/test_warp_cases_host.py; every size follows the kernels' compile-time shape (warp_info).

Bar: tolerance 0, the bar the warp tests of test_gpu_parity.py hold.  Pixels with np.array_equal; fields as uint32 bits, except that where the oracle has a
NaN the device must have a NaN (sign and payload are not compared: x86 and the GPU make different default NaNs).  Every launch form a case names is read back
from the context (warp_last) and asserted: XCD tile order exactly from MESH_XCD_MIN_ROWS tile rows with pfx_tune "mesh_xcd" on, control points in LDS exactly up
to MESH_LDS_PTS, PAIR exactly from a width of 2, BUF32 as pfx_tune "warp_buf32" says (0 runs the 64-bit-address instantiations, which otherwise need a source of
4 GiB), the dab launch plain or over the chunk list.  Every destination and field lies between guard bytes (dev_buffers.Dev), every source is read back.

Wall time on an MI355X: the whole file 2.4 s (24 tests); the slowest are the mesh rows at 257 x 1105 (15 rows, 0.65 s) and at 300 x 1009 (15 rows, 0.60 s), then
the displacement fields at 300 x 1009 (0.06 s).
"""
import time

import numpy as np
import pytest

from . import oracle_lib as O
from . import warp_cases as WC
from .dev_buffers import SENTINEL, Dev

pytestmark = pytest.mark.gpu
f32 = np.float32
KNOBS = [(1, 1), (0, 1), (1, 0), (0, 0)]      # pfx_tune mesh_xcd, warp_buf32


@pytest.fixture(scope="module")
def gpu():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


@pytest.fixture(autouse=True)
def stop_after_a_device_error(gpu):
    """a HIP error behind a test ends the session: nothing more is launched on a device that has reported one"""
    yield
    from paintfe_amd import PfxError
    try:
        gpu.synchronize()
    except PfxError as e:
        pytest.exit(f"the device reported an error after this test: {e}", returncode=3)


class knobs:
    """pfx_tune mesh_xcd / warp_buf32 for a block, back to the defaults afterwards"""
    def __init__(self, gpu, xcd=1, buf32=1):
        self.gpu, self.v = gpu, (xcd, buf32)

    def __enter__(self):
        self.gpu.tune("mesh_xcd", self.v[0])
        self.gpu.tune("warp_buf32", self.v[1])

    def __exit__(self, *exc):
        self.gpu.tune("mesh_xcd", 1)
        self.gpu.tune("warp_buf32", 1)


def get_field(d, ptr, w, h):
    return d.get(ptr, (h * w * 8,)).view(f32).reshape(h, w, 2)


def put_field_sentinel(d, w, h):
    return d.sentinel((h * w * 8,))


def oracle_mesh(row):
    (w, h), (cols, rows) = row.size, row.grid
    orig, deformed = WC.mesh_points(row)
    field = O.mesh_displacement_fast(deformed, cols, rows, w, h) if orig is None else O.mesh_displacement(orig, deformed, cols, rows, w, h)
    return orig, deformed, field, O.warp_displacement(WC.source(w, h), field)


def differing(got, want):
    bad = (got != want).any(-1)
    return f"{int(bad.sum())} pixels differ, first at (y, x) = {tuple(np.argwhere(bad)[0]) if bad.any() else None}"


def test_warp_info_and_the_hooks_before_any_launch():
    from paintfe_amd import GpuRenderer
    fresh = GpuRenderer(0)
    try:
        assert [fresh.warp_last(k) for k in range(5)] == [-1] * 5 and fresh.warp_last(5) == -1
        c = WC.consts()
        assert tuple(fresh.warp_info(k) for k in range(6)) == tuple(c) and fresh.warp_info(6) == -1
    finally:
        fresh.close()


# ---- the fused mesh warp and the mesh field ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", WC.sizes(), ids=str)
def test_mesh_rows_on_every_launch_form(gpu, size):
    """every row of the size: the fused warp under both tile orders and both address forms, and the field alone, all equal to the oracle"""
    t0 = time.perf_counter()
    w, h = size
    src = WC.source(w, h)
    rows = [r for r in WC.mesh_rows() if r.size == size]
    assert rows
    for row in rows:
        cols, nrows = row.grid
        orig, deformed, field, want = oracle_mesh(row)
        with Dev(gpu) as d:
            p_src = d.put(src)
            for xcd, buf32 in KNOBS:
                p_dst = d.sentinel((h, w, 4))
                with knobs(gpu, xcd, buf32):
                    gpu.warp_mesh_catmull_rom_dev(p_src, orig, deformed, cols, nrows, w, h, p_dst)
                what = f"{row} mesh_xcd={xcd} warp_buf32={buf32}"
                assert gpu.warp_last(0) == WC.mesh_flags(row, xcd, buf32), what
                assert (gpu.warp_last(1), gpu.warp_last(2)) == WC.tile_grid(w, h), what
                got = d.get(p_dst, (h, w, 4))
                assert np.array_equal(got, want), f"{what}: {differing(got, want)}"
            p_f = put_field_sentinel(d, w, h)
            gpu.mesh_displacement_dev(orig, deformed, cols, nrows, w, h, p_f)
            assert gpu.warp_last(0) == (WC.IN_LDS if WC.n_points(row.grid) <= WC.consts().lds_pts else 0), row
            assert WC.same_field(get_field(d, p_f, w, h), field), f"{row}: field"
            assert np.array_equal(d.get(p_src, src.shape), src)
    print(f"mesh {size}: {len(rows)} rows, {time.perf_counter() - t0:.2f} s")


def test_mesh_and_displacement_bands_in_both_tile_orders(gpu):
    """rows [first, first + n) of an h_full-row result: the band equals those rows of the whole-image launch and of the oracle; the first three bands are tall
    enough for the XCD order, so band + XCD order is compared with something"""
    t0 = time.perf_counter()
    w, h_full, bands = WC.band_cases()
    src = WC.source(w, h_full)
    for proto in WC.BAND_MESHES:
        row = proto._replace(size=(w, h_full))
        cols, nrows = row.grid
        orig, deformed, field, want = oracle_mesh(row)
        with Dev(gpu) as d:
            p_src, p_whole = d.put(src), d.sentinel((h_full, w, 4))
            gpu.warp_mesh_catmull_rom_dev(p_src, orig, deformed, cols, nrows, w, h_full, p_whole)
            whole = d.get(p_whole, (h_full, w, 4))
            assert np.array_equal(whole, want), f"{row}: {differing(whole, want)}"
            for k, (first, n) in enumerate(bands):
                for xcd in (1, 0):
                    p_band = d.sentinel((n, w, 4))
                    with knobs(gpu, xcd, 1):
                        gpu.warp_mesh_catmull_rom_band_dev(p_src, orig, deformed, cols, nrows, w, h_full, p_band, first, n)
                    what = f"{row} band {first}+{n} mesh_xcd={xcd}"
                    assert bool(gpu.warp_last(0) & WC.XCD) == (xcd == 1 and k < 3) == bool(xcd and WC.takes_xcd_order(n)), what
                    assert (gpu.warp_last(1), gpu.warp_last(2)) == WC.tile_grid(w, n), what
                    got = d.get(p_band, (n, w, 4))
                    assert np.array_equal(got, want[first:first + n]), f"{what}: {differing(got, want[first:first + n])}"
                    assert np.array_equal(got, whole[first:first + n]), what
            assert np.array_equal(d.get(p_src, src.shape), src)
    for kind in ("random", "border_wave_y", "nonfinite"):
        img, disp = WC.field_case(kind, (w, h_full))
        want = O.warp_displacement(img, disp)
        with Dev(gpu) as d:
            p_src = d.put(img)
            for first, n in bands:
                p_disp, p_band = d.put(disp[first:first + n]), d.sentinel((n, w, 4))
                gpu.warp_displacement_band_dev(p_src, img.shape[1], img.shape[0], p_disp, w, n, p_band, first)
                assert gpu.warp_last(0) == WC.displacement_flags(img.shape[1], 1)
                got = d.get(p_band, (n, w, 4))
                assert np.array_equal(got, want[first:first + n]), f"displacement {kind} band {first}+{n}: {differing(got, want[first:first + n])}"
                assert np.array_equal(d.get(p_disp, (n, w, 2 * 4)).view(f32).view(np.uint32), disp[first:first + n].view(np.uint32))
    print(f"bands: {time.perf_counter() - t0:.2f} s")


# ---- the displacement warp -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", WC.sizes(), ids=str)
def test_displacement_fields_on_both_address_forms(gpu, size):
    t0 = time.perf_counter()
    w, h = size
    yr = WC.consts().warp_yr
    for kind in WC.FIELD_KINDS:
        img, disp = WC.field_case(kind, size)
        sh, sw = img.shape[:2]
        want = O.warp_displacement(img, disp)
        with Dev(gpu) as d:
            p_src, p_disp = d.put(img), d.put(disp)
            for buf32 in (1, 0):
                p_dst = d.sentinel((h, w, 4))
                with knobs(gpu, 1, buf32):
                    gpu.warp_displacement_dev(p_src, sw, sh, p_disp, w, h, p_dst)
                what = f"{kind} {size} source {sw}x{sh} warp_buf32={buf32}"
                assert gpu.warp_last(0) == WC.displacement_flags(sw, buf32), what
                assert (gpu.warp_last(1), gpu.warp_last(2)) == (-(-w // 64), -(-h // (4 * yr))), what
                got = d.get(p_dst, (h, w, 4))
                assert np.array_equal(got, want), f"{what}: {differing(got, want)}"
            assert np.array_equal(d.get(p_src, img.shape), img)
            assert np.array_equal(d.get(p_disp, (h, w, 8)).view(np.uint32), disp.view(np.uint32))
    print(f"displacement {size}: {time.perf_counter() - t0:.2f} s")


# ---- dabs ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def run_dabs(gpu, d, start, calls):
    h, w = start.shape[:2]
    p = d.put(start)
    for dabs in calls:
        gpu.displacement_brushes_dev(p, w, h, dabs)
    return get_field(d, p, w, h)


@pytest.mark.parametrize("which", range(6), ids=lambda k: WC.dab_lists()[k].name.replace(" ", "_"))
def test_dab_lists_in_one_call_and_split_at_the_cull_width(gpu, which):
    """a lane walks the dabs its wave can see 64 at a time and must keep the order of the `+=` across the groups: one call and two calls (split at the cull
    width) both equal the oracle applied dab by dab; what no dab reaches keeps its bits, -0.0 included"""
    t0 = time.perf_counter()
    L = WC.dab_lists()[which]
    (w, h), n0 = L.size, WC.consts().dab_cull
    start = WC.start_field(w, h)
    want = WC.apply_dabs(start.copy(), L.dabs)
    with Dev(gpu) as d:
        got = run_dabs(gpu, d, start, [L.dabs])
        assert gpu.warp_last(3) == L.launch and (gpu.warp_last(4) > 0) == (L.launch == WC.DAB_CHUNKED), L.name
        assert WC.same_field(got, want), f"{L.name}: one call, {int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())} entries differ"
        untouched = want.view(np.uint32) == start.view(np.uint32)
        assert np.array_equal(got.view(np.uint32)[untouched], start.view(np.uint32)[untouched])
        split = run_dabs(gpu, d, start, [L.dabs[:n0], L.dabs[n0:]])
        assert WC.same_field(split, want), f"{L.name}: split at {n0}"
    print(f"dabs {L.name}: {time.perf_counter() - t0:.2f} s")


def test_single_dab_edge_table_on_the_device_and_the_host_form(gpu):
    t0 = time.perf_counter()
    w, h = WC.EDGE_SIZE
    start = WC.start_field(w, h)
    with Dev(gpu) as d:
        for name in WC.EDGE_DABS:
            for mode in range(5):
                dab = WC.edge_dab(name, mode)
                want = WC.apply_dabs(start.copy(), [dab])
                got = run_dabs(gpu, d, start, [[dab]])
                assert gpu.warp_last(3) == (WC.DAB_PLAIN if WC.reaches_canvas([dab], w, h) else WC.DAB_NONE), (name, mode)
                assert WC.same_field(got, want), f"{name} mode {mode}: device"
                assert WC.same_field(gpu.displacement_brush(start.copy(), *dab), want), f"{name} mode {mode}: host form"
    print(f"single dabs: {time.perf_counter() - t0:.2f} s")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_destination_at_the_sentinel(gpu):
    from paintfe_amd import PfxError
    w, h = WC.small_size()
    src = WC.source(w, h)
    with Dev(gpu) as d:
        p_src, p_dst, p_f = d.put(src), d.sentinel((h, w, 4)), put_field_sentinel(d, w, h)
        for cols, rows in ((0, 3), (3, 0), (WC.MAX_CELLS + 1, 1), (1, WC.MAX_CELLS + 1)):
            pts = np.zeros(((cols + 1) * (rows + 1), 2), f32)
            with pytest.raises(PfxError):
                gpu.warp_mesh_catmull_rom_dev(p_src, pts, pts, cols, rows, w, h, p_dst)
            with pytest.raises(PfxError):
                gpu.mesh_displacement_dev(None, pts, cols, rows, w, h, p_f)
        row = WC.MeshRow((w, h), (6, 6), "nonuniform", "jitter")
        orig, deformed = WC.mesh_points(row)
        for first, n in ((h, 1), (h - 1, 2), (0, h + 1), (0, 0), (2 ** 32 - 1, 2)):
            with pytest.raises(PfxError):
                gpu.warp_mesh_catmull_rom_band_dev(p_src, orig, deformed, 6, 6, w, h, p_dst, first, n)
        with pytest.raises(PfxError):
            gpu.displacement_brushes_dev(p_f, w, h, [(0, 20.0, 20.0, 1.0, 1.0, 9.0, 0.5), (5, 20.0, 20.0, 1.0, 1.0, 9.0, 0.5)])
        with pytest.raises(PfxError):
            gpu.displacement_brushes_dev(p_f, w, h, [(-1, 20.0, 20.0, 1.0, 1.0, 9.0, 0.5)])
        assert (d.get(p_dst, (h, w, 4)) == SENTINEL).all() and (d.get(p_f, (h * w * 8,)) == SENTINEL).all()
        assert np.array_equal(d.get(p_src, src.shape), src)
