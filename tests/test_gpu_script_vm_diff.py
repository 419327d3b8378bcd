"""Differential test of the script VM (k_script.hip: vm_kernel) against the host interpreter (pfx_rhai.cpp: Interp), on the seeded
closure corpus of tests/closure_gen.py.  The host runs the same closure text on the same inputs (tests/closure_ref.py), pixel by
pixel, and the bulk iterators' write-back rule turns its results into the expected image.  Result elements that do not touch
pow / sin / cos / tan / atan2 / exp / ln are held bit-exact; the others may differ by 1 on fewer than 0.1 % of them from the host with
glibc (the contract against the reference), and must equal at tolerance 0 the host run again with the device's libm results substituted for
the calls it traced (tests/vm_libm_probe.py: the libm seam and the device probe).  A failing closure must fail on the device with the host's
message, at the host's line, for the first failing pixel in row-major order."""
import numpy as np
import pytest

from paintfe_amd import PfxError

from . import closure_gen as G
from . import closure_ref as R
from . import vm_libm_probe as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def clip_region(p, w, h, region=None):
    if p.kind != "for_region":
        return 0, 0, w, h
    rx, ry, rw, rh = region if region is not None else p.region
    # scripting.rs:513-516 in u32: a negative far edge wraps to a huge one and is clipped to the image
    x0, y0 = max(rx, 0), max(ry, 0)
    x1, y1 = min((rx + rw) & 0xffffffff, w), min((ry + rh) & 0xffffffff, h)
    if x0 >= x1 or y0 >= y1:
        return 0, 0, 0, 0
    return x0, y0, x1, y1


def device_run(r, src, img, mask):
    try:
        out, _ = r.execute_script_sync(src, img, mask)
        return out, None
    except PfxError as e:
        return None, (e.status, e.line, R.error_text(str(e).split(": ", 1)[1]))


def expected_image(img, pixels, results):
    exp = img.copy()
    for (x, y), res in zip(pixels, results):
        exp[y, x] = R.write_back(img[y, x], res)
    return exp


def compare(p, out, exp, pixels, what):
    """bit-exact on elements without libm, |diff| <= 1 on < 0.1 % of the libm ones"""
    libm = list(p.libm[:4]) + [False] * (4 - len(p.libm[:4]))
    ys = np.array([y for _, y in pixels], dtype=np.int64)
    xs = np.array([x for x, _ in pixels], dtype=np.int64)
    got, want = out[ys, xs].astype(np.int64), exp[ys, xs].astype(np.int64)
    for c in range(4):
        d = np.abs(got[:, c] - want[:, c])
        if not libm[c]:
            bad = np.nonzero(d)[0]
            assert bad.size == 0, (f"{what}: channel {c} differs at {bad.size} pixels, first (x, y) = {pixels[bad[0]]}: "
                                   f"device {got[bad[0]]} host {want[bad[0]]}\n{p.device_script()}")
        else:
            assert d.max(initial=0) <= 1 and np.count_nonzero(d) <= 0.001 * d.size, (what, c, int(d.max()), int(np.count_nonzero(d)))


def compare_substituted(p, out, exp_sub, pixels, what):
    """every element, libm or not, equals the host run with the device's libm: tolerance 0"""
    ys = np.array([y for _, y in pixels], dtype=np.int64)
    xs = np.array([x for x, _ in pixels], dtype=np.int64)
    got, want = out[ys, xs], exp_sub[ys, xs]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} pixels differ from the host with the device's libm, first (x, y) = {pixels[bad[0]]}: "
                           f"device {got[bad[0]]} host {want[bad[0]]}\n{p.device_script()}")


def check_errors(dev_err, host_err, src):
    assert dev_err is not None, f"the host fails with {host_err}, the device does not\n{src}"
    assert dev_err[0] == -6 and host_err[0] == -6, (dev_err, host_err)
    assert dev_err[1] == host_err[1], (dev_err, host_err, src)
    assert R.same_error(dev_err[2], host_err[2]), (dev_err, host_err, src)


SMALL = G.CORPUS_SEEDS


@pytest.mark.parametrize("chunk", range(8))
def test_small_corpus_matches_host(r, chunk):
    seeds = SMALL[chunk::8]
    for seed in seeds:
        p = G.generate(seed)
        w, h = p.width, p.height
        img, mask = R.image(w, h)
        x0, y0, x1, y1 = clip_region(p, w, h)
        (results, host_err), sub, _ = P.substituted(r, lambda: R.host_loop(p, (x0, y0, x1, y1), w, h))
        src = p.device_script()
        out, dev_err = device_run(r, src, img, mask)
        if host_err is not None:
            check_errors(dev_err, host_err, src)
            continue
        assert dev_err is None, f"seed {seed}: the device fails with {dev_err}, the host does not\n{src}"
        pixels = [(x, y) for y in range(y0, y1) for x in range(x0, x1)]
        assert len(results) == len(pixels)
        exp = expected_image(img, pixels, results)
        # pixels outside the region keep their value
        outside = np.ones((h, w), bool)
        outside[y0:y1, x0:x1] = False
        assert np.array_equal(out[outside], img[outside]), f"seed {seed}: pixels outside the region changed"
        compare(p, out, exp, pixels, f"seed {seed}")
        if sub is not None:
            assert sub[1] is None, (seed, sub[1])
            compare_substituted(p, out, expected_image(img, pixels, sub[0]), pixels, f"seed {seed}")


# ---------------------------------------------------------------- launch geometry
FRAMES = {256: [(2048, 1100), (63, 41), (1, 900)], 192: [(1600, 1000), (191, 9)], 128: [(1100, 1000), (65, 33)],
          64: [(1024, 600), (193, 7), (900, 1)]}
GRID = 256 * 32   # blocks of a launch before the grid stride (PFXK_VM_MAX_BLOCKS)


def geometry_programs():
    """one program per (lanes, lcode, heavy) class, chosen through the shape probe, generated for a frame of its class (x / y ranges)"""
    chosen = {}
    for seed in sorted(G.CORPUS_SEEDS, key=lambda s: G.knobs_for(s)["errors"]):   # programs without planted failures first
        k = G.knobs_for(seed)
        if k["kind"] == "for_region":
            continue
        w, h = FRAMES[k["lanes"]][0]
        p = G.generate(seed, {"w": w, "h": h})
        sh = R.closure_shape(p.device_script(), w, h)
        key = (sh["lanes"], sh["lcode"], sh["heavy"])
        if key not in chosen:
            chosen[key] = (p, sh)
    return chosen


def sample_pixels(w, h, lanes, rng):
    n = w * h
    idx = {0, n - 1, w - 1, n - w}
    stride = GRID * lanes
    for k in range(1, n // lanes + 1, max(1, n // lanes // 300)):
        idx |= {k * lanes - 1, k * lanes}
    for j in range(1, n // stride + 1):
        idx |= {j * stride - 1, j * stride, j * stride + lanes - 1}
    for y in range(1, h, max(1, h // 200)):
        idx |= {y * w - 1, y * w}
    idx = {i for i in idx if 0 <= i < n}
    extra = rng.choice(n, size=min(n, max(0, 3000 - len(idx))), replace=False) if n > len(idx) else []
    idx |= {int(i) for i in extra}
    return [(i % w, i // w) for i in sorted(idx)]


def test_geometry_classes_against_host(r, record_property):
    chosen = geometry_programs()
    table = sorted(chosen)
    record_property("vm_launch_classes", str(table))
    print("VM launch classes run:", table)
    assert len(chosen) == 16, sorted(set((l, c, hv) for l in (256, 192, 128, 64) for c in (0, 1) for hv in (0, 1)) - set(chosen))
    rng = np.random.default_rng(5)
    for key, (p, sh) in sorted(chosen.items()):
        lanes = sh["lanes"]
        for (w, h) in FRAMES[lanes]:
            q = p if (w, h) == FRAMES[lanes][0] else G.generate(p.seed, {"w": w, "h": h})
            img, mask = R.image(w, h)
            out, dev_err = device_run(r, q.device_script(), img, mask)
            pixels = sample_pixels(w, h, lanes, rng)
            (results, host_err), sub, _ = P.substituted(r, lambda: R.host_run(q, pixels, w, h))
            if host_err is not None:
                # the host stops at the first failing pixel of the sample; the device reports the first of the frame: same kind, not before it
                assert dev_err is not None and dev_err[0] == -6, (key, (w, h), host_err, dev_err)
                continue
            assert dev_err is None, (key, (w, h), dev_err)
            compare(q, out, expected_image(img, pixels, results), pixels, f"class {key} frame {w}x{h} seed {q.seed}")
            if sub is not None:
                assert sub[1] is None, (key, (w, h), sub[1])
                compare_substituted(q, out, expected_image(img, pixels, sub[0]), pixels, f"class {key} frame {w}x{h} seed {q.seed}")


def test_whole_frame_equals_four_region_bands(r):
    """a closure that reads no other pixel gives the same image over the whole frame and as four for_region bands (grid stride vs region offsets)"""
    for seed in G.CORPUS_SEEDS:
        k = G.knobs_for(seed)
        if k["kind"] != "for_each_pixel" or k["errors"] or k["lanes"] != 256:
            continue
        w, h = 2048, 1100
        p = G.generate(seed, {"w": w, "h": h})
        text = "\n".join(p.body)
        if "get_" in text or p.fn_name:
            continue
        img, mask = R.image(w, h)
        whole, err = device_run(r, p.device_script(), img, mask)
        assert err is None
        bands = [(0, 0, 300), (0, 300, 1), (0, 301, 498), (0, 799, 301)]
        src = "\n".join(p.header + [f"for_region({x}, {y}, {w}, {bh}, {text});" for x, y, bh in bands])
        banded, err = device_run(r, src, img, mask)
        assert err is None
        assert np.array_equal(whole, banded)
        return
    pytest.fail("no for_each_pixel program without pixel reads in the corpus")


# ---------------------------------------------------------------- first failing pixel
@pytest.mark.parametrize("lanes_regs", [(256, 0), (64, 22)])
@pytest.mark.parametrize("offset", [(0, 0), (5, 3)])
def test_first_failing_pixel_in_row_major_order(r, lanes_regs, offset):
    """two failing pixels: the earlier one (row-major) runs in the last block of the first grid pass, the later one in block 0 of the second
    pass, so it is likely to fail first in time; its error is on an earlier line.  The reported error must be the row-major first one's."""
    lanes, n_pad = lanes_regs
    ox, oy = offset
    w, h = (2048, 1100) if lanes == 256 else (1024, 600)
    rw, rh = w - ox, h - oy
    stride = GRID * lanes
    first = (GRID - 1) * lanes + 3           # last block, first pass
    later = stride + 3                       # block 0, second pass
    assert later > first and later < rw * rh
    fx, fy = ox + first % rw, oy + first // rw
    lx, ly = ox + later % rw, oy + later // rw
    pads = "".join(f"    let p{j} = r ^ {j + 3};\n" for j in range(n_pad))
    use = " ^ ".join(f"p{j}" for j in range(n_pad)) or "0"
    src = ("for_region(%d, %d, %d, %d, |x, y, r, g, b, a| {\n" % (ox, oy, rw, rh) + pads +
           f"    if x == {lx} && y == {ly} {{ let e = -((-9223372036854775807 - 1) + (r - r)); }}\n"
           f"    if x == {fx} && y == {fy} {{ let e = 1000 / (g - g); }}\n"
           f"    [r, g ^ ({use} & 0), b, a]\n}});")
    later_line, first_line = 2 + n_pad, 3 + n_pad
    img, mask = R.image(w, h)
    sh = R.closure_shape(src, w, h)
    assert sh["lanes"] == lanes
    out, err = device_run(r, src, img, mask)
    assert out is None and err is not None
    assert err[0] == -6 and err[1] == first_line and err[2] == "Division by zero", (err, later_line)


# ---------------------------------------------------------------- disagreements the differential run pins
@pytest.mark.parametrize("expr,msg", [("(-9223372036854775807 - 1) % (r - 2)", "Modulo division overflow"),   # was 'Division overflow'
                                      ("clamp(g, b, r)", "clamp: min > max")])                                 # was a silent clamp
def test_vm_error_texts_match_host(r, expr, msg):
    src = f"map_channels(|r, g, b, a| {{\n    let v = {expr};\n    [v, g, b, a]\n}});"
    img = np.zeros((3, 5, 4), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 9, 0, 3
    img[1, 2, 0:3] = (1, 7, 2)        # r - 2 == -1; clamp bounds 2 > 1
    out, dev_err = device_run(r, src, img, None)
    assert out is None and dev_err == (-6, 2, msg)
    host = R.check_console(f"let f = |r, g, b, a| {{\n    let v = {expr};\n    [v, g, b, a]\n}};\nprint(f.call(1, 7, 2, 0));")[1]
    assert host[1] == 2 and R.same_error(msg, host[2]), host


# ---------------------------------------------------------------- negative control of the exact comparison
NUDGES = [1 << j for j in range(0, 53, 2)]
NUDGE_DETECTED = 1 << 42     # measured: the smallest nudge the corpus detects


def test_nudged_libm_table_is_detected(r, record_property):
    """the substituted comparison is not vacuous: the device's libm results nudged by k ulps make the corpus differ from the device.  The smallest
    k (of 1, 4, 16, ..) that some corpus program detects is recorded"""
    runs = []
    for seed in SMALL:
        p = G.generate(seed)
        if not any(p.libm[:4]):
            continue
        w, h = p.width, p.height
        img, mask = R.image(w, h)
        x0, y0, x1, y1 = clip_region(p, w, h)
        run = (lambda p=p, reg=(x0, y0, x1, y1), w=w, h=h: R.host_loop(p, reg, w, h))
        (results, host_err), sub, table = P.substituted(r, run)
        if host_err is not None or sub is None:
            continue
        out, dev_err = device_run(r, p.device_script(), img, mask)
        assert dev_err is None
        pixels = [(x, y) for y in range(y0, y1) for x in range(x0, x1)]
        runs.append((p, img, pixels, out, run, table))
        if len(runs) == 24:
            break
    assert runs, "no corpus program with libm-dependent channels"
    detected = None
    for k in NUDGES:
        for p, img, pixels, out, run, table in runs:
            with P.traced(P.nudge(table, k)):
                res, err = run()
            if err is not None or not np.array_equal(expected_image(img, pixels, res)[tuple(np.array(pixels).T[::-1])],
                                                     out[tuple(np.array(pixels).T[::-1])]):
                detected = k
                break
        if detected is not None:
            break
    record_property("smallest_detected_nudge_ulps", detected)
    print(f"smallest nudge detected over {len(runs)} corpus programs: {detected} ulps")
    assert detected is not None and detected <= NUDGE_DETECTED
