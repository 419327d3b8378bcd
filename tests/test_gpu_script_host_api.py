"""The script host API (pfx_script_host.cpp: ScriptHost::call) on the device against the stateful model of tests/script_model.py: the hand-written edge table
of tests/script_cases.py on every size, and the seeded corpus of statement sequences in seed order — image shape and bytes, console lines and canvas-op list
at tolerance 0.  One renderer serves the whole module, so whatever a script leaves behind (the ping-pong buffers, the mask, a failed run) is there for the
next.  tests/test_script_model_host.py holds the model to the reference and proves what the corpus reaches.

The direct entry points pfx_flip_rotate[_dev] and pfx_resize_canvas[_dev] launch the same permute and recanvas kernels: compared with the oracle on every size."""
import ctypes as C

import numpy as np
import pytest

from . import oracle_lib as O
from . import script_cases as SC
from . import script_model as M
from .dev_buffers import Dev

pytestmark = pytest.mark.gpu
CHUNK = 40


@pytest.fixture(scope="module")
def r():
    from paintfe_amd import GpuRenderer
    r = GpuRenderer(0)
    r.set_exact(True)   # apply_blur / apply_sharpen / apply_glow: the bit-exact Gaussian
    try:
        yield r
    finally:
        r.set_exact(False)


@pytest.fixture(autouse=True)
def stop_after_a_device_error(r):
    """a HIP error behind a test ends the session: nothing more is launched on a device that has reported one"""
    yield
    from paintfe_amd import PfxError
    try:
        r.synchronize()
    except PfxError as e:
        pytest.exit(f"the device reported an error after this test: {e}", returncode=3)


def first_difference(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape[1]}x{got.shape[0]}, the model has {want.shape[1]}x{want.shape[0]}"
    bad = np.argwhere((got != want).any(-1))
    if not len(bad):
        return None
    y, x = (int(v) for v in bad[0])
    return f"{len(bad)} pixels differ, the first at ({x}, {y}): {got[y, x].tolist()}, the model has {want[y, x].tolist()}"


def run_program(r, prog):
    """one program on the device and in the model; the text of the first mismatch, or None"""
    from paintfe_amd import PfxError
    img, mask = prog.inputs()
    src = SC.script(prog.statements)
    line = SC.fails_at(prog.statements)
    where = f"{prog.name} ({prog.size[0]}x{prog.size[1]}, image seed {prog.image_seed}, {'caller mask' if mask is not None else 'no mask'})\n{src}\n"
    if line is not None:
        try:
            r.execute_script_sync(src, img, mask, with_ops=True)
        except PfxError as e:
            if e.status == -6 and e.line == line:
                return None
            return f"{where}raised status {e.status} on line {e.line}; line {line} fails"
        return f"{where}did not raise; line {line} fails"
    want = M.Model(img, mask).run(prog.statements)
    out, console, ops = r.execute_script_sync(src, img, mask, with_ops=True)
    d = first_difference(out, want.pixels)
    if d:
        return where + d
    if console != want.console:
        k = next((k for k, (a, b) in enumerate(zip(console, want.console)) if a != b), min(len(console), len(want.console)))
        return f"{where}console line {k}: {console[k:k + 1]}, the model has {want.console[k:k + 1]} ({len(console)} and {len(want.console)} lines)"
    if ops != want.ops:
        return f"{where}canvas ops {ops}, the model has {want.ops}"
    return None


def run_all(r, progs):
    for p in progs:
        problem = run_program(r, p)
        assert problem is None, problem


@pytest.mark.parametrize("size", SC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_table(r, size):
    run_all(r, [p for p in SC.edge_programs() if p.size == size])


@pytest.mark.parametrize("first", range(SC.SEEDS.start, SC.SEEDS.stop, CHUNK))
def test_corpus(r, first):
    """in seed order: a failing program raises PfxError -6 with the line of its failing statement, and the program after it still matches the model"""
    run_all(r, [SC.program(s) for s in range(first, min(first + CHUNK, SC.SEEDS.stop))])


# ------------------------------------------------------------------ the direct entry points
def targets(w, h):
    return [(w + 4, h + 6), (w + 3, h + 5), (max(w - 2, 1), max(h - 4, 1)), (max(w - 3, 1), max(h - 1, 1)), (w + 3, max(h - 3, 1)), (max(w - 3, 1), h + 3)]


FILL = (9, 200, 31, 77)
ANCHORS = [(ax, ay) for ay in range(3) for ax in range(3)]


@pytest.mark.parametrize("size", SC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_direct_entry_points_equal_the_oracle(r, size):
    w, h = size
    img = SC.image(w, h, 11)
    for op in O.CANVAS_OPS:
        d = first_difference(r.flip_rotate(img, op), O.flip_rotate(img, op))
        assert d is None, f"flip_rotate {op} {w}x{h}: {d}"
    for nw, nh in targets(w, h):
        for anchor in ANCHORS:
            d = first_difference(r.resize_canvas(img, nw, nh, anchor, FILL), O.resize_canvas(img, nw, nh, anchor, FILL))
            assert d is None, f"resize_canvas {w}x{h} -> {nw}x{nh} anchor {anchor}: {d}"


@pytest.mark.parametrize("size", SC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_direct_entry_points_on_device_buffers(r, size):
    """the _dev tier: source and destination between guard bytes, which stay intact"""
    w, h = size
    img = SC.image(w, h, 12)
    lib, ctx = r._lib, r._h
    with Dev(r) as dev:
        src = dev.put(img)
        for op, k in O.CANVAS_OPS.items():
            want = O.flip_rotate(img, op)
            dst = dev.sentinel(want.shape)
            r._check(lib.pfx_flip_rotate_dev(ctx, C.c_void_p(src), C.c_uint32(w), C.c_uint32(h), C.c_void_p(dst), C.c_int(k)))
            d = first_difference(dev.get(dst, want.shape), want)
            assert d is None, f"flip_rotate_dev {op} {w}x{h}: {d}"
        fill = (C.c_uint8 * 4)(*FILL)
        for nw, nh in targets(w, h):
            for ax, ay in ANCHORS:
                want = O.resize_canvas(img, nw, nh, (ax, ay), FILL)
                dst = dev.sentinel(want.shape)
                r._check(lib.pfx_resize_canvas_dev(ctx, C.c_void_p(src), C.c_uint32(w), C.c_uint32(h), C.c_void_p(dst), C.c_uint32(nw), C.c_uint32(nh), C.c_uint32(ax),
                                                   C.c_uint32(ay), fill))
                d = first_difference(dev.get(dst, want.shape), want)
                assert d is None, f"resize_canvas_dev {w}x{h} -> {nw}x{nh} anchor ({ax}, {ay}): {d}"
        assert np.array_equal(dev.get(src, img.shape), img)
