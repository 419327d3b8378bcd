"""Parity (GPU): the pointwise adjustment bank (k_pointwise.hip, k_pointwise.h) at its edges, bit for bit against the CPU oracle.
  - every one of the 2^24 colours through every op, at parameter sets chosen for a branch or a rounding tie (the per-pixel functions are branch-free
    rewrites of branchy reference code: each is right or wrong per colour, not per image) — through pointwise_kernel and through pointwise_chain_kernel;
  - every path of pointwise_kernel (the straight-line interior branch, the 16-byte general path, the pixel-by-pixel one) under all three sparse modes and
    with and without a selection, staged and on device buffers, out of place and in place, on images that hold a chunk to skip and a chunk to drop;
  - parameters at and beyond the ends of their domains and non-finite ones, which the host folds before the kernel sees them (pfx_api.cpp: prepare_adjust).
The inputs and tables are tests/pointwise_cases.py; tests/test_pointwise_cases_host.py holds them to the conditions that give them their teeth.
References: src/ops/adjustments.rs:21-631, 944-1012, 1240-1441; src/ops/scripting.rs:869-1075."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from . import oracle_lib as O
from . import pointwise_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    return GpuBackend(0)


@pytest.fixture(scope="module")
def oracle():
    from .backends import OracleBackend
    return OracleBackend()


@pytest.fixture(scope="module")
def cube():
    img = PC.colour_cube()
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def cube_dev(gpu, cube):
    """the cube on the device and a second image of its size: (src, dst)"""
    r = gpu.r
    a, b = r.dev_alloc(cube.nbytes), r.dev_alloc(cube.nbytes)
    r.dev_upload(a, cube)
    yield a, b
    r.dev_free(a)
    r.dev_free(b)


@pytest.fixture(scope="module")
def lattice():
    img = PC.lattice()
    img.setflags(write=False)
    return img


def show(v):
    return "(" + ", ".join(repr(float(x)) for x in v) + ")"


def oracle_run(img, op_id, params, lut=None, mask=None, sparse=PC.DENSE):
    kind, op = PC.split_id(op_id)
    if kind == "adjust":
        return O.adjust(img, op, params, lut=lut, mask=mask, sparse=sparse)
    p = PC.oracle_rhai_params(op, params)
    if img.shape[0] < 1024:
        return O.rhai_adjust(img, op, p)
    # the Rhai closure is one serial loop over pixels and every pixel is on its own: bands of rows on a few threads give the same bytes sooner
    out = np.ascontiguousarray(img).copy()
    arr = np.asarray(list(p) + [0.0] * (8 - len(p)), np.float32)
    bands = np.array_split(np.arange(out.shape[0]), 16)

    def band(rows):
        part = out[rows[0]:rows[-1] + 1]
        O.lib().pfxo_rhai_adjust(part.ctypes.data_as(C.c_void_p), C.c_size_t(part.size // 4), C.c_int(O.RHAI[op]), arr.ctypes.data_as(C.c_void_p))

    with ThreadPoolExecutor(8) as pool:
        list(pool.map(band, bands))
    return out


def gpu_run(gpu, img, op_id, params, lut=None, mask=None, sparse=PC.DENSE):
    kind, op = PC.split_id(op_id)
    return gpu.adjust(img, op, params, lut=lut, mask=mask, sparse=sparse) if kind == "adjust" else gpu.rhai_adjust(img, op, params)


def chain_op(op_id, params, lut):
    kind, op = PC.split_id(op_id)
    return (kind, op, params, None if lut is None else np.ascontiguousarray(lut).reshape(-1))


def difference(got, want, src):
    """None when equal, else: how many pixels differ and the first of them with its source colour"""
    if np.array_equal(got, want):
        return None
    bad = (got != want).any(axis=-1)
    y, x = (int(v[0]) for v in np.nonzero(bad))
    return (f"{int(bad.sum())} of {bad.size} px differ; first at x={x} y={y}: source rgba {tuple(int(c) for c in src[y, x])} -> "
            f"device {tuple(int(c) for c in got[y, x])}, oracle {tuple(int(c) for c in want[y, x])}")


# ------------------------------------------------------------------ 1, 2: every colour
@pytest.mark.parametrize("op_id", PC.OP_IDS)
def test_every_colour(gpu, cube, op_id):
    """all 2^24 colours (tests/pointwise_cases.py: colour_cube, alpha of every value) at every parameter set of the op, dense, tolerance 0"""
    for k, (params, lut) in enumerate(PC.every_colour_sets(op_id)):
        d = difference(gpu_run(gpu, cube, op_id, params, lut), oracle_run(cube, op_id, params, lut), cube)
        assert d is None, f"{op_id} set {k} {show(params)}: {d}"


@pytest.mark.parametrize("op_id", PC.OP_IDS)
def test_every_colour_through_the_chain(gpu, cube, cube_dev, op_id):
    """the op's first parameter set as a chain of one op on the cube: pointwise_chain_kernel's instantiation of the same per-pixel functions"""
    params, lut = PC.every_colour_sets(op_id)[0]
    a, b = cube_dev
    gpu.r.chain_dev(a, b, 4096, 4096, [chain_op(op_id, params, lut)])
    gpu.r.synchronize()
    d = difference(gpu.r.dev_download(b, cube.shape), oracle_run(cube, op_id, params, lut), cube)
    assert d is None, f"{op_id} {show(params)} as a chain: {d}"


# ------------------------------------------------------------------ 3: every path of pointwise_kernel
PATH_OPS = [("hsl", [47.0, 35.0, -12.0], None), ("invert_alpha", [], None), ("lut_rgba", [], PC.alpha_to_zero_luts()), ("sepia", [], None),
            ("threshold", [127.5], None)]
PATH_RHAI = [("rhai_hsl", [47.0, 35.0, -12.0]), ("rhai_levels", [20.0, 230.0, 0.8])]


@pytest.mark.parametrize("shape", PC.PATH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_paths(gpu, shape):
    """five ops x three sparse modes x four selections on an image with a chunk to skip, a chunk to drop and a chunk kept alive by its last pixel: through the
    staged entry and on device buffers, out of place (into an image prefilled with 0xA5: a chunk the block remap leaves out shows) and in place"""
    w, h = shape
    r = gpu.r
    fill = np.full((h, w, 4), 0xA5, np.uint8)
    a, b, m = r.dev_alloc(w * h * 4), r.dev_alloc(w * h * 4), r.dev_alloc(w * h)
    try:
        for seed in PC.path_seeds(shape):
            img = PC.path_image(w, h, seed)
            for mi, mask in enumerate(PC.path_masks(w, h, seed)):
                if mask is not None:
                    r.dev_upload(m, mask)
                mp = 0 if mask is None else m
                for op, params, lut in PATH_OPS:
                    for sparse in (PC.DENSE, PC.FROM_FLAT, PC.IN_PLACE):
                        what = f"{op} {w}x{h} seed {seed} sparse {sparse} mask {mi}"
                        want = O.adjust(img, op, params, lut=lut, mask=mask, sparse=sparse)
                        d = difference(gpu.adjust(img, op, params, lut=lut, mask=mask, sparse=sparse), want, img)
                        assert d is None, f"{what}, staged: {d}"
                        r.dev_upload(a, img)
                        r.dev_upload(b, fill)
                        r.adjust_dev(a, b, w, h, op, params, lut=lut, mask_ptr=mp, sparse=sparse)
                        r.synchronize()
                        d = difference(r.dev_download(b, img.shape), want, img)
                        assert d is None, f"{what}, device buffers: {d}"
                        assert np.array_equal(r.dev_download(a, img.shape), img), f"{what}: the source changed"
                        r.adjust_dev(a, a, w, h, op, params, lut=lut, mask_ptr=mp, sparse=sparse)
                        r.synchronize()
                        d = difference(r.dev_download(a, img.shape), want, img)
                        assert d is None, f"{what}, in place: {d}"
            for op_id, params in PATH_RHAI:
                want = oracle_run(img, op_id, params)
                d = difference(gpu_run(gpu, img, op_id, params), want, img)
                assert d is None, f"{op_id} {w}x{h} seed {seed}, staged: {d}"
                r.dev_upload(a, img)
                gpu.rhai_adjust_dev(a, w, h, PC.split_id(op_id)[1], params)
                r.synchronize()
                d = difference(r.dev_download(a, img.shape), want, img)
                assert d is None, f"{op_id} {w}x{h} seed {seed}, device buffer: {d}"
    finally:
        for p in (a, b, m):
            r.dev_free(p)


# ------------------------------------------------------------------ 4: parameter edges
@pytest.mark.parametrize("op_id", sorted(PC.EDGE_PARAMS))
def test_parameter_edges(gpu, lattice, op_id):
    """+-0, NaN, +-inf, +-3e36, +-1e38 in every parameter and the ends of each op's own domain, on the lattice (interior path), dense.  HSL and vibrance pick
    their round-and-pack by whether the host found the folded parameters finite (apply_px: p[11]): their sets also run with FROM_FLAT and as one-op chains."""
    h, w = lattice.shape[:2]
    two_packs = op_id in ("hsl", "vibrance")
    if two_packs:
        a, b = gpu.r.dev_alloc(lattice.nbytes), gpu.r.dev_alloc(lattice.nbytes)
        gpu.r.dev_upload(a, lattice)
    try:
        for k, (params, lut) in enumerate(PC.EDGE_PARAMS[op_id]):
            want = oracle_run(lattice, op_id, params, lut)
            d = difference(gpu_run(gpu, lattice, op_id, params, lut), want, lattice)
            assert d is None, f"{op_id} set {k} {show(params)}: {d}"
            if two_packs:
                if PC.non_finite_set(params):
                    d = difference(gpu_run(gpu, lattice, op_id, params, lut, sparse=PC.FROM_FLAT), oracle_run(lattice, op_id, params, lut, sparse=PC.FROM_FLAT), lattice)
                    assert d is None, f"{op_id} set {k} {show(params)} FROM_FLAT: {d}"
                gpu.r.chain_dev(a, b, w, h, [chain_op(op_id, params, lut)])
                gpu.r.synchronize()
                d = difference(gpu.r.dev_download(b, lattice.shape), want, lattice)
                assert d is None, f"{op_id} set {k} {show(params)} as a chain: {d}"
    finally:
        if two_packs:
            gpu.r.dev_free(a)
            gpu.r.dev_free(b)


# ------------------------------------------------------------------ 5: the table ops' own entries
def test_auto_levels_and_levels_paths(gpu, oracle):
    """auto_levels (min / max reduction, then the table kernel) and levels on an image of whole chunks and on one with ragged 16-byte rows"""
    for (w, h) in ((128, 64), (132, 70)):
        for seed in PC.path_seeds((w, h)):
            img = PC.path_image(w, h, seed)
            narrow = (img // 3 + 40).astype(np.uint8)      # channel ranges that the stretch really moves
            narrow[..., 3] = img[..., 3]
            mask = np.zeros((h, w), np.uint8)
            mask[5:h - 9, 17:w - 30] = 255
            for src in (img, narrow):
                d = difference(gpu.auto_levels(src), oracle.auto_levels(src), src)
                assert d is None, f"auto_levels {w}x{h} seed {seed}: {d}"
                d = difference(gpu.auto_levels(src, mask), oracle.auto_levels(src, mask), src)
                assert d is None, f"auto_levels masked {w}x{h} seed {seed}: {d}"
                for args in ((20.0, 235.0, 1.2, 10.0, 240.0), (0.0, 255.0, 1.0, 0.0, 255.0), (200.0, 50.0, 0.5, 255.0, 0.0)):
                    d = difference(gpu.levels(src, *args), oracle.levels(src, *args), src)
                    assert d is None, f"levels {args} {w}x{h} seed {seed}: {d}"
                    d = difference(gpu.levels(src, *args, mask=mask), oracle.levels(src, *args, mask=mask), src)
                    assert d is None, f"levels {args} masked {w}x{h} seed {seed}: {d}"
