"""The tables of tests/pointwise_cases.py, held to the conditions that make them worth running on the device — with the CPU oracle alone (no GPU).  A set that
is in the tables "for a tie" or "for a branch" has to reach that tie or branch; an image that is there "for a dropped chunk" has to make the oracle drop one.
These are conditions, not measurements: when one fails, the table is wrong."""
import ctypes as C

import numpy as np
import pytest

from . import oracle_lib as O
from . import pointwise_cases as PC

f32 = np.float32


@pytest.fixture(scope="module")
def cube():
    img = PC.colour_cube()
    img.setflags(write=False)
    return img


def oracle_run(img, op_id, params, lut=None, mask=None, sparse=PC.DENSE):
    kind, op = PC.split_id(op_id)
    if kind == "rhai":
        return O.rhai_adjust(img, op, PC.oracle_rhai_params(op, params))
    return O.adjust(img, op, params, lut=lut, mask=mask, sparse=sparse)


def rgb_to_hsl(r, g, b):
    h, s, l = C.c_float(), C.c_float(), C.c_float()
    O.lib().pfxo_rgb_to_hsl(C.c_float(r / 255.0), C.c_float(g / 255.0), C.c_float(b / 255.0), C.byref(h), C.byref(s), C.byref(l))
    return f32(h.value), f32(s.value), f32(l.value)


def chunk_is_zero(img):
    """per 64 x 64 chunk (row-major): every byte of the chunk is zero"""
    h, w = img.shape[:2]
    return np.asarray([not img[y0:y1, x0:x1].any() for (x0, y0, x1, y1) in PC.chunk_boxes(w, h)])


# ------------------------------------------------------------------ the images
def test_cube_holds_every_colour_and_every_alpha_and_no_empty_chunk(cube):
    assert cube.shape == (4096, 4096, 4)
    px = cube.reshape(-1, 4).astype(np.uint32)
    key = px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)
    assert np.array_equal(key, np.arange(1 << 24, dtype=np.uint32))            # pixel i is colour i: all 2^24, once each
    i = np.arange(1 << 24, dtype=np.uint64)
    assert np.array_equal(px[:, 3], ((i * 2654435761) % (1 << 32)) >> 24)
    assert len(np.unique(cube[..., 3])) == 256
    zero = float((cube[..., 3] == 0).mean())
    assert 0.0038 < zero < 0.0040, zero                                          # 1 / 256 = 0.39 %
    assert cube[..., 3].reshape(64, 64, 64, 64).max(axis=(1, 3)).min() > 0       # no chunk of zero alpha: the sparse modes equal the dense one here
    for op, params in (("hsl", [47, 35, -12]), ("invert_alpha", [])):
        dense = O.adjust(cube, op, params)
        assert np.array_equal(O.adjust(cube, op, params, sparse=PC.IN_PLACE), dense), op


def test_lattice_takes_the_interior_path_and_holds_the_neighbours_of_every_clamp():
    img = PC.lattice()
    h, w = img.shape[:2]
    n = len(PC.LATTICE_VALUES) ** 3
    assert w == 512 and h >= 128 and (h - 1) * w < n <= h * w                   # whole interior chunks, the padding only in the last row
    assert {0, 1, 2, 127, 128, 129, 253, 254, 255} <= set(PC.LATTICE_VALUES) and set(range(0, 256, 5)) <= set(PC.LATTICE_VALUES)
    flat = img.reshape(-1, 4)
    assert len(np.unique(flat[:n, :3], axis=0)) == n
    assert not flat[n:].any()
    assert {int(a) for a in np.unique(flat[:n, 3])} == set(PC.LATTICE_ALPHAS)
    assert ((flat[:n, 3] == 0) & (flat[:n, :3].max(axis=1) > 0)).any()          # transparent but coloured


def test_path_shapes_cover_every_path_and_every_swizzle_residue():
    shapes = set(PC.PATH_SHAPES)
    assert len(shapes) == len(PC.PATH_SHAPES)
    for s in [(64, 64), (128, 64), (192, 128), (68, 64), (64, 65), (132, 70), (197, 141), (63, 64), (1, 1), (3, 130), (130, 1), (5, 3)]:
        assert s in shapes, s
    assert {PC.n_chunks(64 * n, 64) % 8 for n in range(1, 18) if (64 * n, 64) in shapes} == set(range(8))
    assert all((64 * n, 64) in shapes for n in range(1, 18))
    for (w, h) in PC.INTERIOR_SHAPES + PC.STRIP_SHAPES:
        assert w % 64 == 0 and h % 64 == 0
    for (w, h) in PC.VEC_EDGE_SHAPES:
        assert w % 4 == 0 and (w % 64 or h % 64) and w >= 64 and h >= 64      # 16-byte rows, a ragged chunk next to a whole one
    for (w, h) in PC.SCALAR_SHAPES:
        assert w % 4 != 0


@pytest.mark.parametrize("shape", [s for s in PC.PATH_SHAPES if PC.n_chunks(*s) >= 2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_path_images_hold_the_chunks_the_sparse_modes_treat_differently(shape):
    w, h = shape
    seen = set()
    for seed in PC.path_seeds(shape):
        img = PC.path_image(w, h, seed)
        assert img.shape == (h, w, 4)
        assert np.array_equal(img, PC.path_image(w, h, seed))                   # deterministic
        assert ((img[..., 3] == 0) & (img[..., :3].max(axis=-1) > 0)).any()     # transparent but coloured
        for (x0, y0, x1, y1) in PC.chunk_boxes(w, h):
            a = img[y0:y1, x0:x1, 3]
            if not a.any():
                seen.add("zero")
            elif (a == 255).all():
                seen.add("full")
            elif np.count_nonzero(a) == 1 and a[-1, -1] != 0:
                seen.add("single")
    assert seen == {"zero", "full", "single"}, seen


# ------------------------------------------------------------------ the every-colour sets
def test_every_op_has_sets_and_every_set_has_what_its_op_reads():
    assert set(PC.ADJUST_PARAMS) == set(PC.ADJUST_OPS) == set(O.OPS) and set(PC.RHAI_PARAMS) == set(PC.RHAI_OPS) == set(O.RHAI_OPS)
    assert len(PC.OP_IDS) == 24
    need = {"brightness_contrast": 2, "hsl": 3, "exposure": 1, "highlights_shadows": 2, "temperature_tint": 2, "threshold": 1, "posterize": 1,
            "color_balance": 9, "black_and_white": 3, "vibrance": 1, "sepia_strength": 1, "levels": 3}
    for op_id in PC.OP_IDS:
        kind, op = PC.split_id(op_id)
        sets = PC.every_colour_sets(op_id)
        assert 1 <= len(sets) <= {"hsl": 12, "posterize": 5}.get(op_id, 4), op_id
        for params, lut in sets:
            assert len(params) == need.get(op, 0), (op_id, params)
            assert (lut is not None) == (kind == "adjust" and op in ("lut_rgba", "gradient_map")), op_id
            if lut is not None:
                assert np.asarray(lut).dtype == np.uint8 and np.asarray(lut).size == 1024
    for op_id, sets in PC.EDGE_PARAMS.items():
        kind, op = PC.split_id(op_id)
        assert all(len(params) == need[op] and lut is None for params, lut in sets), op_id


def test_threshold_sets_split_the_cube_except_at_the_two_ends(cube):
    levels = [p[0] for p, _ in PC.ADJUST_PARAMS["threshold"]]
    assert levels == [0.0, 127.5, 255.0, 255.5]
    for lv in levels:
        out = O.adjust(cube, "threshold", [lv])
        assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()
        got = {int(v) for v in np.flatnonzero(np.bincount(out[..., 0].ravel(), minlength=256))}
        want = {255} if lv == 0.0 else {0} if lv == 255.5 else {0, 255}
        assert got == want, (lv, got)


def test_posterize_sets_leave_exactly_k_levels_per_channel(cube):
    ks = [int(p[0]) for p, _ in PC.ADJUST_PARAMS["posterize"]]
    assert ks == [2, 3, 4, 255, 256]
    for k in [k for k in ks if k <= 16]:
        out = O.adjust(cube, "posterize", [float(k)])
        for c in range(3):
            assert np.count_nonzero(np.bincount(out[..., c].ravel(), minlength=256)) == k, (k, c)


def test_hsl_sectors_arms_and_hue_boundaries_occur(cube):
    px = cube.reshape(-1, 4)
    r, g, b = (px[:, c].astype(np.int16) for c in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    # the reference's if-chain: max == r first, then max == g, else b; l > 0.5 <=> max + min > 255
    for name, sel in (("grey", grey), ("red", ~grey & (mx == r)), ("green", ~grey & (mx != r) & (mx == g)), ("blue", ~grey & (mx != r) & (mx != g))):
        assert sel.any(), name
        if name != "grey":
            assert (sel & (mx + mn > 255)).any() and (sel & (mx + mn <= 255)).any(), name
    # the first HSL set leaves the hue alone: the green channel's t is h itself; yellows sit on 1/6, cyans on 1/2, blues on 2/3 — exactly
    params, _ = PC.ADJUST_PARAMS["hsl"][0]
    assert params == [0.0, 0.0, 0.0]
    third = f32(1.0) / f32(3.0)
    bounds = {"1/6": f32(1.0) / f32(6.0), "1/2": f32(0.5), "2/3": f32(2.0) / f32(3.0)}
    hit = {k: 0 for k in bounds}
    for k in range(1, 256):
        for (cr, cg, cb) in ((k, k, 0), (0, k, k), (0, 0, k), (k, 0, k), (k, 0, 0), (0, k, 0)):
            h, s, l = rgb_to_hsl(cr, cg, cb)
            nh = f32(h + f32(params[0]) / f32(360.0))
            nh = f32(nh - np.trunc(nh))
            tr, tb = f32(nh + third), f32(nh - third)
            tr = f32(tr - f32(1.0)) if tr > 1.0 else tr
            tb = f32(tb + f32(1.0)) if tb < 0.0 else tb
            for name, v in bounds.items():
                hit[name] += int(nh == v) + int(tr == v) + int(tb == v)
    assert all(n > 0 for n in hit.values()), hit
    # the rest of the hue family is there, and the grey branch, and both lightness ends
    hsl = [tuple(p) for p, _ in PC.ADJUST_PARAMS["hsl"]]
    for want in [(60, 0, 0), (120, 0, 0), (180, 0, 0), (-180, 0, 0), (360, 0, 0), (-360, 0, 0), (0, -100, 0), (0, 100, 0), (0, 0, 100), (0, 0, -100)]:
        assert tuple(float(v) for v in want) in hsl, want
    grey_out = O.adjust(cube, "hsl", [0.0, -100.0, 0.0])
    assert (grey_out[..., 0] == grey_out[..., 1]).all() and (grey_out[..., 1] == grey_out[..., 2]).all()   # saturation -100: hsl_to_rgb's grey branch


def unrounded(op, params, img):
    """the simple ops' unrounded f32 result, re-evaluated in numpy with the reference's operation order (no contraction): (h, w, 3)"""
    v = img[..., :3].astype(f32)
    p = [f32(x) for x in params]
    if op == "exposure":
        return v * f32(np.exp2(np.float64(p[0])))      # powf(2, integer) is exact
    if op == "temperature_tint":
        temp, tint = p[0] * f32(1.5), p[1] * f32(1.0)
        return np.stack([v[..., 0] + temp, v[..., 1] - tint * f32(0.5), v[..., 2] - temp], axis=-1)
    if op == "brightness_contrast":
        factor = (f32(259.0) * (p[1] + f32(255.0))) / (f32(255.0) * (f32(259.0) - p[1]))
        return factor * (v + p[0] - f32(128.0)) + f32(128.0)
    raise KeyError(op)


@pytest.mark.parametrize("op,index", PC.TIE_SETS, ids=[f"{o}-{i}" for o, i in PC.TIE_SETS])
def test_tie_sets_put_values_exactly_on_a_half(cube, op, index):
    params, _ = PC.ADJUST_PARAMS[op][index]
    if op == "exposure":
        assert params == [-1.0]
    if op == "temperature_tint":
        assert params == [0.0, 1.0]
    for img in (PC.lattice(), cube):
        u = unrounded(op, params, img)
        in_range = (u > 0.0) & (u < 255.0)
        ties = in_range & (u - np.floor(u) == f32(0.5))
        assert ties.sum() > 0, (op, params)
        # the re-evaluation above is the oracle's arithmetic: rounding it half away from zero gives the oracle's bytes (every value here is a multiple of 0.5)
        assert (u * f32(2.0) == np.floor(u * f32(2.0))).all()
        want = np.clip(np.floor(u) + (u - np.floor(u) >= f32(0.5)), 0, 255).astype(np.uint8)
        assert np.array_equal(O.adjust(img, op, params)[..., :3], want), (op, params)


# ------------------------------------------------------------------ the sparse modes on the path images
@pytest.mark.parametrize("shape", [s for s in PC.PATH_SHAPES if PC.n_chunks(*s) >= 2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sparse_modes_skip_and_drop_chunks_on_every_multi_chunk_shape(shape):
    w, h = shape
    img = PC.path_image(w, h, 0)
    in_place = O.adjust(img, "hsl", [47.0, 35.0, -12.0], sparse=PC.IN_PLACE)
    zeroed = chunk_is_zero(in_place)
    assert (zeroed & ~chunk_is_zero(img)).any() and (~zeroed).any()             # a coloured chunk skipped, another one alive
    for op, lut in (("invert_alpha", None), ("lut_rgba", PC.alpha_to_zero_luts())):
        dense = O.adjust(img, op, lut=lut)
        flat = O.adjust(img, op, lut=lut, sparse=PC.FROM_FLAT)
        assert (chunk_is_zero(flat) & ~chunk_is_zero(dense)).any(), op          # FROM_FLAT drops a chunk that DENSE keeps


# ------------------------------------------------------------------ the parameter edges
@pytest.mark.parametrize("op_id", sorted(PC.EDGE_PARAMS))
def test_edge_sets_have_a_defined_answer(op_id):
    """every beyond-domain and non-finite set: the oracle returns an image of the lattice's shape, twice the same one (no uninitialised read, no dependence on
    the thread schedule)"""
    img = PC.lattice()
    sets = PC.EDGE_PARAMS[op_id]
    kind, op = PC.split_id(op_id)
    n_float = len(sets[0][0])
    flat = [tuple(repr(v) for v in p) for p, _ in sets]
    for k in range(n_float):                                                       # every value at every position
        assert {repr(v) for v in PC.EDGE_VALUES} <= {t[k] for t in flat}, (op_id, k)
    for params, lut in sets:
        a = oracle_run(img, op_id, params, lut)
        b = oracle_run(img, op_id, params, lut)
        assert a.shape == img.shape and a.dtype == np.uint8
        assert np.array_equal(a, b), (op_id, params)
        assert np.array_equal(a[..., 3], img[..., 3]), (op_id, params)             # none of these ops writes alpha


def test_edge_sets_name_the_cases_the_host_folding_can_get_wrong():
    def has(op_id, params):
        return any([repr(float(v)) for v in params] == [repr(v) for v in p] for p, _ in PC.EDGE_PARAMS[op_id])
    for v in (0.0, 1.0, 1.5, 1e30):
        assert has("posterize", [v])
    assert any(p[1] == 259.0 for p, _ in PC.EDGE_PARAMS["brightness_contrast"]) and any(p[1] == -255.0 for p, _ in PC.EDGE_PARAMS["brightness_contrast"])
    assert has("exposure", [200.0]) and has("exposure", [-200.0])
    assert any(PC.non_finite_set(p) for p, _ in PC.EDGE_PARAMS["hsl"]) and any(PC.non_finite_set(p) for p, _ in PC.EDGE_PARAMS["vibrance"])
