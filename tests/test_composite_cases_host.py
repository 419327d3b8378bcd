"""tests/composite_cases.py reaches the kernel states it was written for (computed with numpy from the table alone), and the oracle alone handles every
value in it: the hand-derived results of canvas_state.rs:505-698, :1246-1422 and layers.rs:276-325 are fixed here, every other adjustment row must change the
picture, and the whole table goes through the oracle in a time that is printed (measured: 2.5 s for 3600 composites, under a millisecond each)."""
import time

import numpy as np
import pytest

from . import composite_cases as CC
from . import oracle_lib as O

T, F_ = CC.K_TEMPLATE | CC.P_GENERAL, CC.P_FAST   # flatten_kernel<true, .>; the fast-division bit


def every_group():
    return {"A": CC.group_a(), "B rows": [c for _, a, b in CC.group_b_rows() for c in (a, b)], "B positions": CC.group_b_positions(),
            "B modes": CC.group_b_modes(), "B canvases": CC.group_b_canvases(), "C": CC.group_c(),
            "D": [c for s in CC.D_CANVASES for c in CC.group_d(*s)], "E": [c for s in CC.E_CANVASES for c in CC.group_e(*s)],
            "F": [c for s in CC.F_CANVASES for c in CC.group_f(*s)]}


def test_the_lattice_holds_every_alpha_conceal_pair_once():
    img, mask = CC.lattice()
    pairs = img[..., 3].astype(np.uint32) * 256 + mask
    assert pairs.size == 65536 and len(np.unique(pairs)) == 65536


def test_the_oracles_masked_alpha_is_the_integer_formula():
    """canvas_state.rs:660-665 read off an Overwrite layer at 1.0 (its alpha is the layer's, :1275-1281; alpha 0 keeps the transparent base's 0)"""
    img, mask = CC.lattice()
    case = next(c for c in CC.group_a() if "over transparent mode 14 opacity 1.0" in c.name)
    a, c = img[..., 3].astype(np.uint32), mask.astype(np.uint32)
    assert np.array_equal(case.want(O.composite)[..., 3], a * (255 - c) // 255)


def test_group_a_covers_the_routes_and_the_extras():
    names = [c.name for c in CC.group_a()]
    for base in CC.BASES:
        for mode, opacity in CC.A_DESCRIPTORS:
            for route in (CC.STORE, CC.DEV):
                assert f"lattice over {base} mode {mode} opacity {opacity} {route}" in names
    a = {c.name: c for c in CC.group_a()}
    assert a["mask set"].path() == (T | F_, 0xFF) and a["mask cleared with NULL"].fast_kernel() and a["mask on a hidden layer store"].fast_kernel()
    assert a["mask set"].layers[1]["pixels"] is a["mask cleared with NULL"].layers[1]["pixels"]     # the store keeps the pixels and only drops the mask
    vanished = a["all-255 mask: the layer vanishes, its chunks stay populated store"].want(O.composite)
    pop = CC.populated(a["all-255 mask: the layer vanishes, its chunks stay populated store"].layers[1]["pixels"])[CC.chunk_of_pixels(*CC.LATTICE)] != 0
    assert pop.any() and not pop.all()
    assert (vanished[pop] == (255, 255, 255, 0)).all() and (vanished[~pop] == 0).all()   # Invert over an active, empty accumulator; inactive chunks stay 0


def test_every_adjustment_row_changes_the_picture_or_is_a_fixed_identity():
    rows = CC.group_b_rows()
    assert len(rows) == len(CC.EXPOSURE_EV) + len(CC.BRIGHTNESS) * len(CC.CONTRAST) + len(CC.MIXERS) + 4 * len(CC.OPACITIES)
    without = {}
    for row, case, twin in rows:
        for c in (case, twin):
            assert c.layers[1] == row.layer() or (row.layer()["opacity"] != row.layer()["opacity"] or any(v != v for v in row.params))   # NaN != NaN
            key = id(c.layers[-1])
            if key not in without:
                without[key] = O.composite(CC.b_without(c.layers), c.w, c.h)
            got = c.want(O.composite)
            assert np.array_equal(got, without[key]) == row.identity, f"{c.name}: identity = {row.identity}"
        own = F_ if row.opacity >= CC.FAST_DIV_MIN else 0                      # the row's own opacity counts as well (NaN fails the comparison)
        assert case.path() == (T | own, 0xFF) and twin.path() == (T, 0xFF)    # the twin: flatten_kernel<true, false>


def invert_over(src, opacity):
    h, w = src.shape[:2]
    return O.composite([dict(pixels=src), CC.adj(CC.ADJ_INVERT, (), opacity)], w, h)


def test_hand_derived_adjustment_values():
    """layers.rs:314-325: t = opacity.clamp(0, 1), out = (p * (1 - t) + adj * t).round() as u8"""
    w, h = CC.B_MAIN
    src = CC.adj_source(w, h)
    plain = O.composite([dict(pixels=src)], w, h)
    assert CC.populated(src).all()
    assert (invert_over(src, CC.NAN) == 0).all()                          # NaN.clamp is NaN, NaN as u8 is 0: every populated pixel, alpha included
    assert np.array_equal(invert_over(src, -1.0), plain)                   # t = 0
    assert np.array_equal(invert_over(src, 2.0), invert_over(src, 1.0))    # t = 1
    half = invert_over(src, 0.5)                                           # p / 2 + (255 - p) / 2 = 127.5 for every p: round half away from zero
    assert (half[..., :3] == 128).all() and np.array_equal(half[..., 3], plain[..., 3])
    # gain = 2^128 = inf: 0 * inf = NaN -> 0, p * inf = inf -> 255 (read on the opaque pixels, where the accumulator is the layer's pixel, canvas_state.rs:1258)
    out = O.composite([dict(pixels=src), CC.adj(CC.ADJ_EXPOSURE, [128.0])], w, h)
    opaque = src[..., 3] == 255
    assert np.array_equal(out[opaque][:, :3], np.where(src[opaque][:, :3] == 0, 0, 255)) and (out[opaque][:, 3] == 255).all()
    assert (src[opaque][:, :3] == 0).any()
    # an Invert at the bottom of the stack meets the empty accumulator of every active chunk
    dot = np.zeros((3, 5, 4), np.uint8)
    dot[1, 2] = (9, 8, 7, 255)
    out = O.composite([CC.adj(CC.ADJ_INVERT), dict(pixels=dot)], 5, 3)
    assert tuple(out[1, 2]) == (9, 8, 7, 255) and (np.delete(out.reshape(-1, 4), 7, 0) == (255, 255, 255, 0)).all()
    bottom = next(c for c in CC.group_b_positions() if c.name == "bottom of the stack")
    assert bottom.layers[0]["kind"] == CC.ADJ_INVERT and bottom.layers[0]["opacity"] == 1.0


def test_group_b_sources_positions_and_twins():
    src = CC.adj_source(*CC.B_MAIN)
    for alpha in (0, 143, 255):
        sel = src[src[..., 3] == alpha]
        for ch in range(3):
            assert len(np.unique(sel[:, ch])) == 256, (alpha, ch)
    names = {c.name for c in CC.group_b_positions()}
    for want in ("bottom of the stack", "top", "two in a row", "three in a row", "between rasters", "hidden", "adjustment layers only", "every raster hidden"):
        assert want in names and want + ", zero-opacity twin" in names
    for cases in (CC.group_b_positions(), CC.group_b_modes(), CC.group_b_canvases()):
        for c in cases:
            twin = c.name.endswith("zero-opacity twin")
            if c.name == "hidden":    # no visible adjustment layer: a raster-only stack
                assert c.fast_kernel()
            else:
                assert c.path() == ((T, 0xFF) if twin else (T | F_, 0xFF)), c.name
    assert {c.layers[3]["mode"] for c in CC.group_b_modes()} == set(range(25))
    # the mixer below the 25 modes does rewrite alpha: transparent accumulators become opaque, opaque ones lose their alpha
    c = CC.group_b_modes()[0]
    out = O.composite(c.layers[:3], c.w, c.h)
    assert ((out[..., 3] == 255) & (src[..., 3] == 0)).any() and ((out[..., 3] < 255) & (src[..., 3] == 255)).any()
    assert {(c.w, c.h) for c in CC.group_b_canvases()} == set(CC.CANVASES)


@pytest.mark.parametrize("size", CC.C_CANVASES)
def test_group_c_has_active_inactive_and_mixed_quads(size):
    w, h = size
    seen_active = seen_inactive = mixed = 0
    for variant in range(len(CC.ROLES)):
        act = CC.pixel_activity(w, h, variant)
        layers = CC.activity_layers(w, h, variant)
        union = np.zeros_like(CC.populated(layers[0]["pixels"]))
        for L in layers:
            if L.get("visible", True) and not CC.is_adj(L):
                union |= CC.populated(L["pixels"])
        assert np.array_equal(union[CC.chunk_of_pixels(w, h)] != 0, act)          # the layout is what the images hold
        out = O.composite(layers, w, h)
        assert (out[~act] == 0).all()                                              # inactive stays (0, 0, 0, 0) under the Invert and the mixer
        ghost = layers[3]["pixels"]
        assert (ghost[..., 3] == 0).all() and (ghost[..., :3] != 0).any() == ("ghost" in CC.roles_of(w, h, variant))
        seen_active += int(act.any()); seen_inactive += int((~act).any()); mixed += CC.mixed_quads(act)
    assert seen_active and seen_inactive and mixed
    if w == 66:   # the quad over x = 62 .. 65 of row 1 (pixel indices 128 .. 131) has one side in each chunk
        act = CC.pixel_activity(w, h, 0).ravel()
        assert act[128:130].all() and not act[130:132].any()
    kinds = {c.route for c in CC.group_c() if (c.w, c.h) == size}
    assert kinds == {CC.STORE, CC.DEV, CC.KEYS}
    keyed = [c for c in CC.group_c() if (c.w, c.h) == size and c.keys is not None]
    assert any(not k.keys.any() for k in keyed) and any(k.keys.all() for k in keyed)
    assert any(((k.keys != 0) & (CC.populated(k.layers[0]["pixels"]) == 0)).any() and not k.keys.all() for k in keyed)   # a transparent chunk marked as held
    for k in keyed:   # the keys never leave out a chunk a visible layer holds
        for L in k.layers:
            if L.get("visible", True) and not CC.is_adj(L):
                assert not ((CC.populated(L["pixels"]) != 0) & (k.keys == 0)).any()


@pytest.mark.parametrize("size", CC.D_CANVASES)
def test_group_d_image_holds_every_alpha_pair_in_a_present_chunk(size):
    w, h = size
    S = CC.PreviewStacks(w, h)
    if w * h >= 90:
        for cp in ("ones", "checker"):
            on = CC.present(cp, w, h)[CC.chunk_of_pixels(w, h)] != 0
            pairs = {(int(a), int(b)) for a, b in zip(S.active[..., 3][on], S.preview[..., 3][on])}
            assert pairs == {(a, b) for a in CC.LAYER_ALPHAS for b in CC.PREVIEW_ALPHAS}
            cols = S.preview[on][:, :3]
            assert (cols == 0).all(1).any() and (cols == 255).all(1).any() and ((cols != 0) & (cols != 255)).any()
    assert (S.ghost[..., 3] == 0)[CC.chunk_of_pixels(w, h) == CC.chunk_of_pixels(w, h).max()].all() and (S.ghost[..., :3] != 0).any()
    cases = CC.group_d(w, h)
    seen = {(c.preview["blend_mode"], bool(c.preview.get("is_eraser")), bool(c.preview.get("replaces_layer"))) for c in cases}
    if size == CC.D_CANVASES[-1]:
        assert seen >= {(m, e, r) for m in CC.PREVIEW_MODES for e, r in ((False, False), (True, False), (False, True))}
    for position in CC.POSITIONS:
        for cp in CC.CHUNK_PRESENT:
            for with_adj in (False, True):
                for route in (CC.STORE, CC.DEV):
                    assert any(f"chunk_present {cp} active {position} adj {with_adj} {route}" in c.name for c in cases)
    assert all(c.path()[0] & (CC.P_PREVIEW | CC.P_GENERAL) == (CC.P_PREVIEW | CC.P_GENERAL) for c in cases)


@pytest.mark.parametrize("size", CC.E_CANVASES)
def test_group_e_rectangles_realise_every_alignment(size):
    w, h = size
    rects = [r for _, r in CC.rectangles(w, h)]
    assert {(x % 4, rw % 4) for x, _, rw, _ in rects} == {(a, b) for a in range(4) for b in range(4)}
    assert {rw for _, _, rw, _ in rects} >= set(range(1, 9))
    aligned = set()
    for x, y, rw, rh in rects:   # flatten_kernel: p0 = (y0 + ry) * w + x0 + 4 qx, o0 = ry * rw + 4 qx; the 16-byte path needs (p0 | o0) & 3 == 0 and a whole quad
        for ry in range(rh):
            for qx in range((rw + 3) // 4):
                aligned.add((((y + ry) * w + x + 4 * qx) | (ry * rw + 4 * qx)) & 3 == 0 and 4 * qx + 4 <= rw)
    assert aligned == {True, False}
    for r in rects + [(0, 0, w, h)]:
        assert r[0] + r[2] <= w and r[1] + r[3] <= h and r[2] and r[3]
    for x, y, rw, rh in CC.refused_rectangles(w, h):
        assert not (rw and rh and x + rw <= w and y + rh <= h)
    assert {(1, 1)} <= {(rw, rh) for _, _, rw, rh in rects} and (0, h // 2, w, 1) in rects and (w - 1, 0, 1, h) in rects
    if w > 64 and h > 64:   # across the corner (64, 64), whose four chunks differ in activity
        act = CC.pixel_activity(w, h, CC.E_VARIANT)
        assert len({bool(act[63, 63]), bool(act[63, 64])}) == 2 and len({bool(act[64, 63]), bool(act[64, 64])}) == 2
        assert any(x < 64 < x + rw and y < 64 < y + rh for x, y, rw, rh in rects)
    cases = CC.group_e(w, h)
    assert all(c.path()[0] & CC.P_REGION for c in cases if c.expect == CC.ORACLE)
    assert sum(c.expect == CC.STATUS for c in cases) == 2 * len(CC.refused_rectangles(w, h))


def test_group_f_sits_on_both_sides_of_the_threshold():
    assert CC.F_SLOW[-1] < CC.FAST_DIV_MIN == 2.0 ** -40 and CC.F_SLOW[-2] == 2.0 ** -41
    for size in CC.F_CANVASES:
        cases = CC.group_f(*size)
        assert {c.layers[2]["mode"] for c in cases} == set(range(25)) | {25, 255}
        for c in cases:
            o = c.layers[2]["opacity"]
            slow = any(o is s or o == s for s in CC.F_SLOW)
            assert (c.path() == (CC.K_TEMPLATE, 0xFF)) == slow and c.fast_kernel() == (not slow), c.name    # flatten_kernel<false, false> or a fast kernel
    alpha = CC.group_f(67, 66)[0].layers[0]["pixels"][..., 3].ravel()
    assert {0, 77, 143, 200, 255} <= set(alpha.tolist())


@pytest.mark.parametrize("n_layers", [6, 18])
@pytest.mark.parametrize("seed", CC.SESSION_SEEDS)
def test_session_scripts_hold_every_step_kind(seed, n_layers):
    steps, doc = CC.session(seed, n_layers)
    kinds = [s["kind"] for s in steps]
    assert len(steps) >= 60 and set(kinds) == set(CC.STATE_STEPS + CC.COMPOSITE_STEPS)
    assert kinds[0] in CC.STATE_STEPS
    for kind in ("composite_full", "composite_rect", "composite_preview"):
        assert any(k == kind and kinds[i - 1] in CC.STATE_STEPS for i, k in enumerate(kinds))
    for i, k in enumerate(kinds):
        if k == "composite_repeat":   # the same composite twice in a row
            assert kinds[i - 1] == "composite_full" and steps[i]["info"] == steps[i - 1]["info"]
    paths = {CC.Case("", doc.w, doc.h, s["layers"], preview=s.get("preview"), rect=s.get("rect")).path()[0] for s in steps if s["kind"] in CC.COMPOSITE_STEPS}
    assert any(p & CC.P_PREVIEW for p in paths) and any(p & CC.P_REGION for p in paths) and CC.P_FAST in paths and (T | F_) in paths
    assert len(doc.store) == n_layers and len(doc.order) >= n_layers + 1
    # a same-generation upload leaves the mirror alone; a hole opens and closes inside layer 1's opaque chunk
    x, y, pw, ph = CC.HOLE
    first = next(s for s in steps if s["kind"] == "upload" and s["idx"] == 1)["pixels"]
    assert (first[y:y + ph, x:x + pw, 3] == 255).all() and x // 64 == (x + pw - 1) // 64 == 1
    assert any(s["kind"] == "open_hole" and (s["pixels"][..., 3] == 0).all() for s in steps)


def test_the_oracle_finishes_the_whole_table():
    t0 = time.perf_counter()
    n = 0
    for name, cases in every_group().items():
        for c in cases:
            if c.expect == CC.ORACLE:
                out = c.want(O.composite)
                assert out.shape == ((c.rect[3], c.rect[2], 4) if c.rect else (c.h, c.w, 4))
                n += 1
    for seed in CC.SESSION_SEEDS:
        for n_layers in (6, 18):
            steps, doc = CC.session(seed, n_layers)
            for s in steps:
                if s["kind"] in CC.COMPOSITE_STEPS:
                    CC.Case("", doc.w, doc.h, s["layers"], preview=s.get("preview"), rect=s.get("rect")).want(O.composite)
                    n += 1
    dt = time.perf_counter() - t0
    print(f"oracle: {n} composites in {dt:.2f} s, {1e3 * dt / n:.2f} ms each")
    assert n > 3000
