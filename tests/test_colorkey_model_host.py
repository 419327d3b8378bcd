"""The colour-removal model (tests/colorkey_model.py) held to what is known without a GPU: the reference's own five unit tests (color_removal.rs:441-486, the
only recorded results for this code), its two formulations of the Color Remover's core and rings against each other, the halo argument of the device's ring
kernel on a CPU emulation, and the conditions that keep tests/test_gpu_colorkey.py from passing vacuously."""
import numpy as np
import pytest

from . import colorkey_cases as CC
from . import colorkey_model as M


def px(*rgba):
    return np.array([[rgba]], np.uint8)


# ---- the reference's unit tests as known answers -------------------------------------------------------------------------------------------------------------------
def test_exact_target_becomes_transparent():                   # :442
    assert M.color_to_alpha(px(255, 0, 0, 255))[0, 0].tolist() == [0, 0, 0, 0]


def test_distant_colour_stays_unchanged():                     # :449
    assert M.color_to_alpha(px(0, 180, 40, 255))[0, 0].tolist() == [0, 180, 40, 255]


def test_mixed_colour_is_partially_removed():                  # :456
    p = M.color_to_alpha(px(220, 35, 0, 255))[0, 0]
    assert 0 < p[3] < 255 and p[1] >= 35


def test_selection_mask_is_respected():                        # :465
    img = np.array([[(255, 0, 0, 255), (255, 0, 0, 255)]], np.uint8)
    out = M.color_to_alpha(img, np.array([[255, 0]], np.uint8))
    assert out[0, 0].tolist() == [0, 0, 0, 0] and out[0, 1].tolist() == [255, 0, 0, 255]


def test_existing_alpha_ratio_is_preserved():                  # :477
    p = M.color_to_alpha(px(255, 0, 0, 128), strength=0.5)[0, 0]
    assert 0 < p[3] < 128


def test_rounding_is_half_away_from_zero():
    assert M._round(np.array([0.5, 1.5, 2.5, 2.4999998], np.float32)).tolist() == [1.0, 2.0, 3.0, 2.0]


# ---- colour to alpha: the GPU test's cases are not vacuous -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("name", sorted(CC.CTA_SETTINGS))
def test_colour_to_alpha_cases_hold_every_kind_of_pixel(name, masked):
    img, mask, want, info = CC.cta_expected(name, 130, 70, masked)
    assert {0, 1, 255} <= set(np.unique(img[..., 3]).tolist())
    assert (~info["changed"]).any() and np.array_equal(want[~info["changed"]], img[~info["changed"]])
    block = info["changed"][3:67, 10:74]
    if name == "tolerance-0-softness-0":
        # a hard key has no partial pixel: one channel step, 1 / 255, is already beyond tolerance + softness = 0.001, so exactly the target's colour goes
        is_target = (img[..., :3] == np.array(CC.CTA_SETTINGS[name]["target"], np.uint8)).all(axis=2)
        assert np.array_equal(info["changed"], is_target & (img[..., 3] != 0) & (True if mask is None else mask != 0)) and not info["partial"].any()
    else:
        assert info["partial"].any()
    if CC.CTA_SETTINGS[name].get("alpha_floor", 0.0) > 0:
        # no alpha can reach 0 above a floor: the exact-target block sits at the floor instead, round(0.2 * 255) = 51, and nothing passes the ceiling
        assert (want[3:67, 10:74, 3][block] == 51).all() and block.any() and want[..., 3][info["changed"]].max() <= 204
    elif CC.CTA_SETTINGS[name].get("strength", 1.0) < 1:
        # nor at half strength: the removal stops at 0.5, and the exact-target block keeps about half of its alpha
        opaque = block & (img[3:67, 10:74, 3] == 255)
        assert opaque.any() and set(np.unique(want[3:67, 10:74, 3][opaque]).tolist()) <= {127, 128}
    else:
        assert info["zeroed"].any() and not want[info["zeroed"]].any()
    if masked:
        assert {0, 1, 7, 255} <= set(np.unique(mask).tolist())
        assert np.array_equal(want[mask == 0], img[mask == 0])
        for v in (1, 7, 255):
            assert info["changed"][mask == v].any()
        full = CC.cta_expected(name, 130, 70, False)[2]
        assert np.array_equal(want[mask != 0], full[mask != 0])      # 1, 7 and 255 all act as "selected"


def test_spill_rule_is_per_channel():
    img, _, with_spill, info = CC.cta_expected("default", 130, 70, False)
    without = CC.cta_expected("spill-0", 130, 70, False)[2]
    part = info["partial"]
    assert (with_spill[part][:, 0] != without[part][:, 0]).any()                     # red is a channel of the target
    assert np.array_equal(with_spill[..., 1:], without[..., 1:])                     # green and blue are not: untouched by the suppression
    orange = CC.cta_expected("target-no-zero-channel", 130, 70, False)
    assert orange[3]["partial"].any()


def test_hard_key_at_zero_softness():
    s = M.prepare(CC.CTA_SETTINGS["tolerance-0-softness-0"])
    assert s["softness"] == np.float32(0.001) and s["tolerance"] == 0


# ---- the Color Remover: two formulations ---------------------------------------------------------------------------------------------------------------------------
def all_remover_runs():
    for case in CC.REMOVER_CASES:
        for tol in CC.TOLERANCES:
            yield case, tol


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "global"])
@pytest.mark.parametrize("smoothness", CC.SMOOTHNESS)
def test_bfs_transcription_equals_the_dilation_form(smoothness, contiguous):
    changed = 0
    for case, tol in all_remover_runs():
        for with_sel in ((False, True) if (case[1], case[2]) == (130, 70) and tol == 15.0 else (False,)):
            img, seed, sel, want, info = CC.remover_expected(case[0], tol, smoothness, contiguous, with_sel)
            if M.is_noop(img, seed, sel):
                assert np.array_equal(want, img)
                continue
            bfs = M.levels_bfs(img, seed, tol, smoothness, contiguous, sel)
            assert np.array_equal(bfs, info["levels"]), (case[0], tol)
            assert bfs[seed[1], seed[0]] == 0
            changed += int(info["changed"].sum())
    assert changed > 1000


@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "global"])
@pytest.mark.parametrize("smoothness", CC.WALL_SMOOTHNESS)
def test_walled_case_bfs_equals_dilation(smoothness, contiguous):
    img, sel, want, info = CC.walled_expected(smoothness, contiguous)
    assert np.array_equal(M.levels_bfs(img, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, sel), info["levels"])
    assert np.array_equal(M.color_removal(img, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, sel, levels=M.levels_bfs), want)


def test_remover_cases_include_both_noops():
    kinds = set()
    for case in CC.REMOVER_CASES:
        img, seed = CC.remover_image(case)
        if (case[1], case[2]) == (130, 70) and M.is_noop(img, seed, CC.FC.selection()):
            kinds.add("selection")
    clear = CC.FC.clear_regions(130, 70)
    ys, xs = np.nonzero(clear[..., 3] == 0)
    assert len(ys) and M.is_noop(clear, (int(xs[0]), int(ys[0])))
    assert "selection" in kinds


# ---- the walled case's conditions ----------------------------------------------------------------------------------------------------------------------------------------
def test_walled_case_core():
    img, sel, _, info = CC.walled_expected(0, True)
    core = info["levels"] == 0
    assert int(core.sum()) == 40 * CC.WALL_H == 2800 and core[:, :40].all()
    assert int((core & (img[..., 3] == 0)).sum()) == 40           # the pocket: transparent pixels belong to the contiguous core
    glob = CC.walled_expected(0, False)[3]["levels"] == 0
    assert not (glob & (img[..., 3] == 0)).any() and int(glob.sum()) == 2800 - 40
    assert 1 in np.unique(img[..., 3]) and 7 in np.unique(sel)


@pytest.mark.parametrize("smoothness", [s for s in CC.WALL_SMOOTHNESS if s >= 20])
def test_walled_case_rings_are_geodesic_and_the_small_removal_skip_occurs(smoothness):
    img, sel, want, info = CC.walled_expected(smoothness, True)
    lv = info["levels"]
    masked_l1 = M.levels_masked_l1(lv == 0, smoothness, sel)
    assert int((lv != masked_l1).sum()) > (1000 if smoothness == 20 else 0)
    assert int(info["skipped"].sum()) >= 1
    assert (lv[sel == 0] == M.NONE).all()                         # (the core has no unselected pixel here)
    # the scopes differ by the transparent pocket: core in one, rings in the other (it lies inside the block, so the images agree: transparent pixels never change)
    other = CC.walled_expected(smoothness, False)[3]["levels"]
    pocket = img[..., 3] == 0
    assert (lv[pocket] == 0).all() and (other[pocket] > 0).all() and np.array_equal(lv[~pocket], other[~pocket])


def test_scopes_differ_visibly_where_transparent_stripes_carry_the_core():
    a = CC.remover_expected("130x70-clear-inside", 15.0, 3, True)
    b = CC.remover_expected("130x70-clear-inside", 15.0, 3, False)
    assert (a[3] != b[3]).any() and (a[4]["levels"] != b[4]["levels"]).any()


def test_walled_case_rings_cross_the_tile_column_and_fill_the_selection():
    for s in (32, 33):
        lv = CC.walled_expected(s, True)[3]["levels"]
        assert (lv[:, CC.TILE:] != M.NONE).any() and (lv[:, CC.TILE:] == M.NONE).any()
    assert CC.ring_launches(32) == 1 and CC.ring_launches(33) == 2
    lv32, lv33 = (CC.walled_expected(s, True)[3]["levels"] for s in (32, 33))
    assert (lv33 == 33).any() and np.array_equal(lv32 == M.NONE, (lv33 == M.NONE) | (lv33 == 33))
    lv70 = CC.walled_expected(70, True)[3]["levels"]
    assert CC.ring_launches(70) == 3 and ((lv70 > 64) & (lv70 != M.NONE)).any()      # the third launch has rings to add
    assert (lv70[:60, 43:100] != M.NONE).any()                                       # behind the wall, through the gap


# ---- the halo argument ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contiguous", [True, False], ids=["contiguous", "global"])
@pytest.mark.parametrize("smoothness", [0, 1, 4, 5, 9])
def test_tile_halo_chunk_scheme_equals_the_model(smoothness, contiguous):
    img, sel = CC.walled_image(), CC.walled_selection()
    want = M.levels_dilation(img, CC.WALL_SEED, CC.WALL_TOLERANCE, smoothness, contiguous, sel)
    got = M.levels_tiled(want == 0, smoothness, sel, tile=8, chunk=4)
    assert np.array_equal(got, want)
    if smoothness >= 5:
        assert (want > 4).any() and (want != M.levels_masked_l1(want == 0, smoothness, sel)).any()     # a second chunk, and the wall matters


def test_a_halo_one_short_is_not_enough():
    """the emulation is sensitive to the halo: with a window one pixel too small some interior pixel's path leaves it"""
    img, sel = CC.walled_image(), CC.walled_selection()
    want = M.levels_dilation(img, CC.WALL_SEED, CC.WALL_TOLERANCE, 9, True, sel)

    def short_halo(core, smoothness, selection, tile, chunk):
        h, w = core.shape
        blocked_img = np.asarray(selection) == 0
        cur = np.where(core, 0, M.NONE).astype(np.uint32)
        base = 0
        while base < smoothness:
            k = min(chunk, smoothness - base)
            halo = k - 1
            nxt = cur.copy()
            for y0 in range(0, h, tile):
                for x0 in range(0, w, tile):
                    ya, yb, xa, xb = max(y0 - halo, 0), min(y0 + tile + halo, h), max(x0 - halo, 0), min(x0 + tile + halo, w)
                    win, blocked = cur[ya:yb, xa:xb].copy(), blocked_img[ya:yb, xa:xb]
                    for j in range(1, k + 1):
                        win[M._grow4(win == base + j - 1) & (win == M.NONE) & ~blocked] = base + j
                    y1, x1 = min(y0 + tile, h), min(x0 + tile, w)
                    nxt[y0:y1, x0:x1] = win[y0 - ya:y1 - ya, x0 - xa:x1 - xa]
            cur, base = nxt, base + k
        return cur

    assert not np.array_equal(short_halo(want == 0, 9, sel, 8, 4), want)
