"""The tap-by-tap disc (tests/textfx_disc_cases.py) on the host: it is the model's two forms, its `clear` planes are what they claim to be, and neither they
nor the public-call cases built on `slab` and `dots` (tests/textfx_cases.py) would pass a disc with a tap missing or a tap too many.  No GPU."""
import numpy as np
import pytest

from . import textfx_cases as TC
from . import textfx_disc_cases as DC
from . import textfx_model as M

F = np.float32


# ---- disc_taps is dilate_mask, and the model's windowed form is disc_taps ------------------------------------------------------------------------------------------------
def host_planes(radius):
    yield "clear", DC.clear(radius)
    yield "salt", DC.salt()
    yield "rings", TC.text_of(TC.MEASURED)[..., 3]


@pytest.mark.parametrize("radius", DC.HOST_RADII)
def test_disc_taps_is_the_reference_and_the_model(radius):
    for name, plane in host_planes(radius):
        grown = DC.disc_taps(plane, radius)
        as_u8 = np.round(M.dilate_mask(M.coverage(plane), radius).astype(np.float64) * 255.0).astype(np.uint8)   # a / 255.0f * 255 is within 1e-4 of a
        assert np.array_equal(M.coverage(grown), M.dilate_mask(M.coverage(plane), radius)) and np.array_equal(grown, as_u8), name
        assert np.array_equal(grown, M.disc_max_u8(plane, radius)), name
        inverse = 255 - plane
        assert np.array_equal(DC.disc_taps(inverse, radius, take_min=True), M.disc_min_u8(inverse, radius)), name
        assert np.array_equal(DC.disc_taps(plane, radius, take_min=True), M.disc_min_u8(plane, radius)), name
        eroded_f32 = np.maximum(F(1.0) - M.dilate_mask(F(1.0) - M.coverage(inverse), radius), F(0))
        eroded_u8 = np.maximum(F(1.0) - (F(1.0) - M.coverage(DC.disc_taps(inverse, radius, take_min=True))), F(0))
        assert np.array_equal(eroded_u8, eroded_f32), name


def test_the_two_loops_of_disc_taps_agree():
    """the stamp per source pixel and the slice per tap are the same maximum, also with a disc that is not symmetric"""
    plane = DC.salt((67, 5))
    for radius in (1, 2.5, 9):
        for wrong in (None, DC.drop_right_of_every_row, DC.drop_last_row, DC.extra_right_of_rim_rows):
            member = DC.disc_member(radius) if wrong is None else wrong(DC.disc_member(radius))
            dense = np.maximum(plane, 1)                               # every pixel a source: the per-tap loop
            assert len(np.nonzero(dense)[0]) > member.sum() >= 1
            by_tap = DC.taps_max(dense, member)
            stamped = np.zeros_like(dense)
            for y, x in zip(*np.nonzero(dense)):                       # the per-source loop, one pixel at a time
                one = np.zeros_like(dense)
                one[y, x] = dense[y, x]
                stamped = np.maximum(stamped, DC.taps_max(one, member))
            assert np.array_equal(by_tap, stamped), (radius, wrong)


# ---- the clear planes ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", DC.SWEEP)
def test_the_clear_window_is_inside_the_image_and_empty(radius):
    w, h = DC.PLANE
    R = DC.reach_of(radius)
    assert 1 <= R <= 64 and len(DC.clear_centres(radius)) == (4 if R <= 8 else 1)
    for k, (x, y) in enumerate(DC.clear_centres(radius)):
        plane = DC.clear(radius, k)
        assert x - R - 1 >= 0 and y - R - 1 >= 0 and x + R + 1 < w and y + R + 1 < h
        window = plane[y - R - 1:y + R + 2, x - R - 1:x + R + 2]
        assert window.shape == (2 * R + 3, 2 * R + 3) and window[R + 1, R + 1] == 255 and np.count_nonzero(window) == 1
        assert sorted(plane[plane > 0].tolist()) == sorted(DC.BORDER_VALUES + [255])
        # inside the window the expected plane is 255 on the disc and below 255 off it: every tap and every neighbour of the rim is observed
        member = DC.disc_member(radius)
        got = DC.expected("clear", radius, False, k)[y - R - 1:y + R + 2, x - R - 1:x + R + 2]
        assert np.array_equal(got == 255, member[::-1, ::-1]) and np.array_equal(member, member[::-1, ::-1])
        shrunk = DC.expected("clear", radius, True, k)[y - R - 1:y + R + 2, x - R - 1:x + R + 2]
        assert np.array_equal(shrunk == 0, member)


def test_the_sweep_reaches_every_level_and_read_count():
    """build_disc gives a row of L columns the largest window of 4^level <= L columns, level at most 3, and ceil(L / 4^level) reads of it.  The row lengths
    on both sides of each level boundary, 3 | 5, 15 | 17 and 63 | 65, occur in the sweep, and with them every level and every read count"""
    lengths = {L for radius in DC.SWEEP for L in DC.row_lengths(radius)}
    assert {1, 3, 5, 15, 17, 63, 65, 129} <= lengths and max(lengths) == 129
    assert [DC.span_word(L) for L in (1, 3, 5, 15, 17, 63, 65, 129)] == [(0, 1), (0, 3), (1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (3, 3)]
    words = {DC.span_word(L) for L in lengths}
    assert {level for level, _ in words} == {0, 1, 2, 3} and {reads for _, reads in words} == {1, 2, 3, 4}
    for level in range(4):
        assert {reads for lv, reads in words if lv == level} == ({1, 3} if level == 0 else {2, 3} if level == 3 else {2, 3, 4}), level
    halos = {DC.reach_of(r) for r in DC.SWEEP}
    assert halos == set(range(1, 65))


# ---- a wrong disc would be seen ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_wrong_disc_changes_the_clear_planes(capsys):
    skipped = {name: [] for name in DC.WRONG}
    for radius in DC.SWEEP:
        for take_min in (False, True):
            for k in range(len(DC.clear_centres(radius))):
                plane = DC.holes(radius, k) if take_min else DC.clear(radius, k)
                want = DC.expected("clear", radius, take_min, k)
                for name, wrong in DC.WRONG.items():
                    got = DC.disc_taps(plane, radius, take_min, wrong=wrong)
                    if got is None:                                    # nothing to drop: only the long-row variant below a halo of 8
                        assert name == "both end taps of every row of length >= 16 dropped" and max(DC.row_lengths(radius)) < 16, (name, radius)
                        if k == 0:
                            skipped[name].append((radius, "min" if take_min else "max"))
                        continue
                    assert not np.array_equal(got, want), (name, radius, take_min, k)
    with capsys.disabled():
        print("\nskipped (variant, radius, form) pairs: " + "; ".join(f"{name}: {len(v)}" for name, v in skipped.items()))
    for name in DC.NEVER_SKIPPED:
        assert skipped[name] == []
    assert sum(len(v) for v in skipped.values()) == 2 * sum(1 for r in DC.SWEEP if max(DC.row_lengths(r)) < 16)


def test_a_tap_dropped_from_every_row_changes_the_salt_planes():
    """salt is there for discs that overlap, not for single taps (the one tap of the last row of a large disc is lost among the others: that is what
    `clear` is for), but a tap off every row shows here too"""
    name = "rightmost tap of every row dropped"
    for radius in DC.SALT_RADII:
        for take_min in (False, True):
            plane = DC.pepper() if take_min else DC.salt()
            assert 0.02 < np.count_nonzero(DC.salt()) / DC.salt().size < 0.04
            assert not np.array_equal(DC.disc_taps(plane, radius, take_min, wrong=DC.WRONG[name]), DC.expected("salt", radius, take_min)), (name, radius)


def with_a_wrong_disc(monkeypatch, wrong):
    monkeypatch.setattr(M, "disc_max_u8", lambda alpha, radius: DC.disc_taps(alpha, radius, False, wrong=wrong))
    monkeypatch.setattr(M, "disc_min_u8", lambda alpha, radius: DC.disc_taps(alpha, radius, True, wrong=wrong))


@pytest.mark.parametrize("name,size", TC.DISC_RUNS, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_the_new_public_cases_notice_a_wrong_disc(monkeypatch, name, size):
    want, counts = TC.expected_disc_case(name, size)
    image, effects = TC.DISC_CASES[name]
    stage = "outline" if "outline" in effects else "shadow"
    assert sum(counts[stage]) >= 50, counts
    text = TC.disc_text(name, size)
    with_a_wrong_disc(monkeypatch, None)                               # the model's windowed disc is the tap-by-tap one on these inputs too
    assert np.array_equal(M.apply(text, effects)[0], want)
    changed = {}
    radius = M.outline_radius(M.member(effects, "outline", M.OUTLINE_DEFAULT)) if stage == "outline" else effects["shadow"]["spread"]
    for variant, wrong in DC.WRONG.items():
        if wrong(DC.disc_member(radius)) is None:                      # no row of 16 taps in this case's disc
            changed[variant] = "nothing to drop"
            continue
        with_a_wrong_disc(monkeypatch, wrong)
        changed[variant] = not np.array_equal(M.apply(text, effects)[0], want)
    print(f"{name} {size}: {changed}")
    for variant in DC.NEVER_SKIPPED:
        assert changed[variant], variant


@pytest.mark.parametrize("width,position", TC.TILE_SHAPE_OUTLINES)
def test_the_tile_shape_outlines_notice_a_wrong_disc(monkeypatch, width, position):
    """the second image of test_the_largest_radius_and_the_two_tile_shapes: it draws, and a disc with a tap missing draws something else"""
    effects = dict(outline=dict(width=width, position=position, color=(9, 99, 199, 230)))
    image = TC.tile_shape_image(position)
    want, counts = M.apply(image, effects)
    assert sum(counts["outline"]) > 500
    for variant in DC.NEVER_SKIPPED:
        with_a_wrong_disc(monkeypatch, DC.WRONG[variant])
        assert not np.array_equal(M.apply(image, effects)[0], want), variant


def test_the_slab_keeps_its_eroded_plane():
    """the point of the slab: the minimum over the largest disc is not zero everywhere, at either size, so the 64 x 64 tile's minimum has something to get wrong"""
    for size in TC.SLAB_SIZES:
        alpha = TC.slab_image(*size)[..., 3]
        assert (alpha == 255).mean() > 0.7 and not TC.slab_image(*size)[..., :3].any()
        for radius in (3.0, 8.0, 9.0, 30.0, 64.0):
            eroded = DC.disc_taps(alpha, radius, take_min=True)
            assert len(np.unique(eroded[eroded > 0])) >= 2 and (eroded > 0).mean() > 0.2, (size, radius)
    assert np.array_equal(TC.dots_image()[..., 3], DC.clear(64))


# ---- the tight-bounds documents ---------------------------------------------------------------------------------------------------------------------------------------------
BOUNDS = {"top-left": (0, 0, 1, 1), "top-right": (299, 0, 1, 1), "bottom-left": (0, 199, 1, 1), "bottom-right": (299, 199, 1, 1), "four-corners": (0, 0, 300, 200),
          "column-256": (256, 3, 1, 1), "row-2048": (2, 2048, 1, 1), "row-2099": (4, 2099, 1, 1), "first-and-last": (0, 0, 260, 3)}


def test_the_bounds_documents():
    """each has the box it is named after, its pixels have alpha 1 and still draw, and both the region path and the whole-canvas path occur; the pad is
    ceil(4 + 4 + 0 * 3 + 2) = 10 of the shadow, which beats the outline's ceil(3) + 2"""
    assert set(BOUNDS) == set(TC.BOUNDS_DOCUMENTS)
    for name, box in BOUNDS.items():
        text = TC.bounds_document(name)
        (w, h), pixels = TC.BOUNDS_DOCUMENTS[name]
        assert text.shape == (h, w, 4) and np.count_nonzero(text[..., 3]) == len(pixels) and text[..., 3].max() == 1
        assert M.tight_bounds(text) == box, name
        out, region = TC.expected_bounds_layer(name)
        assert region["pad_px"] == 10 and region["full_canvas"] == int(name in ("four-corners", "first-and-last")), name
        assert out.any(axis=-1).sum() > len(pixels), name
