"""The script host API's model and corpus without a device: tests/script_model.py reproduces the reference's goldens and a few facts derived by hand from
src/ops/scripting.rs, its numpy transforms equal the oracle's, and tests/script_cases.py reaches the situations it is there for — counted over the
generated programs with a small state machine of what a statement sequence leaves pending (a pixel write still only in a host mirror, queued inline
effects, a live mask), which is where the ordering bugs of this layer live.  The counts are conditions: a change to the generator that loses one fails here."""
from collections import Counter

import numpy as np
import pytest

from . import inputs as I
from . import oracle_lib as O
from . import script_cases as SC
from . import script_model as M

MIN_PROGRAMS = 5   # every situation below occurs in at least this many generated programs


def model_of(prog):
    img, mask = prog.inputs()
    return M.Model(img, mask)


# ------------------------------------------------------------------ the reference's goldens
GOLDEN_PROGRAMS = {
    "scripting/for_each_pixel_invert": ((64, 64), [("closure_map_invert",)]),   # the same inversion, per pixel
    "scripting/map_channels_invert": ((64, 64), [("closure_map_invert",)]),
    "scripting/flip_horizontal": ((64, 64), [("flip_horizontal",)]),
    "scripting/flip_vertical": ((64, 64), [("flip_vertical",)]),
    "transforms/flip_canvas_h": ((64, 48), [("flip_canvas_horizontal",)]),
    "transforms/flip_canvas_v": ((64, 48), [("flip_canvas_vertical",)]),
    "transforms/flip_layer_h": ((64, 48), [("flip_horizontal",)]),
    "transforms/flip_layer_v": ((64, 48), [("flip_vertical",)]),
    "transforms/rotate_90cw": ((64, 48), [("rotate_canvas_90cw",)]),
    "transforms/rotate_90ccw": ((64, 48), [("rotate_canvas_90ccw",)]),
    "transforms/rotate_180": ((64, 48), [("rotate_canvas_180",)]),
    "transforms/resize_canvas_center": ((64, 48), [("resize_canvas", 96, 80, "center")]),
}


def test_the_golden_table_is_the_device_tests_list():
    from .test_gpu_script_lang import GOLDEN_SCRIPTS
    assert sorted(GOLDEN_PROGRAMS) == sorted(g[0] for g in GOLDEN_SCRIPTS)
    for key, _src, size in GOLDEN_SCRIPTS:
        assert GOLDEN_PROGRAMS[key][0] == size


@pytest.mark.parametrize("key", sorted(GOLDEN_PROGRAMS))
def test_model_reproduces_the_goldens(golden, key):
    size, sts = GOLDEN_PROGRAMS[key]
    m = M.Model(I.create_test_gradient(*size)).run(sts)
    assert m.pixels.shape == golden[key].shape and np.array_equal(m.pixels, golden[key])
    if key == "scripting/for_each_pixel_invert":   # the closure that asks is_selected, with nothing selected, is the same inversion
        assert np.array_equal(M.Model(I.create_test_gradient(*size)).run([("closure_each_selected",)]).pixels, golden[key])


def test_model_reproduces_the_topleft_golden(golden):
    img = I.create_test_gradient(64, 48)
    assert np.array_equal(M.resize_canvas_np(img, 80, 64, (0, 0), (255, 0, 0, 255)), golden["transforms/resize_canvas_topleft"])


# ------------------------------------------------------------------ the numpy transforms against the oracle
def targets(w, h):
    return [(w + 4, h + 6), (w + 3, h + 5), (max(w - 2, 1), max(h - 4, 1)), (max(w - 3, 1), max(h - 1, 1)), (w + 3, max(h - 3, 1)), (max(w - 3, 1), h + 3), (w, h)]


@pytest.mark.parametrize("size", SC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_numpy_transforms_equal_the_oracle(size):
    w, h = size
    img = SC.image(w, h, 5)
    for mode in O.CANVAS_OPS:
        assert np.array_equal(M.flip_rotate_np(img, mode), O.flip_rotate(img, mode)), mode
    for nw, nh in targets(w, h):
        for anchor in M.ANCHORS:
            got, want = M.resize_canvas_np(img, nw, nh, anchor, (9, 200, 31, 77)), O.resize_canvas(img, nw, nh, anchor, (9, 200, 31, 77))
            assert np.array_equal(got, want), (nw, nh, anchor)


def test_the_cases_name_every_anchor_and_filter_the_reference_parses():
    assert sorted(SC.ANCHOR_NAMES) == sorted(n for names in M.ANCHORS.values() for n in names)
    assert {M.parse_anchor(n) for n in SC.ANCHOR_NAMES} == set(M.ANCHORS) and M.parse_anchor("nowhere") == (0, 0) and M.parse_anchor("CENTER") == (1, 1)
    assert [M.parse_filter(n) for n in SC.FILTER_NAMES + ["nn", "Lanczos3", "whatever"]] == ["nearest", "bilinear", "bicubic", "lanczos3", "nearest", "lanczos3", "bilinear"]


# ------------------------------------------------------------------ facts derived by hand from the reference text
def test_select_rect_corner_truncates_to_32_bits():
    """:1365 `(x2.max(0) as u32).min(w)`: 2^32 + 5 becomes 5"""
    m = M.Model(np.zeros((4, 10, 4), np.uint8)).run([("select_rect", 0, 0, 4294967296 + 5, 4)])
    mask = m.mask.reshape(4, 10)
    assert (mask[:, :5] == 255).all() and (mask[:, 5:] == 0).all()
    assert M.Model(np.zeros((4, 10, 4), np.uint8)).run([("select_rect", 4294967296 + 5, 0, 10, 4)]).mask.reshape(4, 10)[0].tolist() == [0] * 5 + [255] * 5


def test_integer_ellipse_keeps_its_boundary_pixels():
    """:1393 centre (8, 8), radii 5 and 3: dx^2 / 25 + dy^2 / 9 <= 1 holds for |dx| <= 5, 4, 3, 0 on the rows dy = 0, 1, 2, 3; the four axis ends give exactly 1.0"""
    m = M.Model(np.zeros((17, 17, 4), np.uint8)).run([("select_ellipse", 8.0, 8.0, 5.0, 3.0)])
    mask = m.mask.reshape(17, 17)
    want = np.zeros((17, 17), np.uint8)
    for dy, half in ((0, 5), (1, 4), (2, 3), (3, 0)):
        want[8 + dy, 8 - half:8 + half + 1] = 255
        want[8 - dy, 8 - half:8 + half + 1] = 255
    assert np.array_equal(mask, want) and int((mask > 0).sum()) == 45
    assert mask[8, 13] and mask[8, 3] and mask[11, 8] and mask[5, 8] and not mask[8, 14] and not mask[12, 8]
    # radius 0 is 0.001 squared-radius: only dx == 0 survives; 1.0e200 squares to infinity and selects everything
    assert (M.Model(np.zeros((5, 9, 4), np.uint8)).run([("select_ellipse", 4.0, 2.0, 0.0, 10.0)]).mask.reshape(5, 9) > 0).sum(0).tolist() == [0, 0, 0, 0, 5, 0, 0, 0, 0]
    assert (M.Model(np.zeros((5, 9, 4), np.uint8)).run([("select_ellipse", 4.0, 2.0, 1.0e200, 1.0e200)]).mask == 255).all()


def test_centre_offsets_truncate_toward_zero():
    """:790 `((new as i32) - (old as i32)) / 2`: -3 / 2 = -1 and 3 / 2 = 1"""
    assert M.trunc_div2(-3) == -1 and M.trunc_div2(3) == 1 and M.trunc_div2(-4) == -2 and M.trunc_div2(-1) == 0
    img = SC.image(5, 5, 1)
    m = M.Model(img).run([("resize_canvas", 2, 8, "center")])
    assert m.pixels.shape == (8, 2, 4) and m.ops == [(6, 2, 8, 1, 1)]
    assert np.array_equal(m.pixels[1:6], img[:, 1:3]) and not m.pixels[0].any() and not m.pixels[6:].any()
    assert M.clamp_size(0) == 1 and M.clamp_size(-3) == 1 and M.clamp_size(40000) == 32768


def test_a_3x2_mask_is_read_flat_after_a_rotation():
    """select_rect(0, 0, 2, 1) on a 3 x 2 image leaves the bytes [255 255 0 | 0 0 0]; after rotate_canvas_90cw the image is 2 x 3 and the same bytes are rows
    [255 255] [0 0] [0 0] (:343, :630, :1445) — a mask rotated with the image would hold (1, 0) and (1, 1) instead"""
    img = SC.image(3, 2, 2)
    m = M.Model(img).run([("select_rect", 0, 0, 2, 1), ("rotate_canvas_90cw",), ("print", "is_selected", 0, 0), ("print", "is_selected", 1, 0),
                          ("print", "is_selected", 1, 1), ("print", "is_selected", 0, 1), ("fill_selected", 1, 2, 3, 4)])
    assert m.console == ["true", "true", "false", "false"] and m.ops == [(2, 0, 0, 0, 0)]
    rot = np.rot90(img, -1)
    assert m.pixels.shape == (3, 2, 4) and (m.pixels[0] == [1, 2, 3, 4]).all() and np.array_equal(m.pixels[1:], rot[1:])


def test_scalar_access_rules():
    img = SC.image(4, 3, 3)
    m = M.Model(img).run([("set_pixel", 1, 1, 300, -5, 128, 1000), ("print", "get_pixel", 1, 1), ("print", "get_pixel", 4, 0), ("print", "get_r", 0, 3),
                          ("set_a", -1, 0, 9), ("set_g", 3, 2, 256), ("print", "get_g", 3, 2), ("print", "is_selected", 4, 0), ("print", "is_selected", 3, 2),
                          ("invert_selection",), ("print", "is_selected", 3, 2), ("print", "has_selection")])
    assert m.console == ["[255, 0, 128, 255]", "[0, 0, 0, 0]", "0", "255", "false", "true", "false", "true"]
    assert M.Model(img, np.array([0, 1, 7, 200, 255, 0] * 2, np.uint8)).run([("invert_selection",)]).mask.tolist() == [255, 254, 248, 55, 0, 255] * 2


# ------------------------------------------------------------------ what the corpus reaches
CONSUMERS = {"core", "closure", "transform", "fill"}


def box_kind(st, w, h):
    rx, ry, rw, rh = st[1:]
    x0, y0, x1, y1 = max(rx, 0), max(ry, 0), min((rx + rw) & M.U32, w), min((ry + rh) & M.U32, h)
    if x0 >= x1 or y0 >= y1:
        return "outside"
    if (rx, ry, rw, rh) == (0, 0, w, h):
        return "whole"
    return "partly" if rx < 0 or ry < 0 or rx + rw > w or ry + rh > h else "inside"


def reach(prog):
    """the situations a program's statement sequence produces, and whether a mask of an old size ever meets a statement that depends on it"""
    (w, h), tags, violations = prog.size, set(), []
    dirty, pending, mask, rotated, inverted, stale, size_changes = False, 0, prog.mask_seed is not None, False, False, False, 0
    n = len(prog.statements)

    def flush(kind):
        nonlocal dirty, pending
        if dirty:
            tags.add(f"write in the mirror @ {kind}")
        if pending:
            tags.add(f"inline queued @ {kind}")
        dirty, pending = False, 0

    def needs_mask(st):
        if stale:
            violations.append(st)

    for k, st in enumerate(prog.statements):
        fn = st[1] if st[0] == "print" else st[0]
        inside = st[0] == "print" and len(st) == 4 and 0 <= st[2] < w and 0 <= st[3] < h   # a read at (x, y) inside the image
        if fn in ("fail_div", "fail_unknown"):
            tags.add("fails " + ("first" if k == 0 else "last" if k == n - 1 else "in the middle"))
            return tags, violations, size_changes
        if fn in SC.SCALAR_WRITES:
            if 0 <= st[1] < w and 0 <= st[2] < h:
                if pending:
                    tags.add("inline queued @ scalar write")
                    flush("scalar write")
                dirty = True
        elif fn in SC.SCALAR_READS:
            if inside and pending:
                tags.add("inline queued @ scalar read")
                flush("scalar read")
        elif fn == "is_selected":
            needs_mask(st)
            if inside and mask:
                if rotated:
                    tags.add("mask across a rotation @ is_selected")
                if inverted:
                    tags.add("invert_selection @ is_selected")
                inverted = False
        elif fn == "has_selection":
            needs_mask(st)
        elif fn in ("width", "height"):
            pass
        elif fn in SC.TRANSFORMS:
            changes = fn in SC.ROT90 and w != h
            if dirty and changes:
                tags.add("write in the mirror @ size change")
            flush("transform")
            if changes:
                w, h, size_changes = h, w, size_changes + 1
                rotated = rotated or mask
        elif fn in ("resize_canvas", "resize_image"):
            nw, nh = M.clamp_size(st[1]), M.clamp_size(st[2])
            assert max(nw, nh) <= SC.MAX_SIDE, st
            changes = (nw, nh) != (w, h)
            if changes or fn == "resize_canvas":
                if dirty and changes:
                    tags.add("write in the mirror @ size change")
                flush("transform")
            if changes:
                w, h, size_changes = nw, nh, size_changes + 1
                if mask:
                    stale, mask, rotated, inverted = True, False, False, False
        elif fn in ("select_rect", "select_ellipse"):
            mask, rotated, inverted, stale = True, False, False, False
        elif fn == "clear_selection":
            mask, rotated, inverted, stale = False, False, False, False
        elif fn == "invert_selection":
            needs_mask(st)
            inverted, rotated, mask = mask, rotated and mask, True
        elif fn in ("fill_selected", "delete_selected"):
            needs_mask(st)
            if mask and rotated:
                tags.add("mask across a rotation @ fill_selected")
            flush("fill_selected")
        elif fn in SC.CORE_EFFECTS:
            needs_mask(st)
            if mask and rotated:
                tags.add("mask across a rotation @ core effect")
            flush("core effect")
        elif fn in {e[0] for e in SC.INLINE_EFFECTS}:
            if dirty:
                tags.add("write in the mirror @ inline effect")
            pending += 1
            if pending >= 2:
                tags.add("two or more inline effects queued")
            if pending > SC.CHAIN_CAPACITY:
                tags.add("more than eight inline effects queued")
        elif fn.startswith("closure_"):
            kind = box_kind(st, w, h) if fn == "closure_region" else "whole-image closure"
            if fn == "closure_region":
                tags.add("for_region " + kind)
            if fn == "closure_each_selected":
                needs_mask(st)
                if mask:
                    tags.add("live mask @ closure with is_selected")
            if kind != "outside":   # an empty region visits nothing
                flush("closure")
        else:
            raise KeyError(fn)
    flush("end of script")
    return tags, violations, size_changes


REQUIRED = ["write in the mirror @ inline effect", "write in the mirror @ core effect", "write in the mirror @ closure", "write in the mirror @ size change",
            "write in the mirror @ end of script",
            "inline queued @ scalar read", "inline queued @ scalar write", "inline queued @ transform", "inline queued @ fill_selected", "inline queued @ end of script",
            "two or more inline effects queued", "more than eight inline effects queued",
            "mask across a rotation @ is_selected", "mask across a rotation @ core effect", "mask across a rotation @ fill_selected", "invert_selection @ is_selected",
            "live mask @ closure with is_selected",
            "for_region partly", "for_region outside", "for_region whole",
            "three or more size changes", "fails first", "fails last", "fails in the middle", "a failing program, then a passing one"]


def test_the_corpus_reaches_every_situation():
    progs = SC.corpus()
    counts, kinds = Counter(), Counter()
    failed_before = False
    for p in progs:
        assert 6 <= len(p.statements) <= 14, p.name
        tags, violations, size_changes = reach(p)
        assert not violations, (p.name, violations)   # no live mask meets a mask-dependent statement across a size-changing resize
        if size_changes >= 3:
            tags.add("three or more size changes")
        fails = SC.fails_at(p.statements) is not None
        if failed_before and not fails:
            tags.add("a failing program, then a passing one")
        failed_before = fails
        counts.update(tags)
        kinds.update(st[1] if st[0] == "print" else st[0] for st in p.statements)
    print(f"\n{len(progs)} programs, {sum(len(p.statements) for p in progs)} statements, {len(SC.edge_programs())} edge-table programs")
    for tag in sorted(counts):
        print(f"  {counts[tag]:4d}  {tag}")
    short = {t: counts[t] for t in REQUIRED if counts[t] < MIN_PROGRAMS}
    assert not short, short
    # every statement kind of the corpus occurs: the transforms, both resizes with all four filters, the selection calls, every effect, the closures
    names = set(SC.TRANSFORMS) | set(SC.CORE_EFFECTS) | {e[0] for e in SC.INLINE_EFFECTS} | set(SC.SCALAR_READS) | set(SC.SCALAR_WRITES) | {
        "resize_canvas", "resize_image", "select_rect", "select_ellipse", "clear_selection", "invert_selection", "fill_selected", "delete_selected", "is_selected",
        "has_selection", "width", "height", "closure_map_invert", "closure_each_selected", "closure_region", "fail_div", "fail_unknown"}
    assert not names - set(kinds), names - set(kinds)
    filters = {M.parse_filter(st[3]) for p in progs for st in p.statements if st[0] == "resize_image"}
    assert filters == set(M.FILTER_IDS)
    assert {p.size for p in progs} == set(SC.GEN_SIZES) and {p.mask_seed is None for p in progs} == {True, False}


def test_the_generator_is_deterministic_and_renders_one_statement_per_line():
    for seed in (0, 1, 7, 99):
        a, b = SC.program(seed), SC.program(seed)
        assert a.statements == b.statements and a.size == b.size
        assert len(SC.script(a.statements).split("\n")) == len(a.statements)
    assert SC.render(("select_ellipse", 1.0e200, -2.5, 0.0, 3.0)) == "select_ellipse(1.0e200, -2.5, 0.0, 3.0);"
    assert SC.render(("apply_noise", 30.0, False)) == "apply_noise(30.0, false);" and SC.render(("resize_canvas", 3, -1, "tl")) == 'resize_canvas(3, -1, "tl");'
    assert SC.render(("print", "get_pixel", -1, 4)) == "print(get_pixel(-1, 4));" and SC.render(("print", "width")) == "print(width());"


def test_the_edge_table_holds_the_pinned_rows_on_every_size():
    progs = SC.edge_programs()
    assert {p.size for p in progs} == set(SC.SIZES) and len(progs) == len(SC.SIZES) * len(SC.edge_rows(64, 4))
    for w, h in SC.SIZES:
        names = [r[0] for r in SC.edge_rows(w, h)]
        assert len(set(names)) == len(names)
        for t in SC.TRANSFORMS:
            assert t in names and t + "-twice" in names
        for a in SC.ANCHOR_NAMES:
            assert "recanvas-" + a in names
    # the pin of the device's stale-mask rule: has_selection() prints false and fill_selected fills every pixel
    for p in progs:
        if p.name.startswith("stale-mask"):
            m = model_of(p).run(p.statements)
            assert m.console == ["false"] and (m.pixels == [1, 2, 3, 4]).all() and m.pixels.shape == (p.size[1] + 1, p.size[0] + 2, 4)


def test_the_model_runs_the_whole_corpus():
    """every generated program goes through the model; a failing one stops at its failing line"""
    for p in SC.corpus():
        line = SC.fails_at(p.statements)
        if line is None:
            m = model_of(p).run(p.statements)
            assert m.pixels.dtype == np.uint8 and m.pixels.ndim == 3 and max(m.pixels.shape[:2]) <= SC.MAX_SIDE
        else:
            with pytest.raises(M.ScriptFailure) as e:
                model_of(p).run(p.statements)
            assert e.value.line == line
