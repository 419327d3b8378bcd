"""Script front-end beyond call statements on the GPU: the reference's own scripting tests restated
(tests/scripting.rs:30-420), its goldens (scripting/for_each_pixel_invert, map_channels_invert, flip_*; transforms/flip_*,
rotate_*, resize_canvas_center), and per-pixel closures checked against numpy int64 / float64 restatements of the same
expressions.  The language runtime itself (rhai 1.25.1 in the reference, a third-party crate) has no source under the
reference tree: parity is anchored on the reference's call sites, tests and goldens, as the closure semantics are
(src/ops/scripting.rs:442-609)."""
import numpy as np
import pytest

from . import closure_ref as R
from . import inputs as I
from . import oracle_lib as O
from . import vm_libm_probe as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def grad():
    return I.create_test_gradient(64, 64)


def run(r, src, img=None, mask=None, **kw):
    return r.execute_script_sync(src, grad() if img is None else img, mask, **kw)


# ------------------------------------------------------------------ goldens
GOLDEN_SCRIPTS = [
    ("scripting/for_each_pixel_invert", "for_each_pixel(|x, y, r, g, b, a| {\n [255 - r, 255 - g, 255 - b, a]\n});", (64, 64)),
    ("scripting/map_channels_invert", "map_channels(|r, g, b, a| {\n [255 - r, 255 - g, 255 - b, a]\n});", (64, 64)),
    ("scripting/flip_horizontal", "flip_horizontal();", (64, 64)),
    ("scripting/flip_vertical", "flip_vertical();", (64, 64)),
    # tests/visual_transforms.rs:16-213 run the same imageops on a 64x48 gradient
    ("transforms/flip_canvas_h", "flip_canvas_horizontal();", (64, 48)),
    ("transforms/flip_canvas_v", "flip_canvas_vertical();", (64, 48)),
    ("transforms/flip_layer_h", "flip_horizontal();", (64, 48)),
    ("transforms/flip_layer_v", "flip_vertical();", (64, 48)),
    ("transforms/rotate_90cw", "rotate_canvas_90cw();", (64, 48)),
    ("transforms/rotate_90ccw", "rotate_canvas_90ccw();", (64, 48)),
    ("transforms/rotate_180", "rotate_canvas_180();", (64, 48)),
    ("transforms/resize_canvas_center", "resize_canvas(96, 80, \"center\");", (64, 48)),
]


@pytest.mark.parametrize("key,src,size", GOLDEN_SCRIPTS, ids=[g[0] for g in GOLDEN_SCRIPTS])
def test_script_goldens(r, golden, key, src, size):
    out, _ = run(r, src, I.create_test_gradient(*size))
    assert out.shape == golden[key].shape
    assert np.array_equal(out, golden[key])


def test_layer_transform_entry_points_match_the_goldens(r, golden):
    """the same transforms through the direct C entry points a caller uses to replay canvas ops on its other layers"""
    img = I.create_test_gradient(64, 48)
    for op, key in (("flip_horizontal", "flip_canvas_h"), ("flip_vertical", "flip_canvas_v"), ("rotate_90cw", "rotate_90cw"), ("rotate_90ccw", "rotate_90ccw"),
                    ("rotate_180", "rotate_180")):
        assert np.array_equal(r.flip_rotate(img, op), golden["transforms/" + key]), op
    assert np.array_equal(r.resize_canvas(img, 96, 80, (1, 1), (0, 0, 0, 0)), golden["transforms/resize_canvas_center"])
    assert np.array_equal(r.resize_canvas(img, 80, 64, (0, 0), (255, 0, 0, 255)), golden["transforms/resize_canvas_topleft"])
    # shrinking crops; anchors pick the kept corner (transform.rs:393-402)
    big = I.random_rgba(50, 40, 3)
    assert np.array_equal(r.resize_canvas(big, 20, 10, (2, 2), (9, 9, 9, 9)), big[30:, 30:])
    assert np.array_equal(r.resize_canvas(big, 20, 10, (1, 1), None if False else (9, 9, 9, 9)), big[15:25, 15:35])
    # flatten_image of a one-layer document (tests/visual_transforms.rs:221-228) is the compositor on that layer
    r.clear_layers()
    r.ensure_layer_texture(0, img, generation=1)
    assert np.array_equal(r.composite(64, 48, [(0, 1.0, True, 0)]), golden["transforms/flatten_single"])


# ------------------------------------------------------------------ the reference's scripting tests (tests/scripting.rs)
def test_width_height_and_interpolation(r):
    _, console = run(r, "let w = width();\nlet h = height();\nprint_line(`${w}x${h}`);")
    assert console[-1] == "64x64"


def test_set_pixel_and_get_roundtrip(r):
    out, _ = run(r, "set_pixel(0, 0, 255, 0, 0, 255);\nset_pixel(1, 0, 0, 255, 0, 128);")
    assert out[0, 0].tolist() == [255, 0, 0, 255] and out[0, 1].tolist() == [0, 255, 0, 128]
    assert np.array_equal(out[1:], grad()[1:])
    out, _ = run(r, "let r = get_r(0, 0); let g = get_g(0, 0); let b = get_b(0, 0); let a = get_a(0, 0);\nset_pixel(1, 1, r, g, b, a);")
    assert np.array_equal(out[1, 1], grad()[0, 0])
    # out-of-range accesses are ignored / read as zero; values clamp
    out, console = run(r, "set_pixel(-1, 0, 1, 2, 3, 4); set_pixel(64, 0, 1, 2, 3, 4); set_pixel(2, 2, 300, -5, 128, 1000); print(get_pixel(99, 99)); print(get_pixel(2, 2));")
    assert out[2, 2].tolist() == [255, 0, 128, 255] and console == ["[0, 0, 0, 0]", "[255, 0, 128, 255]"]


def test_flip_roundtrip_and_mixing_host_and_device_ops(r):
    out, _ = run(r, "flip_horizontal();\nflip_horizontal();")
    assert np.array_equal(out, grad())
    # host pixel writes interleaved with device effects: the mirror is synced both ways
    out, _ = run(r, "set_pixel(5, 5, 1, 2, 3, 4); apply_invert(); let p = get_pixel(5, 5); set_pixel(6, 5, p[0], p[1], p[2], p[3]); flip_vertical();")
    ref = grad()
    ref[5, 5] = [1, 2, 3, 4]
    ref = O.rhai_adjust(ref, "invert")
    ref[5, 6] = ref[5, 5]
    assert np.array_equal(out, ref[::-1])


def test_print_and_math(r):
    _, console = run(r, 'print_line("hello world");\nprint_line("second line");\nlet v = clamp(300, 0, 255);\nprint_line(`${v}`);')
    assert console == ["hello world", "second line", "255"]


def test_errors(r):
    from paintfe_amd import PfxError
    for src in ("let x = ;", "let x = 1 / 0;"):
        with pytest.raises(PfxError) as e:
            run(r, src)
        assert e.value.status == -6 and e.value.line == 1


def test_selection_api(r):
    out, _ = run(r, "select_rect(10, 10, 30, 30);\nfill_selected(255, 0, 0, 255);")
    ref = grad()
    ref[10:30, 10:30] = [255, 0, 0, 255]
    assert np.array_equal(out, ref)
    out, _ = run(r, "select_ellipse(32.0, 32.0, 15.0, 15.0);\nfill_selected(255, 0, 255, 255);")
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    inside = ((xx - 32.0) ** 2) / 225.0 + ((yy - 32.0) ** 2) / 225.0 <= 1.0
    ref = grad()
    ref[inside] = [255, 0, 255, 255]
    assert np.array_equal(out, ref)
    out, _ = run(r, "select_rect(0, 0, 10, 10);\nclear_selection();\nfill_selected(0, 0, 255, 255);")
    assert (out == np.array([0, 0, 255, 255], np.uint8)).all()
    _, console = run(r, 'print_line("before: " + has_selection());\nselect_rect(0, 0, 10, 10);\nprint_line("after: " + has_selection());\n'
                        'clear_selection();\nprint_line("cleared: " + has_selection());')
    assert console == ["before: false", "after: true", "cleared: false"]
    out, _ = run(r, "select_rect(10, 10, 54, 54);\ninvert_selection();\nfill_selected(255, 0, 255, 255);")
    ref = np.empty_like(grad())
    ref[:] = [255, 0, 255, 255]
    ref[10:54, 10:54] = grad()[10:54, 10:54]
    assert np.array_equal(out, ref)
    out, _ = run(r, "invert_selection();\nfill_selected(1, 2, 3, 4);")  # no selection -> all-zero mask -> nothing filled
    assert np.array_equal(out, grad())
    out, _ = run(r, "select_rect(20, 20, 44, 44);\ndelete_selected();")
    ref = grad()
    ref[20:44, 20:44] = 0
    assert np.array_equal(out, ref)


def test_select_rect_then_closure_with_is_selected(r):
    src = """
    select_rect(0, 0, 32, 64);
    for_each_pixel(|x, y, r, g, b, a| {
        if is_selected(x, y) {
            [255 - r, 255 - g, 255 - b, a]
        } else {
            [r, g, b, a]
        }
    });
    """
    out, _ = run(r, src)
    ref = grad()
    ref[:, :32, :3] = 255 - ref[:, :32, :3]
    assert np.array_equal(out, ref)


def test_selection_limits_core_effects_but_not_inline_ones(r):
    img = I.random_rgba(120, 80, 3)
    out, _ = run(r, "select_rect(30, 20, 100, 60); apply_box_blur(3); apply_vignette(0.8, 0.5); apply_invert();", img)
    mask = np.zeros((80, 120), np.uint8)
    mask[20:60, 30:100] = 255
    ref = O.box_blur(img, 3.0, mask)
    ref = O.vignette(ref, 0.8, 0.5, mask)
    ref = O.rhai_adjust(ref, "invert")
    assert np.array_equal(out, ref)  # vignette: the exact square, as the reference
    # a caller-supplied mask behaves like a selection made before the script
    out2, _ = run(r, "apply_box_blur(3); apply_vignette(0.8, 0.5); apply_invert();", img, mask)
    assert np.array_equal(out, out2)


# ------------------------------------------------------------------ the new effect functions of the Effect API
def test_effect_api_new_functions(r):
    img = I.random_rgba(150, 90, 4)
    r.set_exact(True)
    out, _ = run(r, "apply_reduce_noise(10.0); apply_noise(20.0, true); apply_crystallize(7); apply_bulge(0.6); apply_twist(30.0); "
                    "apply_halftone(5.0); apply_ink(40.0, 0.5); apply_oil_painting(2);", img)
    r.set_exact(False)
    ref = O.reduce_noise(img, 10.0, 2)
    ref = O.add_noise(ref, 20.0, "gaussian", True, 42, 1.0, 1)
    ref = O.crystallize(ref, 7.0, 42)
    ref = O.bulge(ref, 0.6)
    ref = O.twist(ref, 30.0)
    # everything after a +-1 LSB step may amplify it: compare the tail on the GPU's own intermediate instead
    mid, _ = run(r, "apply_reduce_noise(10.0); apply_noise(20.0, true); apply_crystallize(7); apply_bulge(0.6); apply_twist(30.0);", img)
    d = np.abs(mid.astype(int) - ref.astype(int))
    assert (d > 1).mean() < 5e-3  # crystallize averages / bilinear taps can carry an upstream LSB further in rare cells
    tail = O.oil_painting(O.ink(O.halftone(mid, 5.0, 45.0, "circle"), 40.0, 0.5), 2, 20)
    assert np.array_equal(out, tail)


# ------------------------------------------------------------------ closures vs numpy restatements
def closure_case(r, src, fn, img=None):
    img = I.random_rgba(97, 61, 11) if img is None else img
    out, _ = run(r, src, img)
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    c = img.astype(np.int64)
    ref = fn(xx, yy, c[..., 0], c[..., 1], c[..., 2], c[..., 3])
    ref = np.stack([np.clip(v, 0, 255) for v in ref], -1).astype(np.uint8)
    assert np.array_equal(out, ref)


def test_closure_integer_arithmetic_and_clamping(r):
    closure_case(r, "map_channels(|r, g, b, a| [r * 2 - 100, (g + b) / 2, b % 7 * 40, a - 300]);",
                 lambda x, y, r_, g, b, a: (r_ * 2 - 100, (g + b) // 2, b % 7 * 40, a - 300))
    closure_case(r, "for_each_pixel(|x, y, r, g, b, a| [x * 3 + y, (x ^ y) & 255, r >> 2 | 1, (g << 1) % 256]);",
                 lambda x, y, r_, g, b, a: (x * 3 + y, (x ^ y) & 255, r_ >> 2 | 1, (g << 1) % 256))
    # integer division / modulo truncate toward zero
    closure_case(r, "map_channels(|r, g, b, a| [(r - 128) / 3 + 50, (g - 128) % 5 + 10, b ** 2 / 300, a]);",
                 lambda x, y, r_, g, b, a: (np.trunc((r_ - 128) / 3).astype(np.int64) + 50, np.fmod(g - 128, 5) + 10, b ** 2 // 300, a))


def test_closure_division_on_both_sides_of_the_32_bit_fast_path(r):
    """k_script.hip divides operands that are both in [0, 2^31) as 32-bit numbers; everything else takes the 64-bit path — the quotients and remainders must not show the seam"""
    big = 2147483647   # 2^31 - 1: the last value of the fast path
    closure_case(r, f"map_channels(|r, g, b, a| [({big} + r - 255) / 16777216, ({big} + 1 + g) / 16777216 - 100, ({big} - b) % 251, (4294967296 + a) % 256]);",
                 lambda x, y, r_, g, b, a: ((big + r_ - 255) // 16777216, (big + 1 + g) // 16777216 - 100, (big - b) % 251, (4294967296 + a) % 256))
    closure_case(r, f"for_each_pixel(|x, y, r, g, b, a| [(x * 40000000) / (y + 1) % 256, (r * 16843009) / (g + 1) % 256, (0 - b - 1) / 3 + 100, (a * 36028797018963968 / 18014398509481984) % 256]);",
                 lambda x, y, r_, g, b, a: ((x * 40000000) // (y + 1) % 256, (r_ * 16843009) // (g + 1) % 256, -((b + 1) // 3) + 100, (a * 2) % 256))


def test_closure_literals_of_every_operand_kind(r):
    """pfx_rhai.cpp hoist_constants: in a straight-line closure the literals load once per lane into registers of their own — as plain operands, as the third operand
    of clamp / lerp, as elements of the result array and as distance()'s consecutive arguments (moved back into place), the same literal used several times, a
    captured constant, and literals in a closure WITH a branch (left as it is)"""
    closure_case(r, "map_channels(|r, g, b, a| [7, 255 - r, 255, 0]);", lambda x, y, r_, g, b, a: (0 * r_ + 7, 255 - r_, 0 * r_ + 255, 0 * r_))
    closure_case(r, "map_channels(|r, g, b, a| [clamp(r * 2, 10, 200), clamp(g - 300, 0, 255), 2 * g + 2, (b + 2) / 2]);",
                 lambda x, y, r_, g, b, a: (np.clip(r_ * 2, 10, 200), np.clip(g - 300, 0, 255), 2 * g + 2, (b + 2) // 2))
    closure_case(r, "let k = 3; let bias = 40; map_channels(|r, g, b, a| [r * k + bias, g * k - bias, bias, k * 60]);",
                 lambda x, y, r_, g, b, a: (r_ * 3 + 40, g * 3 - 40, 0 * r_ + 40, 0 * r_ + 180))
    closure_case(r, "for_each_pixel(|x, y, r, g, b, a| [to_int(distance(to_float(x), to_float(y), 10.0, 20.0)), to_int(lerp(to_float(r), 255.0, 0.5)), to_int(distance(0.0, 0.0, 3.0, 4.0)) * 50, a]);",
                 lambda x, y, r_, g, b, a: (np.sqrt((10.0 - x) ** 2 + (20.0 - y) ** 2).astype(np.int64), (r_ + (255.0 - r_) * 0.5).astype(np.int64), 0 * r_ + 250, a))
    closure_case(r, "map_channels(|r, g, b, a| if r > 128 { [255, g / 2, 0, a] } else { [0, g * 2, 255, a] });",
                 lambda x, y, r_, g, b, a: (np.where(r_ > 128, 255, 0), np.where(r_ > 128, g // 2, g * 2), np.where(r_ > 128, 0, 255), a))


def test_closure_control_flow_lets_and_builtins(r):
    src = """
    let threshold = 100;
    let gain = 1.5;
    fn luma(r, g, b) { (r * 299 + g * 587 + b * 114) / 1000 }
    for_each_pixel(|x, y, r, g, b, a| {
        let l = luma(r, g, b);
        let v = if l > threshold { to_int(to_float(l) * gain) } else if l < 20 { 0 } else { l / 2 };
        let acc = 0;
        for i in 0..4 { if i == 2 { continue; } acc += i * x; }
        let k = 0;
        while k < 3 && acc < 1000 { acc += y; k += 1; }
        [min(v, 255), abs(r - g), clamp(acc, 0, 255), max(a, 7)]
    });
    """

    def ref(x, y, r_, g, b, a):
        l = (r_ * 299 + g * 587 + b * 114) // 1000
        v = np.where(l > 100, np.trunc(l.astype(np.float64) * 1.5).astype(np.int64), np.where(l < 20, 0, l // 2))
        acc = 0 * x + 1 * x + 3 * x
        for _ in range(3):
            acc = np.where(acc < 1000, acc + y, acc)
        return (np.minimum(v, 255), np.abs(r_ - g), np.clip(acc, 0, 255), np.maximum(a, 7))
    closure_case(r, src, ref)


def test_closure_float_math(r):
    src = """
    map_channels(|r, g, b, a| {
        let rf = to_float(r) / 255.0;
        let s = sqrt(rf) * 255.0;
        let t = to_int(round(lerp(to_float(g), to_float(b), 0.25)));
        let u = to_int(floor(pow(to_float(b) / 255.0, 2.2) * 255.0 + 0.5));
        [to_int(s), t, u, to_int(clamp_f(to_float(a) * 1.1, 0.0, 200.0))]
    });
    """

    def ref(x, y, r_, g, b, a):
        rf = r_ / 255.0
        s = np.sqrt(rf) * 255.0
        lerp = g + (b.astype(np.float64) - g) * 0.25
        t = np.where(lerp >= 0, np.floor(lerp + 0.5), np.ceil(lerp - 0.5)).astype(np.int64)  # f64::round: half away from zero
        u = np.floor((b / 255.0) ** 2.2 * 255.0 + 0.5).astype(np.int64)
        return (np.trunc(s).astype(np.int64), t, u, np.trunc(np.clip(a * 1.1, 0.0, 200.0)).astype(np.int64))
    img = I.random_rgba(64, 50, 2)
    out, _ = run(r, src, img)
    c = img.astype(np.int64)
    exp = np.stack([np.clip(v, 0, 255) for v in ref(None, None, c[..., 0], c[..., 1], c[..., 2], c[..., 3])], -1).astype(np.uint8)
    d = np.abs(out.astype(int) - exp.astype(int))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3  # pow() on the device vs numpy's libm: last-ulp differences before floor()
    # exact: the host interpreter with the device's pow results substituted (tests/vm_libm_probe.py)
    clo = src.strip()[len("map_channels("):-2]
    h, w = img.shape[:2]
    px = [tuple(int(v) for v in img[y, x]) for y in range(h) for x in range(w)]

    def host():
        lines, err = R.check_console(f"let f = {clo};\n" + "\n".join(f"print(f.call({a}, {b}, {c}, {e}));" for a, b, c, e in px))
        return [R.parse_result(s) for s in lines], err
    (_, err), sub, table = P.substituted(r, host)
    assert err is None and sub is not None and sub[1] is None and table
    want = np.array([R.write_back(old, res) for old, res in zip(px, sub[0])], np.uint8).reshape(h, w, 4)
    assert np.array_equal(out, want), int(np.count_nonzero(out != want))


def test_closure_reads_neighbours_from_the_pre_call_image(r):
    """a 3-tap horizontal box written as a closure: get_pixel inside the closure sees the image as it was before the call"""
    src = """
    for_each_pixel(|x, y, r, g, b, a| {
        let l = get_pixel(x - 1, y);
        let rr = get_r(x + 1, y);
        [(l[0] + r + rr) / 3, (l[1] + g + get_g(x + 1, y)) / 3, b, a]
    });
    """
    img = I.random_rgba(70, 33, 8)
    out, _ = run(r, src, img)
    c = np.pad(img.astype(np.int64), ((0, 0), (1, 1), (0, 0)))  # zero outside (scripting.rs:360-366)
    ref = img.copy()
    ref[..., 0] = (c[:, :-2, 0] + c[:, 1:-1, 0] + c[:, 2:, 0]) // 3
    ref[..., 1] = (c[:, :-2, 1] + c[:, 1:-1, 1] + c[:, 2:, 1]) // 3
    assert np.array_equal(out, ref)


def test_closure_result_shapes(r):
    img = I.random_rgba(40, 30, 6)
    # unit / short arrays / non-array results leave the pixel; non-integer elements keep the old channel (scripting.rs:463-471)
    out, _ = run(r, "map_channels(|r, g, b, a| { if r > 128 { [0, 0, 0, 255] } });", img)
    ref = img.copy()
    ref[img[..., 0] > 128] = [0, 0, 0, 255]
    assert np.array_equal(out, ref)
    out, _ = run(r, "map_channels(|r, g, b, a| [1, 2, 3]);", img)
    assert np.array_equal(out, img)
    out, _ = run(r, "map_channels(|r, g, b, a| 42);", img)
    assert np.array_equal(out, img)
    out, _ = run(r, "map_channels(|r, g, b, a| [9, 1.5, true, a, 77]);", img)
    ref = img.copy()
    ref[..., 0] = 9
    assert np.array_equal(out, ref)
    out, _ = run(r, "fn inv(r, g, b, a) { [255 - r, g, b, a] }\nmap_channels(Fn(\"inv\"));", img)
    ref = img.copy()
    ref[..., 0] = 255 - ref[..., 0]
    assert np.array_equal(out, ref)


def test_for_region_bounds(r):
    img = I.random_rgba(50, 40, 9)
    for (rx, ry, rw, rh) in ((10, 5, 20, 10), (-5, -5, 20, 20), (40, 30, 100, 100), (0, 0, 0, 10), (60, 0, 5, 5), (5, 5, -3, 4)):
        out, _ = run(r, f"for_region({rx}, {ry}, {rw}, {rh}, |x, y, r, g, b, a| [x, y, 0, 255]);", img)
        x0, y0 = max(rx, 0), max(ry, 0)
        x1 = min((rx + rw) & 0xFFFFFFFF, 50)  # `(rx + rw) as u32` truncates: a negative sum wraps to a huge bound (scripting.rs:515)
        y1 = min((ry + rh) & 0xFFFFFFFF, 40)
        ref = img.copy()
        if x0 < x1 and y0 < y1:
            yy, xx = np.mgrid[y0:y1, x0:x1]
            ref[y0:y1, x0:x1] = np.stack([xx, yy, 0 * xx, 255 + 0 * xx], -1).astype(np.uint8)
        assert np.array_equal(out, ref), (rx, ry, rw, rh)


def test_closure_runtime_errors_leave_the_image_untouched(r):
    from paintfe_amd import PfxError
    img = I.random_rgba(32, 32, 5)
    img[7, 3, 0] = 0
    img[..., 0][img[..., 0] == 0] = 1
    img[20, 4, 0] = 0  # the only pixel where r == 0
    with pytest.raises(PfxError) as e:
        run(r, "map_channels(|r, g, b, a| {\n  let q = 1000 / r;\n  [q, g, b, a]\n});", img)
    assert e.value.status == -6 and "Division by zero" in str(e.value) and e.value.line == 2
    with pytest.raises(PfxError) as e:
        run(r, "map_channels(|r, g, b, a| [9223372036854775807 + r, g, b, a]);", img)
    assert "Addition overflow" in str(e.value)
    with pytest.raises(PfxError) as e:
        run(r, "map_channels(|r, g, b, a| { let n = 0; loop { n += 1; } });", img)
    assert "Too many operations" in str(e.value)
    # a long but finite loop per pixel: 1e6 iterations x 1024 pixels is far beyond the script's 50 M operations (scripting.rs:288);
    # the launch-wide budget ends it after a bounded number of steps per pixel instead of running 1e9+ VM steps
    with pytest.raises(PfxError) as e:
        run(r, "map_channels(|r, g, b, a| { let i = 0; while i < 1000000 { i += 1; } [r, g, b, a] });", img)
    assert "Too many operations" in str(e.value)
    with pytest.raises(PfxError) as e:
        run(r, "map_channels(|r, g| [r, g, 0, 0]);", img)  # wrong arity
    assert "Function not found" in str(e.value)
    with pytest.raises(PfxError) as e:
        run(r, "map_channels(|r, g, b, a| [sqrt(r), g, b, a]);", img)  # strict typing: sqrt(i64) is not registered
    assert "Function not found: sqrt (i64)" in str(e.value)


def test_readme_example_script(r):
    """the script PaintFE's README shows (README.md:52-60), on a photo-sized image"""
    src = """
    apply_desaturate();
    apply_brightness_contrast(10.0, 40.0);
    apply_vignette(0.5, 0.3);

    map_channels(|r, g, b, a| {
        [clamp(r + 15, 0, 255), g, clamp(b - 8, 0, 255), a]
    });
    """
    img = I.random_rgba(640, 427, 77)
    out, _ = run(r, src, img)
    ref = O.rhai_adjust(img, "desaturate")
    ref = O.rhai_adjust(ref, "brightness_contrast", [10.0, 40.0])
    ref = O.vignette(ref, 0.5, 0.3).astype(np.int64)
    ref[..., 0] = np.clip(ref[..., 0] + 15, 0, 255)
    ref[..., 2] = np.clip(ref[..., 2] - 8, 0, 255)
    assert np.array_equal(out.astype(np.int64), ref)  # vignette: the exact square, as the reference
    # the editor's default script (src/components/script_editor.rs:124)
    out, _ = run(r, "// Write your script here\n// Example: Invert all pixels\nmap_channels(|r, g, b, a| {\n    [255 - r, 255 - g, 255 - b, a]\n});\n", img)
    ref = img.copy()
    ref[..., :3] = 255 - ref[..., :3]
    assert np.array_equal(out, ref)


def test_canvas_ops_and_size_changes(r):
    img = I.create_test_gradient(64, 48)
    out, _, ops = run(r, "rotate_canvas_90cw(); flip_canvas_horizontal(); resize_canvas(30, 100, \"bottom-right\"); print(width()); print(height());", img, with_ops=True)
    assert out.shape == (100, 30, 4)
    assert ops == [(2, 0, 0, 0, 0), (0, 0, 0, 0, 0), (6, 30, 100, 2, 2)]
    rot = np.rot90(img, -1)[:, ::-1]  # 48 wide, 64 high
    ref = np.zeros((100, 30, 4), np.uint8)
    ox, oy = 30 - 48, 100 - 64
    ref[oy:, :] = rot[:, -ox:]
    assert np.array_equal(out, ref)
    from paintfe_amd import PfxError
    with pytest.raises(PfxError):  # the fixed-size C entry point refuses a size change
        import ctypes as C
        from paintfe_amd._lib import ScriptResult
        px = np.ascontiguousarray(img)
        res = ScriptResult()
        st = r._lib.pfx_script_run(r._h, b"rotate_canvas_90cw();", px.ctypes.data_as(C.c_void_p), C.c_uint32(64), C.c_uint32(48), None, C.byref(res))
        assert np.array_equal(px, img)
        r._check(st)


def test_script_on_a_large_image_stays_on_device(r):
    """4K image, closure + effects: the reference's interpreter would hit its 50 M operation limit on a per-pixel closure at
    this size; the compiled kernel does not count interpreter operations"""
    img = I.random_rgba(3840, 2160, 1)
    out, _ = run(r, "map_channels(|r, g, b, a| [255 - r, g / 2, b, a]); flip_horizontal();", img)
    ref = img.copy()
    ref[..., 0] = 255 - ref[..., 0]
    ref[..., 1] //= 2
    assert np.array_equal(out, ref[:, ::-1])
