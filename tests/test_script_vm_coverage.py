"""What the per-pixel closure corpus (tests/closure_gen.py) reaches in the compiler and the launch, measured without a device by the shape
probe (pfx_int_script_closure_shape), and the host reference the GPU differential test (test_gpu_script_vm_diff.py) compares the VM
with: the tree-walking interpreter, pinned here on closures with hand-computed results.

Launch classes: pfxk_vm_shape gives 256 lanes to n_regs <= 32, 192 to 33-42, 128 to 43-64 and 64 to 65-120, and stages the program
in LDS when lanes * n_regs * 8 + 12 * n_code (rounded to 16) fits 64 KiB.  Every class can take both LCODE values — a short program
fits beside any register file below 32 / 42 / 64 / 120 registers, and a long enough one fits beside none — and both HEAVY values,
so all 16 (lanes, lcode, heavy) combinations exist and the corpus must reach each."""
import itertools

import pytest

import paintfe_amd as P

from . import closure_gen as G
from . import closure_ref as R

# opcodes no script source produces: nothing in the compiler emits BC_ERR
UNREACHABLE = {"ERR"}


@pytest.fixture(scope="module")
def corpus():
    out = []
    for seed in G.CORPUS_SEEDS:
        p = G.generate(seed)
        out.append((p, R.closure_shape(p.device_script(), p.width, p.height)))
    return out


def test_every_program_compiles(corpus):
    assert len(corpus) == len(G.CORPUS_SEEDS)
    for p, sh in corpus:
        assert sh["n_params"] == len(p.params)
        assert sh["n_regs"] <= 120 and sh["n_code"] > 0


def test_every_source_reachable_opcode_appears(corpus):
    seen = set()
    for _, sh in corpus:
        seen |= {k for k, v in sh["ops"].items() if v}
    missing = sorted(set(R.BC_NAMES) - UNREACHABLE - seen)
    assert not missing, f"opcodes the corpus no longer reaches: {missing}"


def test_every_launch_class_appears(corpus):
    seen = {(sh["lanes"], sh["lcode"], sh["heavy"]) for _, sh in corpus}
    want = set(itertools.product((256, 192, 128, 64), (0, 1), (0, 1)))
    assert want - seen == set(), f"launch classes the corpus no longer reaches: {sorted(want - seen)}"


def test_constant_hoisting_cases_appear(corpus):
    pre = [sh for _, sh in corpus if sh["n_pre"] > 0]
    assert any(sh["n_pre"] == 0 for _, sh in corpus) and pre
    # the cap: the register file is full (120) and literals past it stay per-pixel loads behind the preamble
    assert any(sh["n_regs"] == 120 and sh["ops"]["LOADK"] > sh["n_pre"] for sh in pre)


def test_constructs_and_kinds_appear(corpus):
    seen = set()
    for p, _ in corpus:
        seen |= set(p.constructs)
    want = {"+", "-", "*", "/", "%", "**", "&", "|", "^", "<<", ">>", "neg", "!", "abs", "abs_i", "sign", "min", "max", "min_i", "max_i",
            "min_f", "max_f", "clamp", "clamp_f", "lerp", "distance", "floor", "ceil", "round", "sqrt", "pow", "sin", "cos", "tan", "atan2",
            "exp", "ln", "to_int", "to_float", "width", "height", "PI", "get_pixel", "get_r", "get_g", "get_b", "get_a", "is_selected",
            "mixed_promotion", "let", "shadowing", "+=", "if", "else_if", "while", "loop", "break", "continue", "for", "for_incl",
            "range_neg", "return", "fn_inline", "captured", "Fn_name", "result_ints", "result_mixed", "result_long", "result_short",
            "unit_result", "shift_edge", "pow_edge", "int_edge", "float_edge", "bool&&", "bool||"}
    assert want - seen == set(), sorted(want - seen)
    assert {p.kind for p, _ in corpus} == set(G.KINDS)
    errs = {m for p, _ in corpus for _, m in p.errors}
    assert errs == {m for m, _ in G.FAILURES}


# ---------------------------------------------------------------- the host reference itself
def call(closure, *args):
    lines, err = R.check_console(f"let f = {closure};\nprint(f.call({', '.join(map(str, args))}));")
    assert err is None, err
    return lines[0]


def test_host_reference_hand_computed():
    assert call("|r, g, b, a| [r * 2, g / 3, b % 7, a]", 1, 2, 3, 4) == "[2, 0, 3, 4]"
    assert call("|r, g, b, a| [-r / 2, -g % 3, r << 62, -1 >> 70]", 7, 8, 0, 0) == "[-3, -2, -4611686018427387904, -1]"
    assert call("|r, g, b, a| [to_int(2.5.round()), to_int(round(-2.5)), to_int(floor(-0.5)), to_int(ceil(-0.5))]", 0, 0, 0, 0) == "[3, -3, -1, 0]"
    assert call("|x, y, r, g, b, a| { let t = 0; for i in range(x, 0, -2) { t += i; } [t, y ** 3, r + 0.5, a] }", 7, 3, 1, 2, 3, 4) == "[16, 27, 1.5, 4]"
    assert call("|r, g, b, a| { let s = 0; let i = 0; loop { i += 1; if i > r { break; } if i % 2 == 0 { continue; } s += i; } [s, i, 0, 0] }",
                6, 0, 0, 0) == "[9, 7, 0, 0]"


def test_host_reference_modulo_overflow_message():
    """INT64_MIN % -1 is 'Modulo division overflow' (the VM said 'Division overflow' before BCE_MOD_OVERFLOW)"""
    _, err = R.check_console("let f = |r, g, b, a| [(-9223372036854775807 - 1) % (r - 2), g, b, a];\nprint(f.call(1, 2, 3, 4));")
    assert err is not None and err[0] == -6 and err[1] == 1
    assert err[2] == "Modulo division overflow: -9223372036854775808 % -1"
    assert R.same_error("Modulo division overflow", err[2]) and not R.same_error("Division overflow", err[2])


def test_statement_if_then_array_literal():
    """a statement-level `if` ends its statement (rhai's parse_stmt): the array literal after it is the next statement, not an index"""
    clo = "|r, g, b, a| { if r > 3 { return [1, 2, 3, 4]; } [r, g, b, a] }"
    assert call(clo, 1, 2, 3, 4) == "[1, 2, 3, 4]"
    assert call(clo, 9, 8, 7, 6) == "[1, 2, 3, 4]"
    assert call(clo, 2, 8, 7, 6) == "[2, 8, 7, 6]"
    # and the same closure compiles for the device
    sh = R.closure_shape(f"map_channels({clo});", 8, 8)
    assert sh["ops"]["RET_ARR"] == 2
    # the value of a trailing if-expression is still the block's value
    assert P.script_check("fn f(x) { if x > 1 { 10 } else { 20 } } print(f(2)); print(f(0));") == ["10", "20"]
    assert P.script_check("let t = 0; if true { t = 1; } -5; print(t);") == ["1"]


def test_host_reference_prelude_reads():
    img, mask = R.image(7, 5)
    assert img.min() >= 0 and mask.shape == (5, 7)
    lines, err = R.check_console(R.prelude(7, 5) + "\nprint(get_pixel(3, 2)); print(get_r(-1, 0)); print(get_a(7, 0)); print(is_selected(0, 0)); "
                                 "print(is_selected(1, 0));", 7, 5)
    assert err is None
    assert lines[0] == "[" + ", ".join(str(int(v)) for v in img[2, 3]) + "]"
    assert lines[1:] == ["0", "0", str(mask[0, 0] > 0).lower(), str(mask[0, 1] > 0).lower()]


def test_hash_inputs_reach_both_ends():
    img, mask = R.image(64, 48)
    for c in range(4):
        assert img[..., c].min() == 0 and img[..., c].max() == 255
    assert (mask == 0).any() and (mask > 0).any()


@pytest.mark.parametrize("src", ["switch r { 1 => 2, _ => 3 }", "{ let s = \"a\"; [r, g, b, a] }", "{ let c = |v| v; [r, g, b, a] }",
                                 "{ try { [r, g, b, a] } catch { [0, 0, 0, 0] } }", "{ throw 1; }", "{ do { r += 1; } while r < 3; [r, g, b, a] }"])
def test_constructs_outside_the_compiled_subset_are_unsupported(src):
    with pytest.raises(P.PfxError) as e:
        R.closure_shape(f"map_channels(|r, g, b, a| {src});", 8, 8)
    assert e.value.status == -5
