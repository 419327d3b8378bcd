"""The f64 opcode probe (tests/vm_libm_probe.py) through the host interpreter, and the interpreter's libm seam.  CPU only.

The probe's decode and encode are exact: every probe returns, through the interpreter, the bits glibc gives for the operation through ctypes
(NaN as NaN).  That also shows the interpreter is glibc, the reference's contract.  glibc's values are computed here, never committed: the GPU
machine's glibc may be another version."""
import numpy as np
import pytest

from . import closure_ref as R
from . import vm_libm_probe as P


def zero_pair(p):
    """min / max of +0 and -0: C99 and IEEE 754-2008 minNum leave the sign open.  The interpreter (fmin_first / fmax_first) and the VM give
    the first operand, as f64::min / max do on x86-64; glibc's fmin gives the second.  test_min_max_of_signed_zeros_is_the_first_operand pins it"""
    return p[0] in ("min", "max") and p[1] == 0.0 and p[2] == 0.0


def check_against_glibc(probes):
    got = P.host_eval(probes)
    bad = [(p, hex(g), hex(P.glibc(p))) for p, g in zip(probes, got) if P.canon(g) != P.glibc(p) and not zero_pair(p)]
    assert not bad, f"{len(bad)} of {len(probes)} probes differ from glibc, first: {bad[:5]}"


def test_probe_shape_is_heavy_in_both_lcode_classes():
    for lcode in (True, False):
        sh = P.shape(lcode)
        assert sh["heavy"] == 1 and sh["lcode"] == int(lcode), (lcode, sh)
        assert sh["n_params"] == 6
        for op in ("FPOW", "FSIN", "FCOS", "FTAN", "FATAN2", "FEXP", "FLN", "FSQRT", "FMOD", "FFLOOR", "FCEIL", "FROUND", "FMIN", "FMAX"):
            assert sh["ops"][op] >= 1, op


def test_probe_specials_equal_glibc():
    probes = P.specials()
    assert {p[0] for p in probes} == set(P.OPS)
    check_against_glibc(probes)


def test_min_max_of_signed_zeros_is_the_first_operand():
    probes = [(op, x, y) for op in ("min", "max") for x, y in ((0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0))]
    got = P.host_eval(probes)
    assert got == [P.f2b(p[1]) for p in probes], [hex(g) for g in got]


def test_ulps_treats_a_change_of_class_as_unbounded():
    f = P.f2b
    assert P.ulps(f(1.0), P.f2b(1.0) + 1) == 1 and P.ulps(f(P.SUB_MIN), f(0.0)) == 1 and P.ulps(f(-P.SUB_MIN), f(P.SUB_MIN)) == 2
    for x, y in ((P.DBL_MAX, P.INF), (-P.DBL_MAX, -P.INF), (0.0, -0.0), (P.NAN, 1.0), (P.INF, P.NAN), (P.INF, -P.INF)):
        assert P.ulps(f(x), f(y)) == P.UNBOUNDED, (x, y)
    assert P.ulps(f(P.NAN), f(-P.NAN)) == 0


def test_referee_refuses_infinite_results_and_signs_its_zeros():
    with pytest.raises(ValueError):
        P.referee(("pow", 0.0, -1.5))
    assert P.referee(("sin", -0.0)) == P.f2b(-0.0) and P.referee(("atan2", -0.0, 1.0)) == P.f2b(-0.0)
    assert P.referee(("pow", -0.0, 3.0)) == P.f2b(-0.0) and P.referee(("pow", -0.0, 2.0)) == P.f2b(0.0)
    assert P.referee(("pow", -P.SUB_MIN, 3.0)) == P.f2b(-0.0) and P.referee(("exp", -800.0)) == P.f2b(0.0)
    assert P.prescribed(("exp", 709.7827128933841)) and P.prescribed(("pow", -P.SUB_MIN, 3.0)) and not P.prescribed(("sin", 2.5))


def test_probe_exact_cases_equal_glibc_and_the_exact_value():
    probes = P.exact_cases()
    got = P.host_eval(probes)
    for p, g in zip(probes, got):
        assert P.canon(g) == P.glibc(p), (p, hex(g), hex(P.glibc(p)))
        assert g == P.exact_value(p), (p, hex(g), hex(P.exact_value(p)))


def test_probe_round_trips_every_binade_and_random_bits():
    """max(v, -inf) is v: the decode and encode lose no bit, subnormals and both ends of the range included"""
    rng = np.random.default_rng(3)
    vals = [v for v in (P.b2f(int(b)) for b in rng.integers(0, 1 << 63, 400, dtype=np.int64)) if v == v]   # NaN: specials
    vals += [2.0 ** e * s for e in range(-1074, 1024, 7) for s in (1.0, -1.0)]
    vals += [P.SUB_MIN, P.SUB_MAX, P.DBL_MIN, P.DBL_MAX, -P.DBL_MAX, 9007199254740991.0, 4503599627370495.5]
    probes = [("max", v, -P.INF) for v in vals]
    got = P.host_eval(probes)
    for v, g in zip(vals, got):
        assert P.canon(g) == P.canon(P.f2b(v)), (v, hex(g))


@pytest.mark.parametrize("fn", ["sin", "cos", "tan", "exp", "ln", "pow", "atan2"])
def test_probe_sweeps_equal_glibc(fn):
    probes = P.sweeps()[fn]
    check_against_glibc(probes)


def test_referee_is_within_one_ulp_of_glibc():
    """glibc's double libm is within 1 ulp of the correctly rounded result on these ranges: a check of the referee's rounding"""
    for fn, probes in P.sweeps().items():
        worst = max(P.ulps(P.referee(p), P.glibc(p)) for p in probes)
        assert worst <= 1, (fn, worst)


# ---------------------------------------------------------------- the libm seam
SEAM_SRC = """fn helper(v) { sin(v) + ln(v) }
let cap = exp(0.5);
let f = |v, w| { pow(v, w) + helper(v) + cos(v) + tan(w) + atan2(v, w) + (v ** 2) + (v ** w) + cap };
print(f.call(0.75, 1.25));
print(exp(2.0));
print(f.call(0.75, 1.25));"""


def run_seam(src=SEAM_SRC):
    lines, err = R.check_console(src)
    assert err is None, err
    return lines


def test_seam_off_changes_nothing():
    plain = run_seam()
    with P.traced() as t:
        traced = run_seam()
    assert traced == plain
    assert run_seam() == plain and P.trace() == ([], 0)


def test_seam_traces_closure_calls_only():
    with P.traced() as t:
        run_seam()
    f2b = P.f2b
    want = {(0, f2b(0.75), f2b(1.25)), (1, f2b(0.75), 0), (6, f2b(0.75), 0), (2, f2b(0.75), 0), (3, f2b(1.25), 0), (4, f2b(0.75), f2b(1.25)),
            (0, f2b(0.75), f2b(2.0))}
    assert set(t.calls) == want, sorted(set(t.calls) ^ want)   # not exp(0.5) of the header, nor exp(2.0) outside the closure
    assert t.misses == 0


def test_seam_override_answers_from_the_table():
    plain = run_seam()
    with P.traced() as t:
        run_seam()
    table = {c: P.f2b(P.b2f(P.glibc(P.call_probe(c))) + (1.0 if c[0] == 0 and c[2] == P.f2b(2.0) else 0.0)) for c in t.calls}
    with P.traced(table) as o:
        got = run_seam()
    assert o.misses == 0
    assert float(got[0]) == float(plain[0]) + 1.0 and float(got[2]) == float(plain[2]) + 1.0   # v ** 2 answered from the table
    assert got[1] == plain[1]                                                                     # exp outside the closure: glibc
    same = {c: P.glibc(P.call_probe(c)) for c in t.calls}
    with P.traced(same) as o:
        assert run_seam() == plain
    with P.traced({}) as o:
        assert run_seam() == plain
    assert o.misses == 2 * 8   # two closure calls of 8 libm calls each (pow(v, w) and v ** w are one entry), every one a miss: glibc answers
    assert run_seam() == plain


def test_seam_nudge_moves_every_finite_result():
    table = {(1, P.f2b(0.5), 0): P.f2b(1.0), (1, P.f2b(0.25), 0): P.f2b(-0.0), (1, P.f2b(2.0), 0): P.f2b(P.INF)}
    n = P.nudge(table, 3)
    assert n[(1, P.f2b(0.5), 0)] == P.f2b(1.0) + 3
    assert n[(1, P.f2b(0.25), 0)] == P.f2b(-0.0) + 3        # -0 -> the third negative subnormal
    assert n[(1, P.f2b(2.0), 0)] == P.f2b(P.INF)
