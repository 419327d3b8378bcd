"""The device-libm model of the oracle (oracle_lib.libm_flavour), checked on the host (CPU only).

* Exhaustive: the oracle's restatement of the device libm_exp (k_libm.h) equals glibc's expf on every f32 in
  [-0x1.9fe368p6, 0]; vignette's powf(q, 2) equals the exact product on [0, 1]; the noise grids' device log / cos forms
  against glibc (counts printed).
* Sync: the table, constants and remainder line of the restatement are those of the device header, read as text.
* Referee: the device flavour is the correctly rounded result (mpmath, 80 bits) except at calls flagged ambiguous.
* Discrimination: on the GPU test's inputs (tests/libm_cases.py) the glibc and device flavours differ where the device
  really differs, and perturbed models (nudged results, libm_exp without fma, the unfused remainder) differ from the device
  flavour — so tests/test_gpu_libm_model.py at tolerance 0 would catch each of them.
"""
import os
import re

import numpy as np
import pytest

from . import libm_cases as LC
from . import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LIBM = os.path.join(ROOT, "paintfe_amd", "csrc", "k_libm.h")
EXP_LO = float.fromhex("-0x1.9fe368p6")
UNFUSED_BAD_X = float.fromhex("-0x1.f8cbb2p+5")   # the one argument where r = z - kd differs from glibc's expf


def _glibc_ok():
    ver = os.confstr("CS_GNU_LIBC_VERSION") if hasattr(os, "confstr") else ""
    m = re.match(r"glibc (\d+)\.(\d+)", ver or "")
    if not m or (int(m.group(1)), int(m.group(2))) < (2, 27):
        return f"glibc >= 2.27 needed for its expf algorithm (found {ver!r})"
    if not O.libm_host_has_fma():
        return "the host CPU lacks FMA: glibc selects another expf variant"
    return ""


needs_glibc_fma = pytest.mark.skipif(bool(_glibc_ok()), reason=_glibc_ok() or "ok")


# ---------------------------------------------------------------- exhaustive
@needs_glibc_fma
def test_libm_exp_equals_glibc_expf_exhaustively():
    n, _ = O.libm_check_exp(0, EXP_LO, 0.0)
    print(f"libm_exp vs expf on [-0x1.9fe368p6, 0]: {n} differences")
    assert n == 0
    # the forms before the fix: one argument wrong, the same one for both
    for variant in (1, 2):
        n, first = O.libm_check_exp(variant, EXP_LO, 0.0)
        print(f"variant {variant}: {n} differences, first at {first.hex()}")
        assert (n, first) == (1, UNFUSED_BAD_X)


def test_vignette_square_is_the_exact_product():
    n = O.libm_check_sq(library=False)
    lib = O.libm_check_sq(library=True)
    print(f"powf(q, 2) as the oracle compiles it vs (float)((double)q*q) on [0, 1]: {n}; glibc's powf routine itself: {lib}")
    assert n == 0


def test_noise_grid_counts():
    n_log, n_cos = O.libm_check_noise("log"), O.libm_check_noise("cos")
    print(f"gaussian noise grids (2^24 each): (float)log((double)u1) != logf on {n_log}, (float)cos((double)a) != cosf on {n_cos}")
    assert 0 < n_log < (1 << 24) // 50 and 0 < n_cos < (1 << 24) // 50


# ---------------------------------------------------------------- sync with the device header
def _device_text():
    with open(K_LIBM) as f:
        return f.read()


def _eval_const(expr):
    """a constant expression of hex floats, decimal literals, '*' and '/', evaluated left to right in f64 like C"""
    toks = re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+f?|\d+\.\d*|[*/]", expr)
    assert "".join(toks).replace(" ", "") == expr.replace(" ", ""), expr
    val = lambda t: float.fromhex(t.rstrip("f")) if "0x" in t else float(t)
    v = val(toks[0])
    for op, t in zip(toks[1::2], toks[2::2]):
        v = v * val(t) if op == "*" else v / val(t)
    return v


def test_restatement_matches_the_device_header():
    src = _device_text()
    tab_src = re.search(r"EXP2F_TAB\[32\]\s*=\s*\{([^}]*)\}", src).group(1)
    dev_tab = [int(t, 16) for t in re.findall(r"0x([0-9a-fA-F]+)ull", tab_src)]
    tab, consts = O.libm_exp_tables()
    assert dev_tab == [int(t) for t in tab]
    names = {}
    for name in ("InvLn2N", "SHIFT", "C0", "C1", "C2"):
        names[name] = _eval_const(re.search(rf"\b{name} = ([^,;]+)[,;]", src).group(1).strip())
    lo = _eval_const(re.search(r"if \(!\(x >= ([^)]+)\)\)", src).group(1))
    hi = _eval_const(re.search(r"if \(x > ([^)]+)\) return", src).group(1))
    assert [names[n] for n in ("InvLn2N", "SHIFT", "C0", "C1", "C2")] + [lo, hi] == list(consts)
    # the remainder is the fused form the exhaustive check holds to glibc
    r_line = re.search(r"const double r = ([^;]+);", src).group(1)
    assert re.sub(r"\s+", "", r_line) == "__builtin_fma(InvLn2N,(double)x,-kd)", r_line


# ---------------------------------------------------------------- mpmath referee
def _correctly_rounded(fn, xs):
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 80
    f = {"cos": mp.cos, "sin": mp.sin, "log": mp.log, "exp": mp.exp}[fn]
    out, margin = [], []
    for x in xs:
        v = f(mp.mpf(float(x)))
        c = np.float32(float(v))
        cands = [c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))]
        errs = [abs(mp.mpf(float(k)) - v) for k in cands]
        best = int(np.argmin(errs))
        ulp = mp.mpf(float(np.spacing(np.abs(cands[best]))))
        out.append(cands[best])
        margin.append(float(abs(ulp / 2 - errs[best]) / ulp))   # distance of v from the nearest midpoint, in f32 ulps
    return np.array(out, np.float32), np.array(margin)


@pytest.mark.parametrize("seed,fn,lo,hi", [(1, "cos", -20.0, 20.0), (2, "sin", -20.0, 20.0), (3, "cos", 0.0, 6.2831855), (4, "log", 1e-4, 1.0),
                                           (5, "exp", -104.0, 0.0), (6, "exp", -4.5, 0.0)])
def test_device_flavour_is_correctly_rounded(seed, fn, lo, hi):
    xs = np.random.default_rng(seed).uniform(lo, hi, 3000).astype(np.float32)
    want, margin = _correctly_rounded(fn, xs)
    flagged = 0
    with O.libm_flavour("device"):
        for x, w, m in zip(xs, want, margin):
            O.libm_reset()
            got = O.libm_eval(fn, x)[0]
            amb = O.libm_ambiguous()
            flagged += amb
            if got != w:
                if fn == "exp":   # glibc's expf algorithm rounds an f64 value with ~2^-34 relative error: only next to a midpoint
                    assert m < 2.0 ** -7 and abs(int(got.view(np.int32)) - int(w.view(np.int32))) == 1, (fn, float(x).hex(), m)
                else:
                    assert amb > 0, f"{fn}({float(x).hex()}): device flavour {float(got).hex()} != correctly rounded {float(w).hex()}"
    print(f"{fn} on [{lo}, {hi}]: {flagged} of {len(xs)} calls ambiguous")


# ---------------------------------------------------------------- discrimination on the GPU test's inputs
def _outputs(flavour, cases, name):
    with O.libm_flavour(flavour):
        return [getattr(O, name)(img, mask=mask, **kw) for img, kw, mask in cases]


def _n_diff(a, b):
    return sum(int((x != y).sum()) for x, y in zip(a, b))


def _twist_cases():
    return [c for a in LC.TWIST_ANGLES for c in LC.twist_cases(a)]


def test_glibc_and_device_flavours_differ_on_the_gpu_inputs():
    cases = _twist_cases()
    n = _n_diff(_outputs("glibc", cases, "twist"), _outputs("device", cases, "twist"))
    print(f"twist: glibc vs device flavour differ in {n} bytes")
    assert n > 0
    img, kw = LC.noise_knife_edge(O)
    with O.libm_flavour("device"):
        dev = O.add_noise(img, **kw)
    assert not np.array_equal(dev, O.add_noise(img, **kw)), "gaussian noise knife edge"
    for name, w, h, start, batches in LC.dab_batches():
        ref = LC.oracle_field(O, start, batches)
        with O.libm_flavour("device"):
            dev = LC.oracle_field(O, start, batches)
        with O.libm_flavour("brush_f64"):
            old = LC.oracle_field(O, start, batches)
        assert np.array_equal(ref.view(np.uint32), dev.view(np.uint32)), f"{name}: the device brush is glibc's expf"
        n_old = int((old.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"liquify {name}: the old (float)exp((double)x) form differs from glibc in {n_old} floats")
        assert n_old > 0


def test_perturbed_models_are_rejected_on_the_gpu_inputs():
    cases = _twist_cases()
    n = _n_diff(_outputs("device", cases, "twist"), _outputs("nudged", cases, "twist"))
    print(f"twist: results nudged on 1 % of arguments change {n} bytes")
    assert n > 0
    for name, w, h, start, batches in LC.dab_batches():
        with O.libm_flavour("device"):
            dev = LC.oracle_field(O, start, batches)
        with O.libm_flavour("nudged"):
            nud = LC.oracle_field(O, start, batches)
        assert not np.array_equal(dev.view(np.uint32), nud.view(np.uint32)), f"liquify {name}: nudged weights"
    # libm_exp without fma and with the unfused remainder: wrong only at -0x1.f8cbb2p+5 on [-104, 0] (exhaustive check above).
    # reduce_noise's centre tap weighs 1, so a weight of ~1e-28 cannot move a byte and the brush's arguments stay in
    # [-4.5, 0]: the input built to reach that argument is the call itself.
    with O.libm_flavour("device"):
        good = O.libm_eval("exp", UNFUSED_BAD_X)[0]
    assert good == O.libm_eval("exp", UNFUSED_BAD_X)[0] == np.float32(float.fromhex("0x1.f45326p-92"))
    for flavour in ("exp_nofma", "exp_unfused_r"):
        with O.libm_flavour(flavour):
            bad = O.libm_eval("exp", UNFUSED_BAD_X)[0]
        assert bad != good and bad == np.float32(float.fromhex("0x1.f45324p-92")), flavour


def test_flavour_switch_restores_and_default_is_glibc():
    assert O.lib().pfxo_get_libm() == 0
    with O.libm_flavour("device"):
        assert O.lib().pfxo_get_libm() == 1
        with O.libm_flavour("nudged"):
            assert O.lib().pfxo_get_libm() == 2
        assert O.lib().pfxo_get_libm() == 1
    assert O.lib().pfxo_get_libm() == 0
