"""Parity (GPU): the effect bank at its edges — tests/effect_cases.py, every row x size x content kind, without and with a selection, against the
CPU oracle.  What the table reaches is shown on the host by tests/test_effect_cases_host.py.

Bars: EXACT (tolerance 0, test_gpu_effects.check) for everything but twist and monochrome gaussian noise; those are held to the oracle's device
flavour at tolerance 0 with its ambiguous-call allowance (libm_checks.check_model) and keep the LIBM bar against glibc.  STATUS rows raise PfxError
and leave the destination as it was.

reduce_noise with strength +-inf / >= ~5e18 (range divisor +inf): before pfx_reduce_noise_dev routed that divisor to `/`, the kernel returned the
source image where noise.rs:236-237 gives range = x / inf = 0, the spatially blurred image.

Wall time on an MI355X: the whole file 3.5 s; the slowest test is outline (1364 cases) at 0.43 s, then oil painting 0.32 s, motion blur 0.28 s.
"""
import time

import numpy as np
import pytest

from . import effect_cases as EC
from .libm_checks import check_glibc, check_model
from .test_gpu_effects import EXACT, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    return GpuBackend(0)


@pytest.fixture(scope="module")
def oracle():
    from .backends import OracleBackend
    return OracleBackend()


def run_row(gpu, oracle, row):
    from paintfe_amd import PfxError
    n = 0
    for (w, h), kind in row.cases():
        img = EC.content(kind, w, h)
        for mask in (None, EC.selection(w, h)):
            what = f"{row.effect} {row.kw} {w}x{h} {kind} mask={mask is not None} tune={row.tune}"
            n += 1
            if row.expect == EC.STATUS:
                out = np.full_like(img, 0xA5)
                with pytest.raises(PfxError):
                    gpu.effect(row.effect, img, mask=mask, out=out, **row.kw)
                assert (out == 0xA5).all(), f"{what}: a refused call wrote to dst"
                continue
            if row.tune:
                gpu.r.tune(row.tune[0], row.tune[1])
            try:
                got = gpu.effect(row.effect, img, mask=mask, **row.kw)
            finally:
                if row.tune:
                    gpu.r.tune(row.tune[0], 1)
            if row.cls == EXACT:
                check(got, oracle.effect(row.effect, img, mask=mask, **row.kw), EXACT, what)
            else:
                call = lambda: oracle.effect(row.effect, img, mask=mask, **row.kw)   # noqa: E731
                check_glibc(got, call(), row.cls, what)
                check_model(got, call, what)
    return n


@pytest.mark.parametrize("effect", EC.EFFECTS)
def test_effect_edges_vs_oracle(gpu, oracle, effect):
    t0 = time.perf_counter()
    rows = EC.rows(effect)
    assert rows
    n = sum(run_row(gpu, oracle, row) for row in rows)
    print(f"{effect}: {len(rows)} rows, {n} cases, {time.perf_counter() - t0:.2f} s")


def test_reduce_noise_with_an_overflowing_range_divisor_is_the_spatial_blur(gpu, oracle):
    """2 * (strength * 2.55)^2 + 0.001 = +inf from strength ~5.1e18 up: range = x / inf = 0 (noise.rs:236-237), every weight exp(-spatial), and the result
    differs from the source; the last finite divisors below it still take the shared reciprocal or `/` to the same bits"""
    img = EC.content("noise", 40, 24)
    for strength in (float("inf"), float("-inf"), 1e19, 5.2e18, 5.0e18, 1e15, 1e12):
        want = oracle.effect("reduce_noise", img, strength=strength, radius=2)
        check(gpu.effect("reduce_noise", img, strength=strength, radius=2), want, EXACT, f"reduce_noise strength {strength}")
        assert (want != img).any(-1).mean() > 0.9
    blur = oracle.effect("reduce_noise", img, strength=float("inf"), radius=2)
    assert np.array_equal(oracle.effect("reduce_noise", img, strength=1e19, radius=2), blur)


@pytest.mark.parametrize("num_exp,den_exp", [((-100, 20), (-48, 20)), ((0, 17), (-10, 100))], ids=["documented", "reduce_noise"])
def test_fast_division_matches_ieee_over_its_stated_ranges(gpu, num_exp, den_exp):
    """k_common.h:rdiv vs the compiler's IEEE divide on 2^28 random pairs: the range k_common.h documents (numerators 2^-100 .. 2^20 or 0,
    denominators 2^-48 .. 2^20) and reduce_noise's (integers <= 195075 over range divisors 0.001 .. 2^100, pfx_reduce_noise_dev).
    Measured on an MI355X: 0 mismatches in both, under 0.01 s a run; with reduce_noise's numerators the first mismatches appear at denominator
    exponents 126 .. 127 (2.0e8 of 2^28: the reciprocal is subnormal there), none at 101 .. 125, so the switch to `/` at 2^100 has room"""
    t0 = time.perf_counter()
    bad = gpu.r.selftest_division_range(seed=0xD1D2, n_millions=268, num_exp=num_exp, den_exp=den_exp)
    print(f"division self-test {num_exp} / {den_exp}: {bad} mismatches, {time.perf_counter() - t0:.2f} s")
    assert bad == 0


def test_division_selftest_refuses_exponents_outside_the_normal_range(gpu):
    from paintfe_amd import PfxError
    for num_exp, den_exp in (((-127, 0), (0, 0)), ((0, 128), (0, 0)), ((3, 2), (0, 0)), ((0, 0), (-200, 0)), ((0, 0), (5, 4))):
        with pytest.raises(PfxError):
            gpu.r.selftest_division_range(seed=1, n_millions=1, num_exp=num_exp, den_exp=den_exp)
