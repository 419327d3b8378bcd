"""The script VM's f64 opcodes on the device (k_script.hip, HEAVY instantiation), through the probe of tests/vm_libm_probe.py.

- Special arguments (C99 Annex F, IEEE 754 §9.2) for every opcode: bit for bit the host interpreter's result, NaN as NaN.
- Exact results stay exact: pow(k, n) below 2^53, pow(2, n) over the whole exponent range, through pow(), `**` and `** n`; exp(0), ln(1), ...
- Accuracy against a correctly rounded referee (mpmath at 200 bits, rounded once), per function, with the distance from glibc recorded.
Both LCODE classes of the probe must give the same bits."""
import pytest

from . import vm_libm_probe as P

pytestmark = pytest.mark.gpu

# measured maxima against the referee over P.sweeps() (ulps)
ULP_BOUND = {"sin": 1, "cos": 1, "tan": 1, "exp": 1, "ln": 1, "pow": 1, "atan2": 1}


@pytest.fixture(scope="module")
def r():
    from paintfe_amd import GpuRenderer
    return GpuRenderer(0)


def device(r, probes):
    got = P.device_eval(r, probes, lcode=True)
    other = P.device_eval(r, probes, lcode=False)
    assert [P.canon(v) for v in got] == [P.canon(v) for v in other], "the two LCODE classes of the probe differ"
    return got


def test_specials_equal_host_bit_for_bit(r, record_property):
    """prescribed entries bit for bit; the ordinary values of the table (sin(2.5), pow(3, 0.5)) within the accuracy bound"""
    probes = P.specials()
    got = device(r, probes)
    host = P.host_eval(probes)
    bad, loose = [], []
    for p, d, h in zip(probes, got, host):
        if P.prescribed(p):
            if P.canon(d) != P.canon(h):
                bad.append((p, hex(d), hex(h)))
        elif P.ulps(d, P.referee(p)) > ULP_BOUND[P.FUNCTION[p[0]]]:
            loose.append((p, hex(d), hex(P.referee(p))))
    record_property("specials_differing", len(bad))
    print(f"specials: {len(bad)} of {sum(map(P.prescribed, probes))} prescribed entries differ from the host", bad[:40])
    assert not bad, f"{len(bad)} prescribed special cases differ from the host interpreter, first: {bad[:10]}"
    assert not loose, f"{len(loose)} ordinary entries beyond their ulp bound, first: {loose[:10]}"


def test_exact_results_stay_exact(r, record_property):
    probes = P.exact_cases()
    got = device(r, probes)
    bad = [(p, hex(d), hex(P.exact_value(p))) for p, d in zip(probes, got) if d != P.exact_value(p)]
    record_property("exact_differing", len(bad))
    print(f"exact: {len(bad)} of {len(probes)} differ", bad[:40])
    assert not bad, f"{len(bad)} of {len(probes)} exact cases are not exact on the device, first: {bad[:10]}"


def test_accuracy_against_correctly_rounded_referee(r, record_property):
    sweeps = P.sweeps()
    probes = [p for ps in sweeps.values() for p in ps]
    got = dict(zip(range(len(probes)), device(r, probes)))
    report, fails = {}, []
    k = 0
    for fn, ps in sweeps.items():
        ref_u, glibc_u, same = 0, 0, 0
        for p in ps:
            d = got[k]
            k += 1
            ref, gl = P.referee(p), P.glibc(p)
            u = P.ulps(d, ref)
            ref_u = max(ref_u, u)
            glibc_u = max(glibc_u, P.ulps(d, gl))
            same += d == gl
            if u > ULP_BOUND[fn]:
                fails.append((p, u, hex(d), hex(ref)))
        report[fn] = (ref_u, glibc_u, same / len(ps))
    record_property("libm_ulps", str(report))
    print("ulps (vs referee, vs glibc, share equal to glibc):", report)
    assert not fails, f"{len(fails)} probes beyond their ulp bound, first: {fails[:10]}"
