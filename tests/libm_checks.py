"""The two bars of the libm-bearing kernels, shared by tests/test_gpu_libm_model.py and tests/test_gpu_effects_edges.py: the device image
against the reference's glibc flavour (EXACT, or LIBM: +-1 on < 0.1 % of channels) and against the oracle's device flavour (tolerance 0 but
for the calls the oracle itself counts as ambiguous)."""
import numpy as np

from . import oracle_lib as O

EXACT, LIBM = "exact", "libm"


def check_glibc(got, ref, cls, what):
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    if cls == EXACT:
        assert d.max() == 0, f"{what} vs glibc: max diff {int(d.max())}, {int((d.max(-1) > 0).sum())} px differ"
    else:
        assert d.max() <= 1, f"{what} vs glibc: max diff {int(d.max())}"
        assert (d > 0).mean() < 1e-3, f"{what} vs glibc: {(d > 0).mean():.2e} of channels off by one"


def check_model(got, fn, what):
    """the device image against the device-flavour oracle; returns the oracle's ambiguous-call count"""
    with O.libm_flavour("device"):
        O.libm_reset()
        model = fn()
        amb = O.libm_ambiguous()
    d = np.abs(got.astype(np.int16) - model.astype(np.int16))
    px = int((d.max(-1) > 0).sum())
    if amb == 0:
        assert d.max() == 0, f"{what} vs device model: max diff {int(d.max())}, {px} px differ, no ambiguous call"
    else:
        assert d.max() <= 1 and px <= amb, f"{what} vs device model: max diff {int(d.max())}, {px} px differ, {amb} ambiguous calls"
    return amb
