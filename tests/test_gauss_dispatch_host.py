"""Which Gaussian kernel runs for a call, and what rides in its store: the one host-side decision (pfx_gauss.cpp), which is exported as the
test seam pfx_int_gauss_path (pfx_internal.h), against a table written out here from the rules.  No device: the decision is a pure function.

The rules, as the entry points have always applied them:
  * radius beyond pfxk_gauss_max_radius(): unsupported;
  * default mode, radius in 1 .. pfxk_gauss_mfma_max_radius(), src != dst: the matrix-core strips;
  * bit-exact mode, radius in 1 .. pfxk_gauss_fused_exact_max_radius(), fused path enabled, src != dst: the fused LDS-ring kernel;
  * otherwise the two passes gauss_h / gauss_v;
  * sharpen / glow ride in the fused bit-exact kernel's store only when the buffers share no byte; otherwise the blur goes into scratch of the context
    (never in place) by the rules above and the combine is its own launch;
  * a pointwise chain rides in the fused bit-exact kernel's store, or (default mode, no table, pfx_tune "chain_mfma" on) in the matrix-core kernel's; a chain
    with an HSL / vibrance op only with pfx_tune "chain_fuse_heavy"; otherwise the blur by the rules above and the chain behind it;
  * the drop shadow's plane form: w % 4 == 0, pfx_tune "shadow_plane" on, "gauss_fast_effects" off, radius 0 (no blur) or in the fused range; it is keyed
    on the knob and not on the mode, unlike sharpen / glow; otherwise the RGBA image is blurred into scratch by the rules above.

The radii limits are queried, so the table is written per radius CLASS; a kernel that widens a range moves radii between columns and every site must follow."""
import ctypes as C

import pytest

from paintfe_amd import _lib

PLAIN, SHARPEN, GLOW, CHAIN, PLANE = range(5)                       # pfx_internal.h: PFX_GAUSS_PLAIN ..
PATHS = {"U": -1, "M": 0, "F": 1, "T": 2, "m": 3, "f": 4, "P": 5}   # unsupported, mfma, fused, two-pass, mfma + rider, fused + rider, plane

# one letter per radius class:   r < 1 | in both ranges | fused range only | mfma range only | in neither, <= max | beyond max
COLS = ("zero", "both", "fused", "mfma", "neither", "beyond")
# (case, exact) -> a row per aliasing: D distinct, S src == dst, O partial overlap
TABLE = {
    ("plain", 0):          {"D": "TMTMTU", "S": "TTTTTU", "O": "TMTMTU"},   # partial overlap is the entry point's to refuse: only src == dst counts
    ("plain", 1):          {"D": "TFFTTU", "S": "TTTTTU", "O": "TFFTTU"},
    ("sharpen", 0):        {"D": "TMTMTU", "S": "TMTMTU", "O": "TMTMTU"},   # never rides; the blur goes into scratch: src == dst does not make it in place
    ("sharpen", 1):        {"D": "TffTTU", "S": "TFFTTU", "O": "TFFTTU"},
    ("chain", 0):          {"D": "TmTmTU", "S": "TmTmTU", "O": "TmTmTU"},   # pfx_chain_dev refuses a blur in place: the ride does not look at aliasing
    ("chain", 1):          {"D": "TffTTU", "S": "TffTTU", "O": "TffTTU"},
    ("chain_lut", 0):      {"D": "TMTMTU", "S": "TTTTTU", "O": "TMTMTU"},
    ("chain_lut", 1):      {"D": "TffTTU", "S": "TffTTU", "O": "TffTTU"},
    ("chain_mfma_off", 0): {"D": "TMTMTU", "S": "TTTTTU", "O": "TMTMTU"},
    ("chain_mfma_off", 1): {"D": "TffTTU", "S": "TffTTU", "O": "TffTTU"},
    ("plane_w4", 0):       {"D": "PPPMTU", "S": "PPPMTU", "O": "PPPMTU"},   # the plane's buffers are the context's own: aliasing does not enter
    ("plane_w4", 1):       {"D": "PPPTTU", "S": "PPPTTU", "O": "PPPTTU"},
    ("plane_w5", 0):       {"D": "TMTMTU", "S": "TMTMTU", "O": "TMTMTU"},
    ("plane_w5", 1):       {"D": "TFFTTU", "S": "TFFTTU", "O": "TFFTTU"},
}
# case -> (ride, n_luts, chain_mfma, w); heavy = fuse_heavy = 0, shadow_plane = 1, fast_effects = 0
CASES = {"plain": (PLAIN, 0, 1, 64), "sharpen": (SHARPEN, 0, 1, 64), "chain": (CHAIN, 0, 1, 64), "chain_lut": (CHAIN, 1, 1, 64),
         "chain_mfma_off": (CHAIN, 0, 0, 64), "plane_w4": (PLANE, 0, 1, 64), "plane_w5": (PLANE, 0, 1, 65)}
ALIAS = {"D": (0, 0), "S": (1, 1), "O": (0, 1)}   # (src == dst, share a byte)


class GaussCase(C.Structure):   # pfx_internal.h: pfx_gauss_case
    _fields_ = [("exact", C.c_int), ("radius", C.c_int), ("same", C.c_int), ("overlap", C.c_int), ("ride", C.c_int), ("n_luts", C.c_uint32),
                ("chain_mfma", C.c_int), ("heavy", C.c_int), ("fuse_heavy", C.c_int), ("w", C.c_uint32), ("shadow_plane", C.c_int),
                ("fast_effects", C.c_int), ("fused_enabled", C.c_int)]


@pytest.fixture(scope="module")
def lib():
    L = _lib.load()
    L.pfx_int_gauss_path.argtypes = [C.POINTER(GaussCase)]
    L.pfx_int_gauss_path.restype = C.c_int
    for f in ("pfxk_gauss_max_radius", "pfxk_gauss_mfma_max_radius", "pfxk_gauss_fused_exact_max_radius", "pfxk_gauss_fused_exact_enabled"):
        getattr(L, f).argtypes = []
        getattr(L, f).restype = C.c_int
    return L


def path(lib, exact, radius, alias, ride, n_luts=0, chain_mfma=1, heavy=0, fuse_heavy=0, w=64, shadow_plane=1, fast_effects=0, fused_enabled=1):
    same, overlap = ALIAS[alias]
    c = GaussCase(exact, radius, same, overlap, ride, n_luts, chain_mfma, heavy, fuse_heavy, w, shadow_plane, fast_effects, fused_enabled)
    return lib.pfx_int_gauss_path(C.byref(c))


def limits(lib):
    return lib.pfxk_gauss_fused_exact_max_radius(), lib.pfxk_gauss_mfma_max_radius(), lib.pfxk_gauss_max_radius()


def column(lib, radius, fused_enabled):
    fused_max, mfma_max, max_r = limits(lib)
    if radius > max_r:
        return "beyond"
    if radius < 1:
        return "zero"
    in_fused = bool(fused_enabled) and radius <= fused_max   # the fused path switched off: no radius is in its range
    in_mfma = radius <= mfma_max
    return {(True, True): "both", (True, False): "fused", (False, True): "mfma", (False, False): "neither"}[(in_fused, in_mfma)]


def test_limits_are_sane_and_the_knob_is_not_the_limit(lib):
    fused_max, mfma_max, max_r = limits(lib)
    assert 1 <= fused_max <= max_r and 1 <= mfma_max <= max_r
    assert lib.pfxk_gauss_fused_exact_enabled() == 1
    lib.pfxk_gauss_set_fused_exact(0)   # pfx_tune "gauss_fused_exact" = 0 (process-wide; restored below)
    try:
        assert lib.pfxk_gauss_fused_exact_enabled() == 0
        assert lib.pfxk_gauss_fused_exact_max_radius() == fused_max, "the compiled limit does not move with the knob"
    finally:
        lib.pfxk_gauss_set_fused_exact(1)
    assert lib.pfxk_gauss_fused_exact_enabled() == 1


@pytest.mark.parametrize("fused_enabled", [1, 0])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_path_table(lib, case, exact, fused_enabled):
    fused_max, mfma_max, max_r = limits(lib)
    radii = sorted({0, 1, 16, 17, 48, 49, fused_max, fused_max + 1, mfma_max, mfma_max + 1, max_r, max_r + 1})
    ride, n_luts, chain_mfma, w = CASES[case]
    rides = (SHARPEN, GLOW) if ride == SHARPEN else (ride,)   # glow follows sharpen's row
    seen = set()
    for alias, row in TABLE[(case, exact)].items():
        for radius in radii:
            col = column(lib, radius, fused_enabled)
            seen.add(col)
            want = PATHS[row[COLS.index(col)]]
            for rd in rides:
                got = path(lib, exact, radius, alias, rd, n_luts=n_luts, chain_mfma=chain_mfma, w=w, fused_enabled=fused_enabled)
                assert got == want, (case, exact, fused_enabled, alias, radius, col, rd, got, want)
    assert {"zero", "neither", "beyond"} <= seen and ("both" in seen or "mfma" in seen)


def test_heavy_chain_rides_only_with_chain_fuse_heavy(lib):
    for exact, alone, riding in ((0, "M", "m"), (1, "F", "f")):
        assert path(lib, exact, 1, "D", CHAIN, heavy=1, fuse_heavy=0) == PATHS[alone]
        assert path(lib, exact, 1, "D", CHAIN, heavy=1, fuse_heavy=1) == PATHS[riding]
        assert path(lib, exact, 1, "D", CHAIN, heavy=0, fuse_heavy=0) == PATHS[riding]
    assert path(lib, 0, 1, "D", CHAIN, heavy=1, fuse_heavy=1, n_luts=1) == PATHS["M"]       # a table still keeps the chain out of the matrix-core store
    assert path(lib, 0, 1, "D", CHAIN, heavy=1, fuse_heavy=1, chain_mfma=0) == PATHS["M"]


def test_plane_form_follows_its_knobs_not_the_mode(lib):
    assert path(lib, 1, 1, "D", PLANE) == PATHS["P"]
    assert path(lib, 1, 1, "D", PLANE, shadow_plane=0) == PATHS["F"]
    # gauss_fast_effects = 1 on a bit-exact context: the shadow blurs its RGBA image (with the fused kernel) while sharpen / glow still fuse their combine
    assert path(lib, 1, 1, "D", PLANE, fast_effects=1) == PATHS["F"]
    assert path(lib, 1, 1, "D", SHARPEN, fast_effects=1) == PATHS["f"]
    assert path(lib, 0, 1, "D", PLANE, fast_effects=1) == PATHS["M"]
    assert path(lib, 1, 0, "D", PLANE, fused_enabled=0) == PATHS["P"]    # no blur at all: the plane layout alone
    assert path(lib, 1, 1, "D", PLANE, fused_enabled=0) == PATHS["T"]
