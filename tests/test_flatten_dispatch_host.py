"""Which compositor kernel runs for a call and in what shape: the host-side decisions of pfx_flatten.cpp, exported as the test seams pfx_int_flatten_plan,
pfx_int_flatten_cands and pfx_int_flatten_verdict (pfx_internal.h), against tables written out here from the rules.  No device: all three are pure functions.

The plan, the first rule that matches (n = descriptors, n_px = w * h; the knobs under their pfx_tune names):
  * a preview or a dirty rectangle forces GENERAL.  GENERAL, an opacity off the fast division, n = 0, n_px >= 2^30 or "flatten_variant" 9: the template
    flatten_kernel<GENERAL, F>, one lane per 4 pixels (a rectangle: per 4 pixels of each of its rows), workgroups of 256, at most 8192 of them;
  * candidates present and flatten_variant != 8: an elimination kernel — class sorting when "dle_kernel" is 0 and the device's UNORM8 conversions are verified,
    else round 3's.  "dle_cfg" 1: 2 pixels per lane (round 3: 3 register sets, ring 2^9), 2: 3 pixels (round 3: 3 sets, ring 2^10), else 3 pixels (round 3: 2 sets,
    ring 2^10); "dle_stats" bit 2, else bit 1, picks a diagnostic build of the class-sorting kernel, which exists with 3 pixels per lane only.
    Units of 64 * pixels-per-lane pixels; a wave owns at most umax = 65535 // unit of them (16-bit offsets: 341 of 192 px, 511 of 128).
    "dle_sched" 0: every wave min(dle_units or 8, umax) units.  Otherwise A = units * dle_frac_a // 100 units go to long streams of UA units, B = units *
    dle_frac_b // 100 to streams of UB = max(UA // 4, 1), the rest one unit a wave; UA = min(dle_units, umax) when set, else ceil(A / 6144) — the long streams fill
    the chip about once — held to 1 .. 8 for the class-sorting kernel and to 4 or more for round 3's.  waves = A // UA + B // UB + units not covered by those.
    Class sorting: re-deal attempts from layer s1 = topmost candidate + (dle_s1 if > 0 else 1), every seg = dle_s2 layers (-1: 3; 0: 1000, one attempt);
    dle_s1 0: seg 0, never;
  * otherwise the streaming kernel.  flatten_variant 1 .. 6: 2x2, 2x3, 4x2, 4x3, 1x3, 3x3 pixels per lane x register sets, one 64 * PX tile per wave; +10: the
    same with a grid stride; any other value 3x3.  0 (and 8): 2x2 with a grid stride up to 16 layers; from 5 layers on 4x2 for light stacks (mode class 2; grid
    stride below 7 layers) and medium ones (class 1; always grid stride).  Workgroups of four waves, at most 8192 with a grid stride, else at most 2^20.
    The path word carries the chunk-start flag.
Candidates: unmasked raster layers above the bottom one that are Overwrite, or Normal at opacity >= 1; the topmost min(PFXK_DLE_MAX, max(1, n // 6)) are kept.
Below "dle_min_layers" they are dropped, or kept with `shallow` set when the caller decides per stack ("dle_adaptive").
Verdict for a shallow stack (probe state 0 none, 1 pending, 2 pays, 3 does not): not usable: nothing; probed stack is another one: probe now, no candidates;
the same stack: candidates only in state 2."""
import ctypes as C
import itertools

import pytest

from paintfe_amd import _lib

TEMPLATE, STREAM, DLE, SRT = range(4)   # pfx_kernels.h: PFXK_FLATTEN_*
GENERAL, FAST, REGION, PREVIEW, CHUNK_START = (1 << b for b in range(4, 9))
DLE_MAX = 4                             # PFXK_DLE_MAX
OVERWRITE, NORMAL, MULTIPLY = 14, 0, 1
KNOBS = dict(variant=0, units=0, cfg=0, sched=1, fracA=75, fracB=20, kernel=0, s1=-1, s2=-1, stats=0)   # pfx_flatten.cpp: the defaults


class FlattenCase(C.Structure):   # pfx_internal.h: pfx_flatten_case
    _fields_ = [("n_desc", C.c_int), ("w", C.c_uint32), ("h", C.c_uint32), ("general", C.c_int), ("has_preview", C.c_int), ("rw", C.c_uint32), ("rh", C.c_uint32)] + \
               [(n, C.c_int) for n in ("fast_div", "mode_class", "n_cands", "cand_top", "unorm_ok", "chunk_start") + tuple(KNOBS)]


class Sched(C.Structure):   # pfx_kernels.h: pfxk_dle_sched
    _fields_ = [(n, C.c_uint32) for n in ("wavesA", "UA", "wavesB", "UB", "UC")]


class Redeal(C.Structure):   # pfx_kernels.h: pfxk_dle_plan
    _fields_ = [("s1", C.c_uint32), ("seg", C.c_uint32)]


class FlattenPlan(C.Structure):   # pfx_kernels.h: pfxk_flatten_plan
    _fields_ = [(n, C.c_int) for n in ("kernel", "path", "general", "fast_div", "px", "nb", "ring", "diag")] + \
               [(n, C.c_uint32) for n in ("grid", "waves", "stats")] + [("sched", Sched), ("redeal", Redeal)]

    def as_tuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_[:11]) + tuple(getattr(self.sched, n) for n, _ in Sched._fields_) + (self.redeal.s1, self.redeal.seg)


class Cands(C.Structure):   # pfx_kernels.h: pfxk_dle_cands
    _fields_ = [("n", C.c_uint32), ("layer", C.c_uint32 * DLE_MAX), ("kind", C.c_uint32 * DLE_MAX), ("stats", C.c_uint32)]


def bind(L):
    L.pfx_int_flatten_plan.argtypes = [C.POINTER(FlattenCase), C.POINTER(FlattenPlan)]
    L.pfx_int_flatten_plan.restype = C.c_int
    L.pfx_int_flatten_cands.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint32, C.c_int, C.c_int, C.POINTER(Cands), C.POINTER(C.c_int)]
    L.pfx_int_flatten_cands.restype = C.c_int
    L.pfx_int_flatten_verdict.argtypes = [C.c_int] * 3
    L.pfx_int_flatten_verdict.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def lib():
    return bind(_lib.load())


def plan(lib, n_desc=9, w=257, h=130, **kw):
    """the plan of a plain call (raster-only, fast division, whole frame, no candidates, default knobs) with the given fields changed"""
    f = dict(KNOBS, n_desc=n_desc, w=w, h=h, fast_div=1, unorm_ok=1)
    assert set(kw) <= {n for n, _ in FlattenCase._fields_}, kw
    f.update(kw)
    c, p = FlattenCase(**f), FlattenPlan()
    assert lib.pfx_int_flatten_plan(C.byref(c), C.byref(p)) == p.kernel == p.path & 0xF
    return p


def cands(lib, layers, min_layers=0, adaptive=0):
    """layers: (mode or -1 for an adjustment layer, opacity, masked) bottom -> top; returns ([(position, kind)], shallow)"""
    n = len(layers)
    out, shallow = Cands(), C.c_int(-1)
    got = lib.pfx_int_flatten_cands((C.c_int * n)(*[m for m, _, _ in layers]), (C.c_float * n)(*[o for _, o, _ in layers]), (C.c_uint8 * n)(*[int(k) for _, _, k in layers]),
                                    n, min_layers, adaptive, C.byref(out), C.byref(shallow))
    assert got == out.n <= DLE_MAX and out.stats == 0
    return [(out.layer[k], out.kind[k]) for k in range(out.n)], shallow.value


# ------------------------------------------------------------------------------------------------------------------------------- the template kernel
def test_template_kernel_corners_and_what_forces_general(lib):
    for general, fast in itertools.product((0, 1), (0, 1)):
        if general == 0 and fast == 1:
            continue   # the plain call: below
        p = plan(lib, general=general, fast_div=fast)
        assert (p.kernel, p.general, p.fast_div, p.path) == (TEMPLATE, general, fast, (GENERAL if general else 0) | (FAST if fast else 0)), (general, fast)
    for why in (dict(n_desc=0), dict(variant=9), dict(w=1 << 15, h=1 << 15)):
        p = plan(lib, **why)
        assert (p.kernel, p.general, p.fast_div, p.path) == (TEMPLATE, 0, 1, FAST), why
    assert plan(lib, w=1 << 15, h=(1 << 15) - 1).kernel == STREAM   # 2^30 - 2^15 pixels
    for fast in (0, 1):
        p = plan(lib, has_preview=1, fast_div=fast)
        assert (p.kernel, p.general, p.fast_div, p.path) == (TEMPLATE, 1, fast, GENERAL | PREVIEW | (FAST if fast else 0))
        p = plan(lib, rw=5, rh=3, fast_div=fast)
        assert (p.kernel, p.general, p.fast_div, p.path) == (TEMPLATE, 1, fast, GENERAL | REGION | (FAST if fast else 0))
    assert plan(lib, rw=5, rh=3, has_preview=1, general=1).path == GENERAL | REGION | PREVIEW | FAST
    assert plan(lib, rw=5, rh=0).kernel == STREAM   # 0 x 0 (either side): the whole canvas
    # candidates, the chunk table and every knob but variant 9 leave a template launch alone
    base = plan(lib, general=1).as_tuple()
    assert plan(lib, general=1, n_cands=2, cand_top=5, chunk_start=1, variant=3, units=5, cfg=1, sched=0, kernel=1, s1=2, s2=2, stats=7).as_tuple() == base


def test_template_kernel_grid(lib):
    # whole canvas: ceil(ceil(n_px / 4) / 256), at most 8192
    for (w, h), grid in {(1, 1): 1, (67, 66): 5, (257, 130): 33, (1024, 1024): 1024, (2896, 2896): 8191, (2897, 2896): 8192, (4096, 4096): 8192, (1 << 15, 1 << 15): 8192}.items():
        assert plan(lib, w=w, h=h, general=1).grid == grid, (w, h)
        assert plan(lib, w=w, h=h, fast_div=0).grid == grid, (w, h)
    # a rectangle: ceil(rw / 4) * rh quads, whatever the canvas
    for (rw, rh), grid in {(1, 1): 1, (5, 3): 1, (67, 66): 5, (4097, 300): 1202, (8192, 1024): 8192, (8188, 1024): 8188, (8189, 1024): 8192}.items():
        assert plan(lib, w=8192, h=4320, rw=rw, rh=rh).grid == grid, (rw, rh)


# ------------------------------------------------------------------------------------------------------------------------------ the streaming kernel
BIG = (8192, 4320)            # 35 389 440 pixels: tiles of 64 / 128 / 192 / 256 -> 138240 / 69120 / 46080 / 34560 workgroups, or 8192 with a grid stride
BIG_GRID = {1: 138240, 2: 69120, 3: 46080, 4: 34560}
# flatten_variant 0 by mode class and depth: (PX, NB, grid stride)
S = {"2s": (2, 2, True), "2t": (2, 2, False), "4s": (4, 2, True), "4t": (4, 2, False)}
DEFAULT_SHAPE = {  # depth:  1     4     5     6     7     16    17
    0: dict(zip((1, 4, 5, 6, 7, 16, 17), ("2s", "2s", "2s", "2s", "2s", "2s", "2t"))),   # heavy
    1: dict(zip((1, 4, 5, 6, 7, 16, 17), ("2s", "2s", "4s", "4s", "4s", "4s", "4s"))),   # medium
    2: dict(zip((1, 4, 5, 6, 7, 16, 17), ("2s", "2s", "4s", "4s", "4t", "4t", "4t"))),   # light
}
VARIANT_SHAPE = {1: (2, 2), 2: (2, 3), 3: (4, 2), 4: (4, 3), 5: (1, 3), 6: (3, 3), 7: (3, 3), 10: (3, 3), 17: (3, 3), 18: (3, 3), 19: (3, 3), -1: (3, 3), 25: (1, 3)}


def stream_shape(p):
    assert p.kernel == STREAM and p.path & ~CHUNK_START == STREAM | FAST and (p.general, p.fast_div, p.ring, p.diag, p.waves) == (0, 1, 0, 0, 0)
    assert p.grid in (8192, BIG_GRID[p.px]), (p.px, p.grid)
    return p.px, p.nb, p.grid == 8192


def test_streaming_kernel_default_shape_by_mode_class_and_depth(lib):
    seen = set()
    for cls, row in DEFAULT_SHAPE.items():
        for depth, key in row.items():
            for variant, n_cands in ((0, 0), (8, 0), (8, 3)):   # variant 8: the same shape, candidates or not
                assert stream_shape(plan(lib, depth, *BIG, mode_class=cls, variant=variant, n_cands=n_cands, cand_top=depth - 1)) == S[key], (cls, depth, variant)
            seen.add(S[key])
    assert seen == set(S.values())


def test_streaming_kernel_variants(lib):
    for variant, (px, nb) in VARIANT_SHAPE.items():
        for depth, cls in itertools.product((1, 9, 17), (0, 2)):
            assert stream_shape(plan(lib, depth, *BIG, mode_class=cls, variant=variant)) == (px, nb, variant >= 10), (variant, depth, cls)
    for variant in range(1, 7):
        assert stream_shape(plan(lib, 9, *BIG, variant=variant + 10)) == VARIANT_SHAPE[variant] + (True,), variant


def test_streaming_kernel_grid_under_both_caps_and_chunk_start_flag(lib):
    # four waves a workgroup, a wave a 64 * PX tile: ceil(ceil(n_px / (64 PX)) / 4)
    for (w, h), variant, grid in (((1, 1), 1, 1), ((67, 66), 1, 9), ((67, 66), 3, 5), ((67, 66), 5, 18), ((257, 130), 1, 66), ((257, 130), 6, 44), ((257, 130), 16, 44),
                                  ((2048, 1024), 1, 4096), ((2048, 1024), 11, 4096), ((2048, 1025), 11, 4100), ((4096, 1024), 11, 8192), ((4096, 1024), 1, 8192), ((4096, 1025), 1, 8200),
                                  ((4096, 1025), 11, 8192), ((1 << 15, 1 << 13), 5, 1 << 20), ((1 << 15, (1 << 13) + 1), 5, 1 << 20), ((1 << 15, (1 << 13) - 1), 5, (1 << 20) - 128),
                                  ((1 << 15, 1 << 14), 15, 8192)):
        assert plan(lib, w=w, h=h, variant=variant).grid == grid, (w, h, variant)
    for chunk_start in (0, 1):
        assert plan(lib, chunk_start=chunk_start).path == STREAM | FAST | (CHUNK_START if chunk_start else 0)


# --------------------------------------------------------------------------------------------------------------------------- the elimination kernels
def elim(lib, **kw):
    kw.setdefault("n_desc", 17), kw.setdefault("n_cands", 1), kw.setdefault("cand_top", 14)
    return plan(lib, **kw)


def sched_model(n_px, srt, cfg=0, sched=1, units=0, fracA=75, fracB=20):
    """the docstring's schedule rule: (wavesA, UA, wavesB, UB, UC, waves)"""
    unit = 64 * (2 if cfg == 1 else 3)
    n_units, umax = -(-n_px // unit), 65535 // unit
    if sched == 0:
        u = min(units or 8, umax)
        return (-(-n_units // u), u, 0, u, u, -(-n_units // u))
    a, b = n_units * fracA // 100, n_units * fracB // 100
    fill = -(-a // 6144)
    ua = min(units or (min(max(fill, 1), 8) if srt else max(fill, 4)), umax)
    ub = max(ua // 4, 1)
    wa, wb = a // ua, b // ub
    return (wa, ua, wb, ub, 1, wa + wb + n_units - min(n_units, wa * ua + wb * ub))


def sched_of(p):
    return (p.sched.wavesA, p.sched.UA, p.sched.wavesB, p.sched.UB, p.sched.UC, p.waves)


def test_elimination_kernel_choice_and_shape(lib):
    # (dle_kernel, unorm_ok, dle_cfg) -> kernel, PX, NB, ring
    table = {(0, 1, 0): (SRT, 3, 0, 0), (0, 1, 1): (SRT, 2, 0, 0), (0, 1, 2): (SRT, 3, 0, 0), (0, 1, 5): (SRT, 3, 0, 0),
             (0, 0, 0): (DLE, 3, 2, 10), (0, 0, 1): (DLE, 2, 3, 9), (0, 0, 2): (DLE, 3, 3, 10), (0, 0, 5): (DLE, 3, 2, 10),
             (1, 1, 0): (DLE, 3, 2, 10), (1, 1, 1): (DLE, 2, 3, 9), (1, 1, 2): (DLE, 3, 3, 10), (1, 0, 0): (DLE, 3, 2, 10), (1, 0, 1): (DLE, 2, 3, 9), (1, 0, 2): (DLE, 3, 3, 10)}
    for (kernel, unorm_ok, cfg), (k, px, nb, ring) in table.items():
        for n_desc, cls, variant in ((2, 0, 0), (17, 2, 0), (32, 1, 3), (32, 0, 14)):   # depth, mode class and the streaming variants do not matter
            p = elim(lib, n_desc=n_desc, cand_top=1, mode_class=cls, variant=variant, kernel=kernel, unorm_ok=unorm_ok, cfg=cfg)
            assert (p.kernel, p.px, p.nb, p.ring, p.diag, p.path, p.grid) == (k, px, nb, ring, 0, k | FAST, 0), (kernel, unorm_ok, cfg)
    assert elim(lib, variant=8).kernel == STREAM and elim(lib, variant=9).kernel == TEMPLATE and elim(lib, n_cands=0).kernel == STREAM
    assert elim(lib, fast_div=0).kernel == elim(lib, general=1).kernel == elim(lib, rw=4, rh=4).kernel == elim(lib, has_preview=1).kernel == TEMPLATE


def test_diagnostic_arms_follow_the_stats_bits(lib):
    for stats, diag in {0: 0, 1: 0, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 4, 8: 0}.items():
        for cfg in (0, 1):
            p = elim(lib, stats=stats, cfg=cfg)
            assert (p.kernel, p.diag, p.stats, p.px) == (SRT, diag, stats, 3 if diag or cfg == 0 else 2), (stats, cfg)
            assert sched_of(p) == sched_model(257 * 130, True, cfg), (stats, cfg)   # the schedule counts dle_cfg's units whatever the build
        p = elim(lib, stats=stats, kernel=1)
        assert (p.kernel, p.diag, p.stats) == (DLE, 0, stats)


def test_schedule_written_out(lib):
    # 7680 x 4320 in 192-pixel units: 172800; A = 129600, B = 34560; ceil(A / 6144) = 22
    assert sched_of(elim(lib, w=7680, h=4320)) == (16200, 8, 17280, 2, 1, 16200 + 17280 + 8640)                     # class sorting: at most 8
    assert sched_of(elim(lib, w=7680, h=4320, kernel=1)) == (5890, 22, 6912, 5, 1, 5890 + 6912 + 8660)              # round 3: the fill rule
    assert sched_of(elim(lib, w=7680, h=4320, sched=0)) == (21600, 8, 0, 8, 8, 21600)
    assert sched_of(elim(lib, w=7680, h=4320, sched=0, units=340)) == (509, 340, 0, 340, 340, 509)
    assert sched_of(elim(lib, w=7680, h=4320, units=340)) == (381, 340, 406, 85, 1, 381 + 406 + (172800 - 381 * 340 - 406 * 85))
    # 67 x 66 = 4422 pixels: 24 units of 192, 35 of 128
    assert sched_of(elim(lib, w=67, h=66)) == (18, 1, 4, 1, 1, 24)
    assert sched_of(elim(lib, w=67, h=66, kernel=1)) == (4, 4, 4, 1, 1, 4 + 4 + 4)
    assert sched_of(elim(lib, w=67, h=66, cfg=1)) == (26, 1, 7, 1, 1, 35)
    assert sched_of(elim(lib, w=67, h=66, units=340)) == (0, 340, 0, 85, 1, 24)
    # the 16-bit clamp: 341 units of 192 pixels, 511 of 128
    assert [elim(lib, units=u, sched=s, cfg=c).sched.UA for u, s, c in itertools.product((341, 342, 1000), (0, 1), (0, 2))] == [341] * 12
    assert [elim(lib, units=u, sched=s, cfg=1).sched.UA for u, s in itertools.product((340, 511, 512, 1000), (0, 1))] == [340, 340, 511, 511, 511, 511, 511, 511]


def test_schedule_against_the_rule_and_every_unit_is_covered(lib):
    sizes = [(67, 66), (257, 130), (1, 1), (192, 1), (193, 1), (7680, 4320), (7680, 64),
             (1536, 1024), (8193, 192), (8194, 192),            # A = 6144 (one unit a long stream), 6144 still, 6145 (two)
             (3072, 1024), (16385, 192), (16386, 192),          # A = 12288 (two), 12288 still, 12289 (three)
             (12288, 1024), (65539, 192),                       # A = 49152 (8), 49154 (9: the class-sorting kernel stays at 8)
             (1 << 15, (1 << 15) - 1)]
    uas = set()
    for (w, h), kernel, cfg, sched, units, (fracA, fracB) in itertools.product(sizes, (0, 1), (0, 1, 2), (0, 1), (0, 1, 8, 340), ((75, 20), (100, 0), (0, 100), (0, 0), (50, 50), (33, 9))):
        p = elim(lib, w=w, h=h, kernel=kernel, cfg=cfg, sched=sched, units=units, fracA=fracA, fracB=fracB)
        what = (w, h, kernel, cfg, sched, units, fracA, fracB)
        assert sched_of(p) == sched_model(w * h, kernel == 0, cfg, sched, units, fracA, fracB), what
        n_units = -(-w * h // (64 * (2 if cfg == 1 else 3)))
        sc = p.sched
        assert p.waves >= 1 and sc.wavesA * sc.UA + sc.wavesB * sc.UB + (p.waves - sc.wavesA - sc.wavesB) * sc.UC >= n_units, what
        assert (p.waves - 1 - sc.wavesA - sc.wavesB) * sc.UC < n_units, what   # and no wave beyond the last unit's
        if units == 0 and sched == 1 and (fracA, cfg) == (75, 0):
            uas.add((w, h, kernel, sc.UA))
    fill = {(1536, 1024): 1, (8193, 192): 1, (8194, 192): 2, (3072, 1024): 2, (16385, 192): 2, (16386, 192): 3, (12288, 1024): 8, (65539, 192): 9}
    for (w, h), ua in fill.items():
        assert (w, h, 0, min(ua, 8)) in uas and (w, h, 1, max(ua, 4)) in uas, (w, h)


def test_redeal_plan(lib):
    for (s1, s2), (first, seg) in {(-1, -1): (1, 3), (-1, 0): (1, 1000), (-1, 1): (1, 1), (-1, 3): (1, 3), (0, -1): (1, 0), (0, 0): (1, 0), (0, 1): (1, 0), (0, 3): (1, 0),
                                   (1, -1): (1, 3), (1, 0): (1, 1000), (1, 1): (1, 1), (1, 3): (1, 3), (3, -1): (3, 3), (3, 0): (3, 1000), (3, 1): (3, 1), (3, 3): (3, 3)}.items():
        for top in (1, 14, 31):
            p = elim(lib, n_desc=32, cand_top=top, s1=s1, s2=s2)
            assert (p.kernel, p.redeal.s1, p.redeal.seg) == (SRT, top + first, seg), (s1, s2, top)
    p = elim(lib, kernel=1, s1=3, s2=3)
    assert (p.kernel, p.redeal.s1, p.redeal.seg) == (DLE, 0, 0)   # round 3's kernel has no re-deal


# ------------------------------------------------------------------------------------------------------------------------------------- candidates
def test_candidates(lib):
    N, O, M = (NORMAL, 1.0, 0), (OVERWRITE, 0.25, 0), (MULTIPLY, 1.0, 0)
    assert cands(lib, []) == ([], 0) and cands(lib, [O]) == ([], 0)                     # the bottom layer never counts
    assert cands(lib, [N, O]) == ([(1, 0)], 0) and cands(lib, [O, N]) == ([(1, 1)], 0)   # kind 0 Overwrite, 1 Normal
    for opacity, ok in ((1.0, True), (1.5, True), (float("inf"), True), (0.99999994, False), (0.0, False), (-1.0, False), (float("nan"), False)):
        assert cands(lib, [M, (NORMAL, opacity, 0)]) == ([(1, 1)] if ok else [], 0), opacity
        assert cands(lib, [M, (OVERWRITE, opacity, 0)]) == ([(1, 0)], 0), opacity       # Overwrite at any opacity
    assert cands(lib, [M, (NORMAL, 1.0, 1), (OVERWRITE, 1.0, 1), (-1, 1.0, 0), M, (13, 1.0, 0)]) == ([], 0)   # masked, adjustment, other modes
    # the topmost min(4, max(1, n // 6)) of them
    for n in (2, 5, 6, 11, 12, 17, 18, 23, 24, 29, 30, 32, 64):
        got, _ = cands(lib, [N] + [O if k % 2 else N for k in range(1, n)])
        keep = min(DLE_MAX, max(1, n // 6))
        assert got == [(k, 0 if k % 2 else 1) for k in range(n - keep, n)], n
    # the depth threshold: cleared, or left to the probe
    stack = [M, O, M, N, M, M, M, M, M]
    for min_layers, adaptive, want in ((0, 0, ([(3, 1)], 0)), (9, 0, ([(3, 1)], 0)), (9, 1, ([(3, 1)], 0)), (10, 0, ([], 0)), (10, 1, ([(3, 1)], 1)), (16, 1, ([(3, 1)], 1)),
                                       (16, 0, ([], 0)), (-1, 0, ([], 0)), (-1, 1, ([(3, 1)], 1))):   # a negative threshold compares as unsigned: every stack is below it
        assert cands(lib, stack, min_layers, adaptive) == want, (min_layers, adaptive)
    assert cands(lib, [M] * 9, 16, 1) == ([], 1)


def test_probe_verdict(lib):
    KEEP, PROBE = 1, 2
    for state in range(4):
        assert lib.pfx_int_flatten_verdict(0, 0, state) == lib.pfx_int_flatten_verdict(0, 1, state) == 0, state   # a call the elimination kernels cannot take
        assert lib.pfx_int_flatten_verdict(1, 0, state) == PROBE, state                                            # another stack's probe, or none
        assert lib.pfx_int_flatten_verdict(1, 1, state) == (KEEP if state == 2 else 0), state                      # pending, or answered


def test_defaults_give_the_shipped_routes(lib):
    """what the benchmark's stacks run: the 32-layer S2 stack (an Overwrite layer at depth 14) on the class-sorting kernel, nine layers streaming"""
    p = elim(lib, n_desc=32, w=7680, h=4320)
    assert (p.kernel, p.px, p.diag, p.sched.UA, p.redeal.s1, p.redeal.seg) == (SRT, 3, 0, 8, 15, 3)
    p = plan(lib, 9, 1024, 1024, mode_class=2)
    assert (p.kernel, p.px, p.nb, p.grid) == (STREAM, 4, 2, 1024)
