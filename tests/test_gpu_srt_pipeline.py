"""Parity gate (GPU): the pipelined passes of the class-sorting compositor (k_flatten.hip: srt_layers_pipe / srt_early_pipe).

The natural pass ends in a peeled tail whose free slot requests the NEXT unit's candidate alpha, the early pass ends on layer r - 1 and
hands its slot to the next early group or to layer r of the natural pass.  What can go wrong is control flow, not arithmetic: a unit
without a successor, a stream boundary on the image's last unit, either parity of either pass, a second candidate read on demand
behind a prefetched first one, one and two early groups, and the classification back-off engaging and releasing (the prefetch is
decided one unit ahead).  Every case is pfx_flatten_dev against the oracle at tolerance 0, seeded, a few hundred units at the most."""
import numpy as np
import pytest

from . import oracle_lib as O

pytestmark = pytest.mark.gpu

OVERWRITE, NORMAL = 14, 0
PLAIN_MODES = [m for m in range(1, 25) if m != OVERWRITE]


@pytest.fixture(scope="module")
def gpu():
    from .backends import GpuBackend
    g = GpuBackend(0)
    yield g
    for key, value in (("dle_units", 0), ("dle_sched", 1), ("dle_cfg", 0)):
        g.r.tune(key, value)


def plain_stack(rng, w, h, n):
    """n raster layers, none of which resets: random colours, alpha with zeros and 255s mixed in, modes other than Overwrite, opacity below 1"""
    stack = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    u = rng.random((n, h, w))
    stack[..., 3] = np.where(u < 0.2, 0, np.where(u < 0.45, 255, stack[..., 3]))
    modes = [NORMAL] + [PLAIN_MODES[(5 * k + 3) % len(PLAIN_MODES)] for k in range(1, n)]
    opac = [float(np.float32(0.35 + 0.6 * rng.random())) for _ in range(n)]
    return stack, modes, opac


def overwrite_layer(rng, stack, modes, opac, k, holes):
    """layer k becomes an Overwrite layer whose alpha is zero on a random fraction `holes` of the pixels (or where the boolean map `holes` says so)"""
    _, h, w, _ = stack.shape
    hole = holes if isinstance(holes, np.ndarray) else rng.random((h, w)) < holes
    modes[k], opac[k] = OVERWRITE, 0.7
    stack[k, ..., 3] = np.where(hole, 0, rng.integers(1, 256, (h, w))).astype(np.uint8)


def opaque_normal_layer(rng, stack, modes, opac, k, translucent):
    """layer k becomes a Normal layer at 100 % that resets where its alpha is 255: everywhere but on a random fraction `translucent`"""
    _, h, w, _ = stack.shape
    modes[k], opac[k] = NORMAL, 1.0
    stack[k, ..., 3] = np.where(rng.random((h, w)) < translucent, rng.integers(0, 255, (h, w)), 255).astype(np.uint8)


def check(gpu, stack, modes, opac, what, stats=False):
    """pfx_flatten_dev against the oracle at tolerance 0; stats: returns the launch's work counters (pfx_flatten_stats) so that a test can see that the
    path it is about did run"""
    n, h, w, _ = stack.shape
    ref = O.flatten_stack(stack, np.asarray(modes, np.uint8), np.asarray(opac, np.float32))
    r = gpu.r
    bufs = [r.dev_alloc(w * h * 4) for _ in range(n + 1)]
    try:
        for k in range(n):
            r.dev_upload(bufs[k], stack[k])
        info = [(k, float(opac[k]), True, int(modes[k])) for k in range(n)]
        if stats:
            r.tune("dle_stats", 1)
            r.flatten_stats(reset=True)
        r.flatten_dev(bufs[:n], info, w, h, bufs[n])
        got = r.dev_download(bufs[n], (h, w, 4))
        st = r.flatten_stats(reset=True) if stats else None
    finally:
        if stats:
            r.tune("dle_stats", 0)
        for b in bufs:
            r.dev_free(b)
    bad = (got != ref).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {w * h} px differ, first at flat index {int(np.flatnonzero(bad)[0])}"
    return st


@pytest.mark.parametrize("size", [(191, 1), (192, 1), (193, 1), (383, 1), (385, 1), (64, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cfg", [0, 1], ids=["px3", "px2"])
def test_pixel_counts_around_one_and_two_units(gpu, size, cfg):
    """one unit, a tail unit, two units of which the second does not exist for some streams (192 pixels per unit; 128 with two pixels per lane)"""
    w, h = size
    rng = np.random.default_rng(100 + w + h)
    stack, modes, opac = plain_stack(rng, w, h, 18)
    overwrite_layer(rng, stack, modes, opac, 9, 0.25)
    gpu.r.tune("dle_cfg", cfg)
    try:
        check(gpu, stack, modes, opac, f"{w}x{h} dle_cfg={cfg}")
    finally:
        gpu.r.tune("dle_cfg", 0)


@pytest.mark.parametrize("units", [1, 2, 3])
@pytest.mark.parametrize("sched", [0, 1], ids=["equal-streams", "shrinking-streams"])
def test_stream_boundaries_on_the_last_unit(gpu, units, sched):
    """streams of 1, 2 and 3 units (and the shorter ones behind them) over images of 40 units, 40 units and a 5-pixel tail, and 41 units less a
    few pixels: the last stream ends on a full unit, on a tail unit, and one unit short of its length"""
    gpu.r.tune("dle_units", units)
    gpu.r.tune("dle_sched", sched)
    try:
        for w, h in ((96, 80), (53, 145), (97, 81), (192 * 3, 1), (192 * 4 + 1, 1)):
            rng = np.random.default_rng(200 + w)
            stack, modes, opac = plain_stack(rng, w, h, 16)
            overwrite_layer(rng, stack, modes, opac, 7, 0.25)
            check(gpu, stack, modes, opac, f"{w}x{h} dle_units={units} dle_sched={sched}")
    finally:
        gpu.r.tune("dle_units", 0)
        gpu.r.tune("dle_sched", 1)


@pytest.mark.parametrize("n,r", [(32, 14), (32, 15), (17, 8), (17, 9), (32, 31), (32, 30), (16, 1), (16, 2)])
def test_both_parities_of_both_passes(gpu, n, r):
    """one reset layer at r of n: the natural pass runs n - r layers, the early pass r (its pixels start at layer 0) — both parities of both, and passes
    of one and two layers, which are all tail"""
    rng = np.random.default_rng(300 + 40 * n + r)
    w, h = 200, 23
    stack, modes, opac = plain_stack(rng, w, h, n)
    overwrite_layer(rng, stack, modes, opac, r, 0.25)
    check(gpu, stack, modes, opac, f"reset layer {r} of {n}")


@pytest.mark.parametrize("s_u,r", [(3, 14), (3, 15), (4, 14), (4, 15)])
def test_early_pass_that_starts_above_the_bottom(gpu, s_u, r):
    """a lower reset layer without holes under the split layer: the early pass runs layers [s_u, r), both parities of r - s_u"""
    rng = np.random.default_rng(350 + 20 * s_u + r)
    w, h = 211, 19
    stack, modes, opac = plain_stack(rng, w, h, 32)
    overwrite_layer(rng, stack, modes, opac, s_u, 0.0)
    overwrite_layer(rng, stack, modes, opac, r, 0.3)
    check(gpu, stack, modes, opac, f"reset layers {s_u} (no holes) and {r}")


@pytest.mark.parametrize("cands", [2, 3, 4])
def test_further_candidates_behind_a_prefetched_first_one(gpu, cands):
    """2, 3 and 4 candidates (Overwrite layers and opaque Normal layers at 100 %) whose topmost leaves pixels unclassified: the lower ones are read on
    demand, per unit, behind the topmost one's prefetched alpha; in the left third of the image the topmost one has no holes and nothing is read on demand"""
    rng = np.random.default_rng(400 + cands)
    w, h = 384, 24
    stack, modes, opac = plain_stack(rng, w, h, 32)
    layers = [26, 19, 11, 5][:cands]
    for i, k in enumerate(layers):
        if i % 2 == 0:
            hole = rng.random((h, w)) < 0.45
            if i == 0:
                hole[:, : w // 3] = False
            overwrite_layer(rng, stack, modes, opac, k, hole)
        else:
            opaque_normal_layer(rng, stack, modes, opac, k, 0.5)
    check(gpu, stack, modes, opac, f"{cands} candidates at {layers[::-1]}")


@pytest.mark.parametrize("holes", [0.25, 0.6], ids=["one-early-group", "two-early-groups"])
@pytest.mark.parametrize("r", [14, 15])
def test_units_that_split_into_one_and_two_early_groups(gpu, holes, r):
    """about 25 % holes in the reset layer: 48 early pixels of 192, one early group; about 60 %: 115, two groups, the first of which hands its slot to the second"""
    rng = np.random.default_rng(500 + int(holes * 100) + r)
    w, h = 192, 40
    stack, modes, opac = plain_stack(rng, w, h, 32)
    overwrite_layer(rng, stack, modes, opac, r, holes)
    st = check(gpu, stack, modes, opac, f"{holes} holes in reset layer {r}", stats=True)
    # "rounds" counts early groups run, "queue_units" the units that split.  192 pixels with hole probability p: 48 +- 6 early pixels at 0.25 — one group of 64
    # unless a unit is 2.7 sigma out, and every unit splits; 115 +- 7 at 0.6 — two groups (65 .. 128 early pixels; fewer is 7 sigma away), except that a unit
    # with more than 128 (1.9 sigma, 3 % of the units) would need all three groups and is not split at all
    if holes < 0.5:
        assert st["queue_units"] == 40 and 40 <= st["rounds"] <= 42, st
    else:
        assert st["queue_units"] >= 36 and st["rounds"] == 2 * st["queue_units"], st


@pytest.mark.parametrize("transparent_first", [True, False], ids=["miss-then-hit", "hit-then-miss"])
def test_classification_back_off_engages_and_releases(gpu, transparent_first):
    """two streams of 40 units (one image row each): the reset layer is fully transparent over 20 units of a stream and hit on the other 20, in either
    order — the back-off stops the probing and takes it up again, and the prefetch is decided one unit ahead of both"""
    rng = np.random.default_rng(600 + int(transparent_first))
    w, h = 192, 80
    stack, modes, opac = plain_stack(rng, w, h, 20)
    rows = np.arange(h) % 40
    dead_rows = rows < 20 if transparent_first else rows >= 20
    hole = (rng.random((h, w)) < 0.25) | dead_rows[:, None]
    overwrite_layer(rng, stack, modes, opac, 10, hole)
    gpu.r.tune("dle_units", 40)
    gpu.r.tune("dle_sched", 0)
    try:
        st = check(gpu, stack, modes, opac, "back-off", stats=True)
        # one candidate, one alpha read per probed unit: the back-off engaged if fewer units were probed than exist, and released (or never engaged on the
        # hit half) if more were probed than the two failing probes at the head of each 14-unit pause could account for (80 units: at most 2 * 6 of those)
        assert 12 < st["alpha_reads"] < st["nat_units"] == 80, st
    finally:
        gpu.r.tune("dle_units", 0)
        gpu.r.tune("dle_sched", 1)
