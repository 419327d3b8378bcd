"""The flood model (tests/flood_model.py) checked against itself and against hand-worked cases, without a GPU: it is the oracle of tests/test_gpu_flood.py, so
its two flood algorithms must agree on every case used there, and every case must have a non-trivial answer (no GPU test may pass vacuously)."""
import numpy as np
import pytest

from . import flood_cases as FC
from . import flood_model as M


def px(v):
    """a pixel whose legacy distance to opaque black is v"""
    return (v, 0, 0, 255)


BLACK = (0, 0, 0, 255)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("mode", [M.LEGACY, M.PERCEPTUAL])
@pytest.mark.parametrize("case", FC.DISTANCE_CASES, ids=[c[0] for c in FC.DISTANCE_CASES])
def test_two_algorithms_agree_and_the_answer_is_not_trivial(case, mode, connectivity):
    d = FC.distance_expected(case[0], mode, connectivity, False, True)     # check=True: Dijkstra == relaxation, asserted inside
    g = FC.distance_expected(case[0], mode, connectivity, True, True)
    assert (d >= g).all()                                                   # a path's largest step is at least its last one
    img, seed, target = FC.case_image(case)
    assert d[seed[1], seed[0]] == g[seed[1], seed[0]]
    if d.size > 1:
        assert len(np.unique(d)) > 1 and len(np.unique(g)) > 1
    for t in (0, 1, 37, 128, 254):                                          # {d <= t} grows with t
        assert (d <= t).sum() <= (d <= t + 1).sum()
        assert not ((d <= t) & ~(d <= t + 1)).any()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(FC.CORRIDORS))
def test_corridors(name, connectivity):
    img, order = FC.CORRIDORS[name]()
    n = img.shape[0]
    d = FC.corridor_expected(name, connectivity, True)
    walls = np.ones((n, n), bool)
    for x, y in order:
        walls[y, x] = False
    assert len(order) > 60 * n and (img[..., 0][walls] >= 100).all()
    # the far end is reached along the corridor only: its distance is the corridor's last value, far below any wall
    fx, fy = order[-1]
    assert d[fy, fx] == 40
    if connectivity == 4:
        assert all(d[y, x] == img[y, x, 0] for x, y in order)              # rising along the corridor: each pixel's own value
    assert (d[walls] >= 100).all()
    tile_crossings = sum(1 for a, b in zip(order, order[1:]) if (a[0] // FC.TILE, a[1] // FC.TILE) != (b[0] // FC.TILE, b[1] // FC.TILE))
    assert tile_crossings >= 24


def test_the_long_corridor_re_enters_the_tiles_it_left():
    img, order = FC.CORRIDORS["long_snake"]()
    assert img.shape[0] == FC.LONG_SNAKE_N and FC.tile_count(*img.shape[1::-1]) == 16
    tiles = [(x // FC.TILE, y // FC.TILE) for x, y in order]
    runs = [t for k, t in enumerate(tiles) if k == 0 or t != tiles[k - 1]]      # the tiles in the order the corridor visits them
    assert len(runs) - 1 >= 40                                                   # border crossings
    entries = {t: runs.count(t) for t in set(runs)}
    print("border crossings", len(runs) - 1, "most entries into one tile", max(entries.values()))
    assert len(entries) == 16 and sum(1 for v in entries.values() if v >= 16) >= 9      # every whole tile is left and entered again dozens of times


@pytest.mark.parametrize("run", FC.MANY_TILE_RUNS, ids=["legacy-4", "perceptual-8"])
@pytest.mark.parametrize("case", FC.MANY_TILE_CASES, ids=[c[0] for c in FC.MANY_TILE_CASES])
def test_many_tile_cases_have_many_tiles_and_an_answer_that_is_not_trivial(case, run):
    mode, connectivity = run
    name, w, h, kind, seed, target = case
    tiles_x, tiles_y = -(-w // FC.TILE), -(-h // FC.TILE)
    if name.startswith("many-"):
        assert (w, h) == (FC.MANY_W, FC.MANY_H) and tiles_x * tiles_y >= 63 and w % FC.TILE == 1 and h % FC.TILE == 1
        assert (seed[0] % FC.TILE, seed[1] % FC.TILE) in ((0, 0), (FC.TILE - 1, FC.TILE - 1))      # a tile's corner pixel
    else:
        assert sorted((tiles_x, tiles_y)) == [1, 40] and w % FC.TILE == FC.TILE - 1 and h % FC.TILE == FC.TILE - 1
    d = FC.many_tile_expected(name, mode, connectivity, False)
    img, seed, target = FC.case_image(case)
    c = M.color_distance(img, target, mode)
    assert np.array_equal(d, M.relaxation(c, seed, connectivity))           # the model's two algorithms agree
    assert np.array_equal(FC.many_tile_expected(name, mode, connectivity, True), c) and (d >= c).all()
    assert len(np.unique(d)) > 1 and len(np.unique(c)) > 1
    below = d < 255                                                          # the flood leaves the seed's tile: pixels below 255 in several tiles
    ys, xs = np.nonzero(below)
    reached = len(set(zip((xs // FC.TILE).tolist(), (ys // FC.TILE).tolist())))
    print(name, run, "tiles", tiles_x * tiles_y, "tiles reached below 255:", reached, "distinct distances", len(np.unique(d)))
    assert reached == tiles_x * tiles_y      # every tile is listed at least once


def test_the_uniform_many_tile_image():
    assert FC.tile_count(FC.MANY_W, FC.MANY_H) == FC.MANY_TILES_X * FC.MANY_TILES_Y >= 63
    img = FC.uniform_many()
    assert img.shape == (FC.MANY_H, FC.MANY_W, 4) and (img == img[0, 0]).all()      # so the model's map is 0 everywhere: c is 0, and d <= max over a path of c
    assert not M.color_distance(img, img[0, 0], M.LEGACY).any()
    for where, seed in FC.MANY_SEEDS.items():
        assert 0 <= seed[0] < FC.MANY_W and 0 <= seed[1] < FC.MANY_H
        for connectivity in (4, 8):
            d = FC.uniform_many_expected(where, connectivity)
            assert d.shape == (FC.MANY_H, FC.MANY_W) and not d.any()


def ring(gap):
    """5 x 5: a wall ring around the centre; with `gap` the wall's corner pixel (1, 1) is open: a diagonal-only way out"""
    v = np.zeros((5, 5), np.uint8)
    v[1:4, 1:4] = 200
    v[2, 2] = 0
    if gap:
        v[1, 1] = 0
    img = np.zeros((5, 5, 4), np.uint8)
    img[..., 0] = v
    img[..., 3] = 255
    return img


def test_ring_wall_by_hand():
    for conn in (4, 8):
        d = M.distance_map(ring(False), (2, 2), BLACK, M.LEGACY, conn, False)
        want = np.full((5, 5), 200, np.uint8)        # every way out crosses the wall
        want[2, 2] = 0
        assert np.array_equal(d, want)
    d4 = M.distance_map(ring(True), (2, 2), BLACK, M.LEGACY, 4, False)
    assert d4[2, 2] == 0 and d4[1, 1] == 200 and d4[0, 0] == 200      # the open corner touches the centre only diagonally
    d8 = M.distance_map(ring(True), (2, 2), BLACK, M.LEGACY, 8, False)
    want = np.zeros((5, 5), np.uint8)
    want[1:4, 1:4] = 200
    want[2, 2] = want[1, 1] = 0
    assert np.array_equal(d8, want)                                      # the flood leaks through the diagonal gap


def test_unreachable_pixels_keep_255():
    img = np.zeros((3, 7, 4), np.uint8)
    img[..., 3] = 255
    img[:, 3, 0] = 255                                                   # a wall at the largest distance
    d = M.distance_map(img, (0, 1), BLACK, M.LEGACY, 8, False)
    assert (d[:, :3] == 0).all() and (d[:, 3:] == 255).all()


def test_both_transparent_is_zero():
    img = np.array([[(10, 20, 30, 0), (10, 20, 30, 1), (200, 0, 0, 255)]], np.uint8)
    for mode in (M.LEGACY, M.PERCEPTUAL):
        c = M.color_distance(img, (99, 98, 97, 0), mode)
        assert c[0, 0] == 0 and c[0, 1] > 0 and c[0, 2] == 255
    assert M.color_distance(img, (99, 98, 97, 0), M.LEGACY)[0, 1] == 89


def test_perceptual_spot_values():
    one = lambda p, t: int(M.color_distance(np.array([[p]], np.uint8), t, M.PERCEPTUAL)[0, 0])
    assert one((255, 255, 255, 255), (0, 0, 0, 255)) == 179      # dluma = 1, dchroma = 0: f32(0.7) * 255 = 178.499997 rounds to the f32 178.5, a tie, away from zero
    assert one((0, 0, 0, 255), (0, 0, 0, 255)) == 0
    assert one((0, 0, 0, 128), (0, 0, 0, 255)) == 127            # the alpha term: |128 / 255 - 1| * 255
    assert one((255, 0, 0, 255), (0, 0, 0, 255)) == 242          # dluma = 0.2126, dchroma = sqrt(0.5 + 0.5) = 1: (0.14882 + 0.8) * 255 = 241.9
    assert one((128, 128, 128, 255), (127, 127, 127, 255)) == 1
    assert one((1, 0, 0, 255), (0, 0, 0, 255)) == 0              # the legacy distance here is 1 (the reason the bucket tool uses legacy, :1267-1271)


def test_tolerance_threshold_spot_values():
    want = {0.0: 0, -3.0: 0, 0.1: 0, 0.2: 1, 10.0: 26, 37.3: 95, 50.0: 128, 99.9: 255, 100.0: 255, 250.0: 255, float("nan"): 0}
    for tol, t in want.items():
        assert M.tolerance_threshold(tol) == t, tol


def test_tolerance_threshold_matches_the_library():
    import paintfe_amd
    for tol in list(np.linspace(-5, 105, 221)) + [float("nan"), float("inf"), -float("inf")]:
        assert paintfe_amd.tolerance_threshold(float(tol)) == M.tolerance_threshold(float(tol)), tol


def test_threshold_alpha_and_combine_by_hand():
    d = np.array([[0, 5, 6, 7, 255]], np.uint8)
    assert M.threshold_alpha(d, 5, False).tolist() == [[255, 255, 0, 0, 0]]
    assert M.threshold_alpha(d, 5, True).tolist() == [[255, 255, 128, 0, 0]]
    assert M.threshold_alpha(d, 254, True).tolist() == [[255, 255, 255, 255, 128]]
    assert M.threshold_alpha(d, 255, True).tolist() == [[255] * 5]        # sat_add(255, 1) == 255 <= threshold: everything is 255
    base = np.array([[200, 0, 200, 90, 255]], np.uint8)
    assert M.wand_mask(d, 5, True, M.REPLACE, base).tolist() == [[255, 255, 128, 0, 0]]
    assert M.wand_mask(d, 5, True, M.ADD, base).tolist() == [[255, 255, 200, 90, 255]]
    assert M.wand_mask(d, 5, True, M.SUBTRACT, base).tolist() == [[0, 0, 72, 90, 255]]
    assert M.wand_mask(d, 5, True, M.INTERSECT, base).tolist() == [[200, 0, 100, 0, 0]]
    assert M.wand_mask(d, 5, True, M.INTERSECT, None).tolist() == [[0] * 5]   # a missing base is all zero


def test_bboxes_by_hand():
    d = np.full((4, 6), 9, np.uint8)
    d[2, 3] = 4
    d[1, 5] = 6
    b = M.bboxes(d)
    assert (b[:4] == -1).all()
    assert b[4].tolist() == [3, 2, 3, 2] and b[5].tolist() == [3, 2, 3, 2]
    assert b[6].tolist() == [3, 1, 5, 2] and b[8].tolist() == [3, 1, 5, 2]
    assert b[9].tolist() == [0, 0, 5, 3] and b[255].tolist() == [0, 0, 5, 3]


def test_threshold_stage_inputs_are_not_trivial():
    d = FC.ramp_distance()
    assert len(np.unique(d)) == 256
    for t in FC.THRESHOLDS[:-1]:
        assert 0 < (d <= t).sum() < d.size
        assert (d == t + 1).any()                                         # the AA band is hit
    assert (d <= 255).all()
    sel = FC.selection()
    assert 0 < (sel > 0).sum() < sel.size and ((sel > 0) & (sel < 255)).any()
    for t in FC.THRESHOLDS[:-1]:
        assert 0 < ((d <= t) & (sel > 0)).sum() < (d <= t).sum()
    assert (M.bboxes(d)[0] >= 0).all()
    d2 = d.copy()
    d2[d2 < 3] = 3
    assert (M.bboxes(d2)[:3] == -1).all() and (M.bboxes(d2)[3] >= 0).all()


def test_bucket_fill_cases_are_not_trivial():
    layer = FC.layer()
    for seed, tol, global_fill in [((5, 5), 5.0, False), ((5, 5), 5.0, True), ((100, 40), 12.0, False)]:
        target = layer[seed[1], seed[0]]
        d = M.distance_map(layer, seed, target, M.LEGACY, 4, global_fill)
        n = (d <= M.tolerance_threshold(tol)).sum()
        assert 0 < n < d.size
    contiguous = M.distance_map(layer, (5, 5), layer[5, 5], M.LEGACY, 4, False) <= M.tolerance_threshold(5.0)
    everywhere = M.distance_map(layer, (5, 5), layer[5, 5], M.LEGACY, 4, True) <= M.tolerance_threshold(5.0)
    assert contiguous.sum() < everywhere.sum()                            # the same colour comes back in a region the flood cannot reach
    out = M.bucket_fill(layer, (5, 5), 5.0, (10, 20, 30, 128), 0, False)
    assert np.array_equal(out[~contiguous], layer[~contiguous]) and (out[contiguous] != layer[contiguous]).any()


def test_lines_through_a_border_seed_are_reached_on_both_sides():
    """the cases whose seed sits on a tile border with nothing else in its tile below 255: the model's line is at 0 on both sides of the border"""
    for name, conn in [("130x70-line-seed-on-border", 4), ("130x70-line-seed-on-border", 8), ("130x70-line-seed-right-border", 4)]:
        d = FC.distance_expected(name, M.LEGACY, conn, False, True)
        assert (d[20] == 0).all() and (np.delete(d, 20, axis=0) == 255).all()
    for name in ("130x70-cross-seed-on-corner", "130x70-cross-seed-before-corner"):
        d = FC.distance_expected(name, M.LEGACY, 4, False, True)
        assert (d[64] == 0).all() and (d[:, 64] == 0).all() and (d == 0).sum() == 130 + 70 - 1
    d = FC.distance_expected("65x1-seed-alone", M.LEGACY, 4, False, True)
    assert d[0, 64] == 0 and (d[0, :64] < 255).all()
