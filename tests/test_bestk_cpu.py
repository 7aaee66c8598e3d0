"""The occlusion-robust sweep's contract without a GPU: what the crafted case of tests/bestk_cases.py holds,
asserted on the mirror (tests/bestk_mirror.py); the mirror against a loop at hand-picked cells; MVS_KEEP_ALL against the summing sweeps'
own references; and the occluder scene's figures that section 22 and the README quote."""
import numpy as np
import pytest

import bestk_cases as bk
import bestk_mirror as bm
import zncc_cases as zc

ABSDIFF, ZNCC, KEEP_ALL = bk.ABSDIFF, bk.ZNCC, bk.KEEP_ALL


def _stacked(cost, r):
    per_view = [bk.crafted_view(cost, r, v) for v in range(bk.Crafted.V)]
    return np.stack([p[0] for p in per_view]), np.stack([p[1] for p in per_view]).astype(np.int64)


@pytest.mark.parametrize("cost,r", bk.COST_RADII)
@pytest.mark.parametrize("keep", (2, 3))
def test_crafted_case_holds_what_it_is_for(cost, r, keep):
    counted, c = _stacked(cost, r)
    # the main camera's views 3 and 4 are in frame everywhere, so the cells with few counted views are those of the ranges without them:
    # every class must hold at least 1 % of the cells of one of the ranges the device tests run
    shares = {}
    for first, count in bk.RANGES:
        n = counted[first:first + count].sum(0)
        for name, share in (("n = 0", (n == 0).mean()), ("0 < n < keep", ((n > 0) & (n < keep)).mean()), ("n = keep", (n == keep).mean()),
                            ("n > keep", (n > keep).mean())):
            shares[name] = max(shares.get(name, 0.0), float(share))
        print("%s r = %d, views [%d, %d): %s %% of the cells with n = 0 .. %d" % (
            bk.NAMES[cost], r, first, first + count, " ".join("%.1f" % (100 * (n == i).mean()) for i in range(count + 1)), count))
    assert all(v >= 0.01 for v in shares.values()), shares
    n = counted.sum(0)
    assert n.max() == bk.Crafted.V
    # the duplicate: equal costs wherever view 0 counts
    assert counted[0].mean() >= 0.10 and (counted[5] == counted[0]).all() and (c[5] == c[0]).all()
    # the identity view: cost 0, the smallest, wherever it counts
    assert counted[3].mean() >= 0.50 and (c[3][counted[3]] == 0).all()
    vol = bk.crafted_volume(cost, r, keep)
    assert ((vol >> 24) == np.minimum(n, keep)).all() and (vol[n == 0] == 0).all()
    if cost == ZNCC:
        # the inverted view: 65024, the top of the scale, is never kept where another view could be: the cell is that of the other views
        assert (c[4][counted[4]] == 65024).all()
        drop = counted[4] & (n >= keep + 1)
        assert drop.mean() >= 0.10
        np.testing.assert_array_equal(vol[drop], bk.crafted_volume(cost, r, keep, (0, 1, 2, 3, 5))[drop])
    one = bk.crafted_volume(cost, r, 1)
    assert (one[counted[3]] == 1 << 24).all(), "keep 1 keeps the identity view's 0"


@pytest.mark.parametrize("cost,r", bk.COST_RADII)
def test_mirror_against_a_loop(oracle, cost, r):
    c = bk.crafted()
    z = c.planes(oracle)
    counted, costs = _stacked(cost, r)
    n = counted.sum(0)
    keep = 3
    few = tuple(np.argwhere((n > 0) & (n < keep))[0])                     # a cell with n < keep
    # views 0 and 5 tie right behind the identity view's 0: keep 2 cuts the tie in the middle, keep 3 takes both
    others = np.where(counted[[1, 2, 4]], costs[[1, 2, 4]], 1 << 30).min(0)
    tie = tuple(np.argwhere(counted[0] & counted[3] & (costs[0] > 0) & (costs[0] < others))[0])
    cells = [(0, 0, 0), (3, 0, c.W - 1), (5, c.H - 1, 0), (c.D - 1, c.H - 1, c.W - 1), few, tie, (2, 9, 40)]
    for d, row, col in cells:
        for k in (1, 2, keep, 8, KEEP_ALL):
            nb, cb, cell = bm.brute_cell(oracle, cost, *c.views(), z[d], r, k, row, col)
            assert nb == n[d, row, col] and cb == [int(x) for x in costs[:, d, row, col][counted[:, d, row, col]]], (d, row, col)
            assert cell == int(bk.crafted_volume(cost, r, k)[d, row, col]), (d, row, col, k)
    d, row, col = tie
    assert sorted(costs[:, d, row, col][counted[:, d, row, col]])[:3] == [0, costs[0, d, row, col], costs[5, d, row, col]]
    assert int(bk.crafted_volume(cost, r, 2)[tie]) == (2 << 24) + costs[0, d, row, col]
    # a view range: the loop over [1, 4)
    for d, row, col in cells[:4]:
        assert bm.brute_cell(oracle, cost, *c.views(), z[d], r, 2, row, col, views=range(1, 4))[2] == int(bk.crafted_volume(cost, r, 2, (1, 2, 3))[d, row, col])


@pytest.mark.parametrize("r", zc.RADII)
def test_keep_all_with_zncc_is_the_zncc_sweep(r):
    np.testing.assert_array_equal(bk.crafted_volume(ZNCC, r, KEEP_ALL, range(5)), zc.crafted_volume(r))
    np.testing.assert_array_equal(bk.crafted_volume(ZNCC, r, KEEP_ALL, (1, 2)), zc.crafted_volume(r, (1, 2)))


def test_keep_all_with_single_pixel_absdiff_is_the_ordinary_sweep(oracle):
    c = bk.crafted()
    ref = oracle.sweep(*c.views(), c.D, c.Z_LO, c.Z_HI, want_volume=True, sampler="fixed")[3]
    np.testing.assert_array_equal(bk.crafted_volume(ABSDIFF, 0, KEEP_ALL), ref)
    ref = oracle.sweep(c.main_cam, c.main_img, c.side_cams[1:4], c.sides[1:4], c.D, c.Z_LO, c.Z_HI, want_volume=True, sampler="fixed")[3]
    np.testing.assert_array_equal(bk.crafted_volume(ABSDIFF, 0, KEEP_ALL, (1, 2, 3)), ref)


@pytest.mark.parametrize("cost,r", bk.COST_RADII)
def test_keep_of_at_least_n_is_keep_all(cost, r):
    counted, _ = _stacked(cost, r)
    n = counted.sum(0)
    every = bk.crafted_volume(cost, r, KEEP_ALL)
    for keep in (1, 2, 3, 8):
        vol = bk.crafted_volume(cost, r, keep)
        np.testing.assert_array_equal(vol[n <= keep], every[n <= keep])
        if keep < bk.Crafted.V:
            assert (vol[n > keep] >> 24 == keep).all() and ((vol[n > keep] & 0xffffff) <= (every[n > keep] & 0xffffff)).all()
    # the volumes of disjoint view ranges do not add
    assert (bk.crafted_volume(cost, r, 2, (0, 1, 2)) + bk.crafted_volume(cost, r, 2, (3, 4, 5)) != bk.crafted_volume(cost, r, 2)).any()


def test_occluder_scene(oracle):
    """the table of DESIGN.md section 22: 160 x 100, 4 views (asserted) and 8 views (printed); bad pixels (more than 1.5 plane steps from
    the analytic depth, winner-take-all) over the whole image and over the background pixels within 12 px of the occluder's outline"""
    o = bk.occluder()
    assert 0.15 <= o.front.mean() <= 0.25 and 0.15 <= o.edge.mean() <= 0.25
    fig = {}
    for V, keeps in ((4, (KEEP_ALL, 2, 3)), (8, (KEEP_ALL, 2, 3, 4))):
        for name, cost, r, D in (("zncc r2", ZNCC, 2, 48), ("absdiff r2", ABSDIFF, 2, 64), ("absdiff r0", ABSDIFF, 0, 64)):
            for keep in keeps:
                fig[V, name, keep] = bk.bad_shares(oracle, bk.occluder_volume(cost, r, D, keep, V), D, V)
                print("%d views %-10s %2d planes keep %-3s bad %.2f %% of the image, %.2f %% of the edge" % (
                    V, name, D, keep or "all", 100 * fig[V, name, keep][0], 100 * fig[V, name, keep][1]))
    print("4 views, edge, keep 2 / keep all: zncc %.2f, absdiff %.2f" % (fig[4, "zncc r2", 2][1] / fig[4, "zncc r2", KEEP_ALL][1],
                                                                        fig[4, "absdiff r2", 2][1] / fig[4, "absdiff r2", KEEP_ALL][1]))
    assert fig[4, "zncc r2", KEEP_ALL][1] > 0 and fig[4, "zncc r2", 2][1] <= 0.5 * fig[4, "zncc r2", KEEP_ALL][1]
    assert fig[4, "absdiff r2", 2][1] < fig[4, "absdiff r2", KEEP_ALL][1]
    # the documented warning, kept honest: best-K of single-pixel costs is worse than their sum
    assert fig[4, "absdiff r0", 2][0] > fig[4, "absdiff r0", KEEP_ALL][0]
