"""The ZNCC sweep's contract without a GPU: what the crafted case of tests/zncc_cases.py holds, asserted on the
mirror (tests/zncc_mirror.py); the views add; the mirror against a loop at hand-picked cells; and the accuracy figures that section 21 and
the README quote, with the oracle's absolute-difference sweep beside them."""
import numpy as np
import pytest

import zncc_cases as zc
import zncc_mirror as zm


@pytest.mark.parametrize("r", zc.RADII)
def test_crafted_case_holds_what_it_is_for(r):
    c = zc.crafted()
    per_view = [zc.crafted_view(r, v) for v in range(c.V)]
    ok = np.stack([p[0] for p in per_view])
    counted = np.stack([p[1] for p in per_view])
    cost = np.stack([p[2] for p in per_view])
    n = counted[:3].sum(0)                       # the general views alone, as the issue's figures
    unseen, partial = (n == 0).mean(), ((n > 0) & (n < 3)).mean()
    flat = (ok[:3] & ~counted[:3]).any(0).mean()
    above = (cost[:3][counted[:3]] > 32512).mean()
    print("r = %d: unseen %.1f %%, partially seen %.1f %%, a view dropped for a flat patch %.1f %%, costs above 32512 %.1f %%" % (
        r, 100 * unseen, 100 * partial, 100 * flat, 100 * above))
    assert unseen >= 0.01 and partial >= 0.20 and flat >= 0.05
    assert not (counted & ~ok).any()
    # view 3 is the main frame itself, view 4 its inverse: the two ends of the scale, wherever the patch is not flat
    assert counted[3].any() and (cost[3][counted[3]] == 0).all()
    assert counted[4].any() and (cost[4][counted[4]] == 65024).all()
    if r <= 3:                                   # pixel (5, 9): the window lies inside the constant block main[2:9, 5:14], so va = 0
        assert ok[3][:, 5, 9].all() and not counted[3][:, 5, 9].any()
    assert (cost[~counted] == 0).all() and cost.max() <= 65024
    vol = zc.crafted_volume(r)
    assert ((vol & 0xffffff) <= 65024 * (vol >> 24)).all() and (vol >> 24).max() == c.V


@pytest.mark.parametrize("r", zc.RADII)
def test_views_add(oracle, r):
    c = zc.crafted()
    whole = zm.volume(oracle, *c.views(), c.planes(oracle), r)
    np.testing.assert_array_equal(whole, zc.crafted_volume(r))
    np.testing.assert_array_equal(zc.crafted_volume(r, (0, 1)) + zc.crafted_volume(r, (2, 3, 4)), whole)
    np.testing.assert_array_equal(sum(zc.crafted_volume(r, (v,)) for v in range(c.V)), whole)
    assert (zc.crafted_volume(r, (1,)) != 0).any() and (zc.crafted_volume(r, (2,)) != 0).any()


@pytest.mark.parametrize("r", zc.RADII)
def test_mirror_against_a_loop(oracle, r):
    c = zc.crafted()
    z = c.planes(oracle)
    for v, d in ((3, 0), (2, 3), (1, 5)):
        B, ok = zm.warped(oracle, c.main_cam, c.side_cams[v], c.sides[v], z[d])
        ok_d, counted, cost = (a[d] for a in zc.crafted_view(r, v))
        np.testing.assert_array_equal(ok, ok_d)
        # the frame's corners, a cell beside the constant block, one in the middle of a tile rest
        for row, col in ((0, 0), (c.H - 1, c.W - 1), (5, 14), (17, 66)):
            N, cnt, cst = zm.brute_cell(c.main_img, B, ok, r, row, col)
            assert (cnt, cst) == (bool(counted[row, col]), int(cost[row, col])), (v, d, row, col)
            if v == 3 and (row, col) in ((0, 0), (c.H - 1, c.W - 1)):
                assert N == (r + 1) ** 2            # the identity view is in frame everywhere: the corner's window is what the frame leaves of it


def test_accuracy(oracle):
    """the table of DESIGN.md section 21: bad pixels (more than 1.5 plane steps from the analytic depth, winner-take-all) and the median
    error after the refinement, absolute difference against ZNCC at radius 3, frames as rendered and with gains and offsets"""
    fig = {}
    for gains in (False, True):
        e = zc.exposure(gains)
        sad = oracle.sweep(*e.views(), e.D, want_volume=True, nthreads=4, sampler="fixed")[3]
        fig[gains, "sad"] = zc.quality(oracle, sad, e.truth, e.D)
        fig[gains, "zncc"] = zc.quality(oracle, zc.exposure_volume(gains, e.R), e.truth, e.D)
        for k in ("sad", "zncc"):
            print("%-12s %-5s bad %.1f %%, median %.4f" % ("with gains" if gains else "as rendered", k, 100 * fig[gains, k][0], fig[gains, k][1]))
    assert fig[True, "zncc"][0] <= 0.05 and fig[True, "sad"][0] >= 0.50
    assert fig[False, "zncc"][0] <= fig[False, "sad"][0]
