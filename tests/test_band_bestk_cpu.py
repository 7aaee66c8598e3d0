"""The windowed band sweep's contract without a GPU: the mirror (tests/band_bestk_mirror.py) against a loop at
hand-picked cells; what the crafted case of tests/band_bestk_cases.py holds, so that every rule is exercised; the three identities with
the sweeps it joins, on the mirror; and the justification: two levels on a filtered prior against the global ZNCC sweep at equal samples
on the exposure scene, with the figures section 24 and the README quote."""
import numpy as np
import pytest

import band_bestk_cases as bb
import band_bestk_mirror as bbm
import band_cases as bc
import band_mirror as bm
import bestk_cases as bk
import bestk_mirror as km
import zncc_cases as zc
import zncc_mirror as zm

ABSDIFF, ZNCC, KEEP_ALL = bb.ABSDIFF, bb.ZNCC, bb.KEEP_ALL


def _stacked(cost, r):
    per_view = [bb.crafted_view(cost, r, v) for v in range(bb.Crafted.V)]
    return np.stack([p[0] for p in per_view]), np.stack([p[1] for p in per_view]).astype(np.int64)


def _member_counts(oracle, cost, r, v):
    """(ok of the centre, members of the window, live pixels of the window) of view v over the crafted case, [D, H, W] each"""
    c = bb.crafted()
    one = bm.band_volume(oracle, c.main_cam, c.main_img, c.side_cams[v][None], [c.sides[v]], c.prior, c.offsets(oracle))
    ok = (one >> 24).astype(np.int64)
    live = bm.planes(c.prior, c.offsets(oracle))[1].astype(np.int64)
    return ok, np.stack([zm.box(m, r) for m in ok]), np.stack([zm.box(m, r) for m in live])


@pytest.mark.parametrize("cost,r", bb.COST_RADII)
def test_mirror_against_a_loop(oracle, cost, r):
    c = bb.crafted()
    delta = c.offsets(oracle)
    counted, costs = _stacked(cost, r)
    n = counted.sum(0)
    D, H, W = n.shape
    cells = [(0, 0, 0), (3, 0, W - 1), (5, H - 1, 0), (D - 1, H - 1, W - 1),           # the frame's corners (three of them beside a NaN)
             (2, 10, 32), (3, 9, 33), (4, 7, 63),                                      # beside the NaNs at (10, 33) and (7, 64)
             (1, 8, 29), (3, 9, 30), (5, 9, 29),                                       # across the prior's step (rows 9.., columns 30..)
             (0, 4, 20), (6, 4, 21), (3, 12, 19), (3, 12, 22), (0, 3, 21), (6, 3, 20),  # in and beside the +-0.995 columns
             (2, 3, 8), (4, 5, 12),                                                    # in and beside the background block
             (3, 12, 50), (2, 17, 66), (5, 18, 68)]                                    # the i.i.d. block; the tile rest (columns 64.., rows 16..)
    for d, row, col in cells:
        for keep in (1, 2, 3, 8, KEEP_ALL):
            nb, cb, cell = bbm.brute_cell(oracle, cost, *c.views(), c.prior, delta[d], r, keep, row, col)
            assert nb == n[d, row, col] and cb == [int(x) for x in costs[:, d, row, col][counted[:, d, row, col]]], (d, row, col)
            assert cell == int(bb.crafted_volume(cost, r, keep)[d, row, col]), (d, row, col, keep)
    for d, row, col in cells[:6]:
        assert bbm.brute_cell(oracle, cost, *c.views(), c.prior, delta[d], r, 2, row, col, views=range(1, 4))[2] == int(bb.crafted_volume(cost, r, 2, (1, 2, 3))[d, row, col])


@pytest.mark.parametrize("cost,r", bb.COST_RADII)
def test_crafted_case_holds_what_it_is_for(oracle, cost, r):
    c = bb.crafted()
    delta = c.offsets(oracle)
    z, live = bm.planes(c.prior, delta)
    counted, costs = _stacked(cost, r)
    n = counted.sum(0)
    has = bm.inside(c.prior)
    # rule 1: pixels without a prior, dead planes of pixels with one, and nothing counted on either
    assert (~has).sum() >= 30 and (has[None] & ~live).mean() >= 0.01 and live.mean() >= 0.5
    assert not counted[:, ~live].any()
    # views 3 and 4 are the main camera: in frame wherever the plane is live
    ok3, members, alive = _member_counts(oracle, cost, r, 3)
    assert (ok3 != 0).sum() == live.sum()
    if r > 0:
        # rule 3: cells whose centre is live while a window member inside the frame is dead: both counts non-zero
        dead_member = live & (members < zm.box(np.ones_like(c.prior, np.int64), r)[None])
        whole = live & (members == (2 * r + 1) ** 2)
        print("%s r = %d: %d cells with a dead member, %d with a whole window" % (bb.NAMES[cost], r, dead_member.sum(), whole.sum()))
        assert dead_member.sum() > 0 and (whole.sum() > 0 or r == 4)
        assert (dead_member & counted[3]).sum() > 0, "a view counted on a window with a dead member"
    for keep in (1, 2, 3):
        vol = bb.crafted_volume(cost, r, keep)
        assert (n > keep).sum() > 0, "cells with n > keep"
        assert ((vol >> 24) == np.minimum(n, keep)).all() and (vol[n == 0] == 0).all()
    # views 3 and 4 count wherever the plane is live, so cells with 0 < n < keep are those of a range without them, which the device tests run
    n01 = counted[:2].sum(0)
    assert (n01 == 1).sum() > 0 and (n01 == 2).sum() > 0 and (live & (n01 == 0)).sum() > 0
    if cost == ZNCC:
        # views dropped for a flat patch: the centre's sample is in frame, va = 0 (the constant block) or vb = 0 (the saturated band)
        ok0 = _member_counts(oracle, cost, r, 0)[0] != 0
        flat3, flat0 = (ok3 != 0) & ~counted[3], ok0 & ~counted[0]
        print("zncc r = %d: %d cells of view 3 and %d of view 0 dropped for a flat patch" % (r, flat3.sum(), flat0.sum()))
        assert flat0.sum() > 0 and (flat3.sum() > 0 or r == 4)          # (the 7 x 9 constant block holds no 9 x 9 window)
        assert (costs[3][counted[3]] == 0).all() and (costs[4][counted[4]] == 65024).all()
    # the volumes of disjoint view ranges add with MVS_KEEP_ALL and only with it
    np.testing.assert_array_equal(bb.crafted_volume(cost, r, KEEP_ALL, (0, 1)) + bb.crafted_volume(cost, r, KEEP_ALL, (2, 3, 4)), bb.crafted_volume(cost, r, KEEP_ALL))
    assert (bb.crafted_volume(cost, r, 2, (0, 1)) + bb.crafted_volume(cost, r, 2, (2, 3, 4)) != bb.crafted_volume(cost, r, 2)).any()


@pytest.mark.parametrize("cost,r", bb.COST_RADII)
def test_identity_a_a_zero_prior_is_the_global_best_k(oracle, cost, r):
    c = zc.crafted()
    prior = np.zeros((c.H, c.W), np.float32)
    delta = c.planes(oracle)
    for keep in (2, KEEP_ALL):
        got = bbm.volume(oracle, cost, *c.views(), prior, delta, r, keep)
        np.testing.assert_array_equal(got, bk.crafted_volume(cost, r, keep, range(5)))


def test_identity_b_single_pixel_absdiff_is_the_band_sweep(oracle):
    c = bb.crafted()
    ref = bm.band_volume(oracle, *c.views(), c.prior, c.offsets(oracle))
    np.testing.assert_array_equal(bb.crafted_volume(ABSDIFF, 0, KEEP_ALL), ref)
    b = bc.crafted()                       # and on the band sweep's own crafted case, against its committed reference
    got = bbm.volume(oracle, ABSDIFF, *b.views(), b.prior, bc.offsets(oracle, b.D, b.HB), 0, KEEP_ALL)
    np.testing.assert_array_equal(got, bc.crafted_volume())


@pytest.mark.parametrize("r", zc.RADII)
def test_identity_c_zncc_on_a_zero_prior_is_the_zncc_sweep(oracle, r):
    c = zc.crafted()
    got = bbm.volume(oracle, ZNCC, *c.views(), np.zeros((c.H, c.W), np.float32), c.planes(oracle), r, KEEP_ALL)
    np.testing.assert_array_equal(got, zc.crafted_volume(r))


FILTER = dict(radius=4, tau=40, max_steps=8.0)


def test_two_levels_on_a_filtered_prior_beat_the_global_zncc_sweep_at_equal_samples(oracle):
    """DESIGN.md section 21 set the criterion: two levels with a ZNCC band level beat 48 global ZNCC planes on the exposure scene's
    bad-pixel share at equal samples.  160 x 100, the gains, radius 3; bad: more than 1.5 steps of the 48-plane table from the analytic
    depth, on the refined maps.  Only the comparison is asserted; section 24 records the values."""
    views, truth = bb.exposure_views(160, 100)
    step = 2.0 / 48
    ref = bb.quality(bb.global_level(oracle, views, 48, -1.0, 1.0, ZNCC, 3, KEEP_ALL)[1], truth, step)
    two = bb.two_levels(oracle, views, 16, 32, ZNCC, 3, KEEP_ALL, FILTER)
    got = bb.quality(two[4], truth, step)
    print("160 x 100: 48 global ZNCC planes %.2f %% bad, median %.4f; 16 + 32 on the filtered prior %.2f %% bad, median %.4f" % (
        100 * ref[0], ref[1], 100 * got[0], got[1]))
    assert got[0] < ref[0]


def test_figures_of_section_24(oracle):
    """the rest of section 24's table, printed: the exposure scene at 96 x 64 and 160 x 100 on raw and filtered priors, the filtered
    coarse prior alone, and best-K in the band on section 22's occluder scene.  The one assertion is the documented warning, kept honest:
    on a RAW prior the windowed band is worse than the global sweep at equal samples"""
    step = 2.0 / 48
    fig = {}
    for W, H in ((96, 64), (160, 100)):
        views, truth = bb.exposure_views(W, H)
        for D in (48, 128):
            fig[W, "%d global" % D] = bb.quality(bb.global_level(oracle, views, D, -1.0, 1.0, ZNCC, 3, KEEP_ALL)[1], truth, step)
        for DB in (16, 32):
            for name, filter in (("raw", None), ("filtered", FILTER)):
                two = bb.two_levels(oracle, views, 16, DB, ZNCC, 3, KEEP_ALL, filter)
                fig[W, "16 + %d %s" % (DB, name)] = bb.quality(two[4], truth, step)
                if DB == 16 and filter:
                    fig[W, "filtered 16-plane prior alone"] = bb.quality(two[1], truth, step)
    for (W, name), (bad, med) in fig.items():
        print("exposure scene, width %3d: %-30s %5.2f %% bad, median %.4f" % (W, name, 100 * bad, med))
    for W in (96, 160):
        assert fig[W, "16 + 32 raw"][0] > fig[W, "48 global"][0]
    o = bk.occluder()
    views, ostep = o.views(), (o.z_hi - o.z_lo) / 48
    for keep in (KEEP_ALL, 2):
        glob = bb.global_level(oracle, views, 48, o.z_lo, o.z_hi, ZNCC, 2, keep)[1]
        two = bb.two_levels(oracle, views, 16, 32, ZNCC, 2, keep, dict(radius=2, tau=40, max_steps=8.0), o.z_lo, o.z_hi)[4]
        for name, depth in (("48 global", glob), ("16 + 32 filtered", two)):
            bad = np.abs(depth - o.truth) > 1.5 * ostep
            print("occluder scene, keep %-3s %-18s %5.2f %% bad of the image, %5.2f %% of the edge" % (keep or "all", name, 100 * bad.mean(), 100 * bad[o.edge].mean()))
