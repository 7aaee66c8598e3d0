"""The band sweep's contract on the CPU: the mirror (tests/band_mirror.py) against the oracle where the two must
agree, the crafted case's own premises, and what two levels buy on the synthetic scene."""
import functools

import numpy as np

import band_cases as bc
import band_mirror as bm
from mvs_amd import synth

FIXED = "fixed"


def test_mirror_with_a_zero_prior_is_the_oracles_sweep(oracle):
    """prior = 0: plane d is 0 + delta_d = delta_d, so the band volume is orc_sweep_fx on the plane table (D, -hb, hb), every cell"""
    W, H, D, V, hb = 40, 24, 9, 4, 0.3
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    ref = oracle.sweep(main_cam, main_img, side_cams, sides, D, z_lo=-hb, z_hi=hb, want_volume=True, sampler=FIXED)[3]
    vol = bm.band_volume(oracle, main_cam, main_img, side_cams, sides, np.zeros((H, W), np.float32), bc.offsets(oracle, D, hb))
    assert (vol >> 24).max() == V and len(np.unique(vol)) > 100
    assert int(np.count_nonzero(vol != ref)) == 0
    # the views add, as the packed cells of the ordinary sweep do
    parts = [bm.band_volume(oracle, main_cam, main_img, side_cams, sides, np.zeros((H, W), np.float32), bc.offsets(oracle, D, hb), views=v) for v in ([0, 1], [2, 3])]
    np.testing.assert_array_equal(parts[0] + parts[1], ref)


def test_mirror_samples_through_the_oracles_wrapper(oracle):
    """band_volume binds orc_sweep_sample_fx itself (speed); cell by cell it is what oracle.sweep_sample_fx gives"""
    c = bc.crafted()
    vol = bc.crafted_volume()
    z, live = bm.planes(c.prior, bc.offsets(oracle, c.D, c.HB))
    qs = [oracle.view_matrix(c.main_cam, c.side_cams[v], c.W, c.H) for v in range(c.V)]
    pads = [oracle.pad_image(s) for s in c.sides]
    rng = np.random.Generator(np.random.PCG64(5))
    for d, r, col in zip(rng.integers(0, c.D, 300), rng.integers(0, c.H, 300), rng.integers(0, c.W, 300)):
        cell = 0
        if live[d, r, col]:
            for v in range(c.V):
                ok, dot = oracle.sweep_sample_fx(qs[v], oracle.lib.orc_pixel_xn(int(col), c.W), oracle.lib.orc_pixel_yn(int(r), c.H), float(z[d, r, col]), pads[v])
                if ok:
                    cell += (1 << 24) + abs(dot - 255 * int(c.main_img[r, col]))
        assert vol[d, r, col] == cell, (d, r, col)


def test_crafted_case_meets_its_conditions(oracle):
    c = bc.crafted()
    vol = bc.crafted_volume()
    count = vol >> 24
    _, live = bm.planes(c.prior, bc.offsets(oracle, c.D, c.HB))
    has = bm.inside(c.prior)
    empty = float(np.mean(count == 0))
    print("cells with count 0: %.3f; 0 < count < V: %.3f; dead planes on pixels with a prior: %d; pixels without a prior: %d" % (
        empty, float(np.mean((count > 0) & (count < c.V))), int((~live & has[None]).sum()), int((~has).sum())))
    assert 0.05 <= empty <= 0.60
    assert ((count > 0) & (count < c.V)).any() and (count == c.V).any()
    assert (~live & has[None]).any()               # dead planes on pixels with a prior
    assert (~has).any() and np.isnan(c.prior).any() and (c.prior == 1.0).any()
    assert (vol[~live] == 0).all()
    assert c.D % 16 == 3 and c.W % 32 == 6 and c.H % 8 == 3
    # the selection sees pixels with and without an index, and every plane range
    depth, cost, index = oracle.argmin(vol, bc.offsets(oracle, c.D, c.HB), sampler=FIXED)
    assert (index < 0).any() and (index == 0).any() and (index == c.D - 1).any() and (index >= 16).any()
    rep = bm.report(c.prior, depth, index, c.D)
    assert rep[0] == int(has.sum()) and 0 < rep[2] < rep[1] <= rep[0] and rep[3] == 0


def test_resolve_and_report():
    prior = np.array([[0.5, 0.99, np.nan, 1.0, -0.99, 0.0]], np.float32)
    off = np.array([[0.25, 0.25, 0.0, 0.0, -0.25, 1.0]], np.float32)
    index = np.array([[3, 7, 0, -1, 0, -1]], np.int32)
    z = bm.resolve(prior, off, index)
    np.testing.assert_array_equal(z, np.array([[0.75, 1.0, 1.0, 1.0, 1.0, 1.0]], np.float32))
    assert bm.report(prior, off, index, 8) == [4, 4, 3, 3]


@functools.lru_cache(maxsize=None)
def _two_levels():
    import orc
    oracle = orc.load()
    W, H, V, DC, DB, hb = 160, 100, 4, 16, 16, 0.1875
    main_cam, main_img, side_cams, sides, truth = synth.make_views(W, H, V)

    def median_error(depth):
        return float(np.median(np.abs(depth.astype(np.float64) - truth)))

    def refined_sweep(D):
        _, _, index, vol = oracle.sweep(main_cam, main_img, side_cams, sides, D, want_volume=True, nthreads=4, sampler=FIXED)
        return oracle.refine_depth(vol, oracle.plane_table(D, -1.0, 1.0), index, sampler=FIXED)

    coarse = refined_sweep(DC)
    delta = bc.offsets(oracle, DB, hb)
    vol = bm.band_volume(oracle, main_cam, main_img, side_cams, sides, coarse, delta)
    _, _, index = oracle.argmin(vol, delta, sampler=FIXED)
    band = bm.resolve(coarse, oracle.refine_depth(vol, delta, index, sampler=FIXED), index)
    return median_error(coarse), median_error(band), median_error(refined_sweep(128)), bm.report(coarse, oracle.refine_depth(vol, delta, index, sampler=FIXED), index, DB)


def test_coarse_to_fine_reaches_the_dense_sweeps_median_error():
    """160 x 100, 4 ring views: 16 planes over [-1, 1], refined, then 16 planes within +-1.5 coarse steps of that map, refined and
    resolved: 32 plane samples per pixel.  Measured: coarse 0.00801, band 0.00508 (0.63 of the coarse), 128 planes 0.00536 (band / dense
    0.95).  The arithmetic is deterministic; the margins cover nothing but a different reading of the contract."""
    coarse, band, dense, rep = _two_levels()
    print("median |depth - truth|: coarse %.5f, band %.5f (%.2f of the coarse), 128 planes %.5f (band / dense %.2f); report %s" % (
        coarse, band, band / coarse, dense, band / dense, rep))
    assert band <= 0.75 * coarse
    assert band <= 1.10 * dense
