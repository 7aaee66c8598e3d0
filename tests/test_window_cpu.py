"""The windowed matching cost without a GPU: the numpy mirror (tests/window_mirror.py) on the crafted volumes of
tests/window_volumes.py, against a pixel-by-pixel restatement, and behind the oracle's sweep, where it has to buy what it is there for."""
import functools

import numpy as np
import pytest

import mvs_amd
import sgm_mirror as sgm
import window_mirror as wm
import window_volumes as wv
from mvs_amd import synth

EINVAL = -1


def _slow_window(vol, cs, radius, tau, guide):
    """the contract read aloud, a cell at a time"""
    D, H, W = vol.shape
    M = (1 << cs) - 1
    out = np.zeros((D, H, W), np.uint32)
    for d in range(D):
        for y in range(H):
            for x in range(W):
                n = int(vol[d, y, x]) >> cs
                if n == 0:
                    continue
                S = N = 0
                for qy in range(max(0, y - radius), min(H, y + radius + 1)):
                    for qx in range(max(0, x - radius), min(W, x + radius + 1)):
                        if tau < 255 and abs(int(guide[qy, qx]) - int(guide[y, x])) > tau:
                            continue
                        c = int(vol[d, qy, qx])
                        if c >> cs:
                            S += c & M
                            N += c >> cs
                out[d, y, x] = (n << cs) | ((S * n) // N)
    return out


@pytest.mark.parametrize("cs", [24, 16])
@pytest.mark.parametrize("radius,tau", [(1, 255), (2, 20), (4, 0), (4, 255)])
def test_mirror_is_the_contract(cs, radius, tau):
    W, H, D = 7, 5, 2
    vol, guide = wv.noise(W, H, D, cs), wv.guide_levels(W, H)
    np.testing.assert_array_equal(wm.window(vol, cs, radius, tau, guide), _slow_window(vol, cs, radius, tau, guide))


@pytest.mark.parametrize("cs", [24, 16])
def test_radius_0_is_the_identity_on_proper_cells(cs):
    vol = wv.noise(65, 9, 5, cs)
    s, n = wm.split(vol, cs)
    assert ((n == 0) & (s != 0)).any() and (n == 0).mean() > 0.2, "the case needs unseen cells with a sum field"
    out = wm.window(vol, cs, 0, 20, wv.guide_levels(65, 9))
    np.testing.assert_array_equal(out[n > 0], vol[n > 0])
    assert (out[n == 0] == 0).all()
    for radius in (1, 4):   # an unseen cell stays unseen, a seen one keeps its count, at every radius
        out = wm.window(vol, cs, radius)
        assert (out[n == 0] == 0).all()
        np.testing.assert_array_equal(wm.split(out, cs)[1], n)


@pytest.mark.parametrize("cs", [24, 16])
def test_extremes(cs):
    W, H, D = 65, 9, 2
    full = wv.full(W, H, D, cs)
    s, n = wm.split(full, cs)
    assert int(n[0, 0, 0]) == wv.MAX_VIEWS[cs] and int(s[0, 0, 0]) == wv.MAX_VIEWS[cs] * wv.PER_SAMPLE[cs]
    if cs == 24:
        assert 81 * int(s[0, 0, 0]) * int(n[0, 0, 0]) >= 1 << 38      # S n: the 40-bit product, far past 32 bits
    for radius in (1, 4):
        np.testing.assert_array_equal(wm.window(full, cs, radius), full)   # the mean of equal cells is the cell
    const = wv.constant(W, H, D, cs)
    np.testing.assert_array_equal(wm.window(const, cs, 4), const)
    # counts that vary per pixel and plane, 30 % unseen: the quotient stays inside the field and below the largest mean of the window
    vol = wv.noise(W, H, 5, cs)
    s, n = wm.split(vol, cs)
    assert 0.25 < (n == 0).mean() < 0.35 and len(np.unique(n)) > 20
    so, no = wm.split(wm.window(vol, cs, 4), cs)
    assert (so <= no * wv.PER_SAMPLE[cs]).all()


def test_constant_volume_ties_to_plane_0(oracle):
    W, H, D = 65, 9, 5
    out = wm.window(wv.constant(W, H, D, 24), 24, 2)
    _, _, index = oracle.argmin(out, oracle.plane_table(D, -1.0, 1.0), sampler="fixed")
    assert (index == 0).all()


def test_checkerboard_and_constant_guides():
    W, H, D, cs = 65, 9, 5, 24
    vol = wv.noise(W, H, D, cs)
    box = wm.window(vol, cs, 2)
    np.testing.assert_array_equal(wm.window(vol, cs, 2, 0, wv.guide_constant(W, H)), box)
    gated = wm.window(vol, cs, 2, 0, wv.guide_checkerboard(W, H))
    assert (gated != box).any()
    # same-colour pixels only: the window of a volume that lives on one colour alone sees that colour's cells or nothing but its own
    y, x = np.mgrid[0:H, 0:W]
    black = (x + y) % 2 == 0
    s, n = wm.split(vol, cs)
    one_colour = np.where(black[None], vol, 0).astype(np.uint32)
    np.testing.assert_array_equal(wm.window(one_colour, cs, 2, 0, wv.guide_checkerboard(W, H))[:, black], gated[:, black])
    other = np.where(black[None], 0, vol).astype(np.uint32)
    np.testing.assert_array_equal(wm.window(other, cs, 2, 0, wv.guide_checkerboard(W, H))[:, ~black], gated[:, ~black])


def _index(vol, cs):
    """mvs_sweep_argmin's rule in numpy: lowest mean cost as an exact rational, ties to the lowest plane"""
    s, n = wm.split(vol, cs)
    D, H, W = s.shape
    bi, bs, bn = -np.ones((H, W), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for d in range(D):
        better = (n[d] > 0) & ((bi < 0) | (s[d] * bn < bs * n[d]))
        bi, bs, bn = np.where(better, d, bi), np.where(better, s[d], bs), np.where(better, n[d], bn)
    return bi


def test_step_case():
    """a condition, not a measurement: within 3 columns of the depth step the gated 5 x 5 window (tau 20) has at most half the box's bad
    pixels; away from the step both have at most 1 %.  (Mirror: 1.0 % against 10.9 % near the step, 0.1 % for both away from it; the raw
    volume has 85 % bad pixels everywhere.)"""
    vol, guide, truth, near = wv.step_case()
    bad_box = _index(wm.window(vol, 24, 2), 24) != truth
    bad_gate = _index(wm.window(vol, 24, 2, 20, guide), 24) != truth
    bad_raw = _index(vol, 24) != truth
    print("step case, bad pixels near / away: raw %.4f / %.4f, box %.4f / %.4f, gated %.4f / %.4f"
          % (bad_raw[near].mean(), bad_raw[~near].mean(), bad_box[near].mean(), bad_box[~near].mean(), bad_gate[near].mean(), bad_gate[~near].mean()))
    assert bad_box[near].mean() > 0.05, "the case needs a box that straddles the step"
    assert bad_gate[near].mean() <= 0.5 * bad_box[near].mean()
    assert bad_box[~near].mean() <= 0.01 and bad_gate[~near].mean() <= 0.01
    assert bad_raw.mean() > 0.5


# ---- behind the oracle's sweep -----------------------------------------------------------------------------------------------------
QW, QH, QV, QD = 96, 64, 4, 32


@functools.lru_cache(maxsize=None)
def _quality_scene():
    import orc
    oracle = orc.load()
    main_cam, main_img, side_cams, sides, truth = synth.make_views(QW, QH, QV, radius=0.3)
    z_lo, z_hi = float(truth.min()) - 0.01, float(truth.max()) + 0.01
    vol = oracle.sweep(main_cam, main_img, side_cams, sides, QD, z_lo, z_hi, want_volume=True, sampler="fixed")[3]
    return oracle, vol, main_img, truth, oracle.plane_table(QD, z_lo, z_hi)


def _quality(depth, truth, z):
    step = abs(float(z[1]) - float(z[0]))
    err = np.abs(depth.astype(np.float64) - truth.astype(np.float64)) / step
    return float((err > 1.0).mean()), float(np.median(err))


def _wta(oracle, vol, z):
    _, _, index = oracle.argmin(vol, z, sampler="fixed")
    return oracle.refine_depth(vol, z, index, sampler="fixed")


def _sgm(vol, z):
    seen = sgm.seen_cells(vol, 24)
    S = sgm.aggregate(sgm.cost16(vol, 24, 4080), 8, 16, 128)
    return sgm.refine(S, seen, z, sgm.select(S, seen, z, 8)[2])


def test_quality_behind_the_oracles_sweep():
    """96 x 64, 4 views, 32 planes over the true depth range +- 0.01; bad = refined depth more than one plane step from the analytic depth.
    The 5 x 5 box's bad-pixel share is at most half the raw volume's (measured: 7.4 % against 21.3 %).  The other rows are printed for
    DESIGN.md section 18 and not asserted."""
    oracle, vol, guide, truth, z = _quality_scene()
    raw = _quality(_wta(oracle, vol, z), truth, z)
    rows = [("raw (winner-take-all)", raw)]
    for radius in (1, 2):
        rows.append(("%d x %d box window" % (2 * radius + 1, 2 * radius + 1), _quality(_wta(oracle, wm.window(vol, 24, radius), z), truth, z)))
    rows.append(("5 x 5 window gated by the main image, tau 20", _quality(_wta(oracle, wm.window(vol, 24, 2, 20, guide), z), truth, z)))
    rows.append(("aggregation (8 paths, 16 / 128) on the raw volume", _quality(_sgm(vol, z), truth, z)))
    rows.append(("aggregation on the 5 x 5 box window", _quality(_sgm(wm.window(vol, 24, 2), z), truth, z)))
    for name, (bad, med) in rows:
        print("%-52s %5.1f %% bad   median %.2f steps" % (name, 100 * bad, med))
    assert rows[2][1][0] <= 0.5 * raw[0], rows


def test_null_context_is_einval_without_a_device():
    lib = mvs_amd.load_library()
    assert lib.mvs_sweep_window(None, 2, 255, None, 0) == EINVAL
    assert lib.mvs_sweep_set_volume_source(None, 0) == EINVAL
    assert lib.mvs_sweep_volume_source(None) == EINVAL
    assert lib.mvs_sweep_window_fetch(None, None) == EINVAL
    assert not lib.mvs_sweep_windowed_device(None, None)
