"""The resolution pyramid's contract on the CPU: the mirror (tests/pyramid_mirror.py) against scalar loops written
from the rules, a crafted depth step along a guide edge, and what a half-resolution coarse level buys on the synthetic scene."""
import functools

import numpy as np

import pyramid_cases as pc
import pyramid_mirror as pm
from mvs_amd import synth

F = np.float32


def _downsample_loops(f):
    H, W = f.shape
    out = np.zeros((H // 2, W // 2), np.uint8)
    for r in range(H // 2):
        for c in range(W // 2):
            out[r, c] = (int(f[2 * r, 2 * c]) + int(f[2 * r, 2 * c + 1]) + int(f[2 * r + 1, 2 * c]) + int(f[2 * r + 1, 2 * c + 1]) + 2) >> 2
    return out


def _prior_loops(zc, tau, gc, gf):
    """rule U a pixel and a tap at a time"""
    Hc, Wc = zc.shape
    out = np.zeros((2 * Hc, 2 * Wc), np.float32)
    for r in range(2 * Hc):
        for c in range(2 * Wc):
            r0, c0 = (r - 1) >> 1, (c - 1) >> 1
            rows = (min(max(r0, 0), Hc - 1), min(max(r0 + 1, 0), Hc - 1))
            cols = (min(max(c0, 0), Wc - 1), min(max(c0 + 1, 0), Wc - 1))
            wy = (3, 1) if r & 1 else (1, 3)
            wx = (3, 1) if c & 1 else (1, 3)
            taps = [(rows[i], cols[j], wy[i] * wx[j]) for i in (0, 1) for j in (0, 1)]
            valid = [t for t in taps if -1.0 < zc[t[0], t[1]] < 1.0]
            members = valid
            if tau < 255:
                like = [t for t in valid if abs(int(gc[t[0], t[1]]) - int(gf[r, c])) <= tau]
                members = like if like else valid
            if not members:
                out[r, c] = 1.0
                continue
            num = None
            for tr, tc, w in members:
                p = F(w) * zc[tr, tc]
                num = p if num is None else F(num + p)
            z = F(num / F(sum(t[2] for t in members)))
            out[r, c] = z if -1.0 < z < 1.0 else 1.0
    return out


def _same_floats(got, ref, what):
    np.testing.assert_array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(ref, np.float32).view(np.uint32), err_msg=what)


def test_rule_d_against_loops():
    rng = np.random.Generator(np.random.PCG64(11))
    for H, W in ((2, 2), (6, 10), (42, 70)):
        f = rng.integers(0, 256, (H, W), dtype=np.uint8)
        np.testing.assert_array_equal(pm.downsample(f), _downsample_loops(f))
    f = np.array([[255, 255], [255, 255]], np.uint8)
    assert pm.downsample(f)[0, 0] == 255
    assert pm.downsample(np.array([[0, 1], [0, 0]], np.uint8))[0, 0] == 0 and pm.downsample(np.array([[1, 1], [0, 0]], np.uint8))[0, 0] == 1
    stack = rng.integers(0, 256, (3, 8, 12), dtype=np.uint8)
    np.testing.assert_array_equal(pm.downsample(stack), np.stack([_downsample_loops(s) for s in stack]))


def test_rule_u_against_loops():
    rng = np.random.Generator(np.random.PCG64(12))
    for Hc, Wc in ((1, 1), (2, 3), (9, 13)):
        for trial in range(3):
            zc = rng.uniform(-1.2, 1.2, (Hc, Wc)).astype(np.float32)
            bad = rng.random((Hc, Wc))
            zc[bad < 0.10] = 1.0
            zc[(bad >= 0.10) & (bad < 0.15)] = -1.0
            zc[(bad >= 0.15) & (bad < 0.22)] = np.nan
            gc = rng.integers(0, 256, (Hc, Wc), dtype=np.uint8)
            gf = rng.integers(0, 256, (2 * Hc, 2 * Wc), dtype=np.uint8)
            for tau in (255, 254, 60, 20, 3, 0):
                _same_floats(pm.prior(zc, tau, gc, gf), _prior_loops(zc, tau, gc, gf), "%d x %d, trial %d, tau %d" % (Wc, Hc, trial, tau))
    c = pc.crafted_prior()
    for tau in (255, 20, 0):
        _same_floats(pm.prior(c.depth, tau, c.coarse_guide, c.fine_guide), _prior_loops(c.depth, tau, c.coarse_guide, c.fine_guide), "crafted, tau %d" % tau)
    # tau = 255 reads no guide
    _same_floats(pm.prior(c.depth), pm.prior(c.depth, 255, c.coarse_guide, c.fine_guide), "tau 255 without guides")


def test_rule_u_weights_and_borders():
    """a constant map stays constant wherever a tap is valid; the weights are 9-3-3-1 / 16; clamped taps keep their weight"""
    z = np.full((3, 4), 0.25, np.float32)
    _same_floats(pm.prior(z), np.full((6, 8), 0.25, np.float32), "constant")
    z = np.zeros((2, 2), np.float32)
    z[0, 0] = 0.5
    up = pm.prior(z)
    assert up[1, 1] == F(9 * 0.5 / 16) and up[1, 2] == F(3 * 0.5 / 16) and up[2, 1] == F(3 * 0.5 / 16) and up[2, 2] == F(0.5 / 16)
    assert up[0, 0] == F(0.5) and up[0, 1] == F(0.5 * 12 / 16) and up[0, 2] == F(0.5 * 4 / 16)   # row 0: both row taps are coarse row 0
    # invalid taps drop out of numerator and denominator
    z = np.array([[0.5, 1.0], [np.nan, -1.0]], np.float32)
    up = pm.prior(z)
    assert (up[:3, :3] == F(0.5)).all() and (up[3, :] == 1.0).all() and (up[:, 3] == 1.0).all()   # the last row and column tap invalid pixels only
    assert (pm.prior(np.full((2, 2), 1.0, np.float32)) == 1.0).all()
    # a mean that leaves (-1, 1) cannot happen from members inside it; an input outside is no tap at all
    z = np.array([[1.5, 0.25]], np.float32)
    up = pm.prior(z)
    assert (up[:, 1:] == F(0.25)).all() and (up[:, 0] == 1.0).all()


def test_depth_step_along_a_guide_edge():
    """coarse depths -0.5 | +0.5 with the step at coarse column 8 (fine column 16), guides 50 | 200 with the same edge: plain bilinear
    (tau = 255) smears the step over the fine columns next to it, the guided rule (tau = 20) keeps every prior pixel at one of the two
    depths"""
    Hc, Wc = 6, 16
    z = np.where(np.arange(Wc)[None, :] < 8, F(-0.5), F(0.5)).repeat(Hc, 0).astype(np.float32)
    gc = np.where(np.arange(Wc)[None, :] < 8, 50, 200).repeat(Hc, 0).astype(np.uint8)
    gf = np.where(np.arange(2 * Wc)[None, :] < 16, 50, 200).repeat(2 * Hc, 0).astype(np.uint8)
    plain = pm.prior(z, 255)
    between = (plain > -0.5) & (plain < 0.5)
    assert between.any() and set(np.nonzero(between)[1]) == {15, 16}
    guided = pm.prior(z, 20, gc, gf)
    assert not ((guided > -0.5) & (guided < 0.5)).any()
    np.testing.assert_array_equal(guided, np.where(np.arange(2 * Wc)[None, :] < 16, F(-0.5), F(0.5)).repeat(2 * Hc, 0))


def test_same_cameras_serve_every_level():
    main_a, sides_a = synth.ring_cameras(4, 160, 100)
    main_b, sides_b = synth.ring_cameras(4, 80, 50)
    np.testing.assert_array_equal(main_a, main_b)
    np.testing.assert_array_equal(sides_a, sides_b)
    # the centre of a coarse pixel is the mean of the centres of its fine pixels
    xf = (2 * np.arange(160) + 1) / 160.0 - 1
    np.testing.assert_allclose((xf[0::2] + xf[1::2]) / 2, (2 * np.arange(80) + 1) / 80.0 - 1, rtol=0, atol=1e-15)


@functools.lru_cache(maxsize=None)
def _scene(freq_scale):
    """160 x 100, 4 ring views, 16 + 16 planes, +-1.5 steps -> (median, RMSE) of the same-resolution two-level sequence, the two-level
    pyramid and the 128-plane sweep; only what a condition below needs is computed"""
    import orc
    oracle = orc.load()
    W, H, V, DC, DB = 160, 100, 4, 16, 16
    main_cam, main_img, side_cams, sides, truth = synth.make_views(W, H, V, freq_scale=freq_scale)

    def errors(depth):
        e = depth.astype(np.float64) - truth
        return float(np.median(np.abs(e))), float(np.sqrt(np.mean(e * e)))

    out = {"pyramid": errors(pc.coarse_to_fine(oracle, main_cam, main_img, side_cams, sides, 2, DC, DB)[0])}
    if freq_scale is not None:
        coarse = pc.refined_sweep(oracle, main_cam, main_img, side_cams, sides, DC)
        out["same"] = errors(pc.band_level(oracle, main_cam, main_img, side_cams, sides, coarse, DB, float(np.float32(1.5 * 2.0 / DC)))[0])
    else:
        out["dense"] = errors(pc.refined_sweep(oracle, main_cam, main_img, side_cams, sides, 128))
    return out


def test_pyramid_on_high_frequency_texture():
    """freq_scale = 1.0 (wavelengths of a few pixels at 160 x 100): the coarse level at half resolution finds the right plane where the
    same-resolution coarse level under-samples the cost curve.  Condition: RMSE <= 0.5 x the same-resolution two-level's and median <=
    its median.  Measured with this mirror (f32 rule U): see the printed line and the README."""
    e = _scene(1.0)
    print("freq_scale 1.0: same-resolution two-level median %.5f RMSE %.4f; pyramid median %.5f RMSE %.4f (RMSE ratio %.2f)" % (
        e["same"] + e["pyramid"] + (e["pyramid"][1] / e["same"][1],)))
    assert e["pyramid"][1] <= 0.5 * e["same"][1]
    assert e["pyramid"][0] <= e["same"][0]


def test_pyramid_on_the_default_scene():
    """the smooth default scene loses nothing: pyramid median <= 1.10 x the 128-plane sweep's"""
    e = _scene(None)
    print("default scene: pyramid median %.5f RMSE %.4f; 128 planes median %.5f RMSE %.4f (median ratio %.2f)" % (
        e["pyramid"] + e["dense"] + (e["pyramid"][0] / e["dense"][0],)))
    assert e["pyramid"][0] <= 1.10 * e["dense"][0]
