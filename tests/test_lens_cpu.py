"""The lens contract without a GPU: tests/lens_mirror.py against a scalar restatement, its crafted properties
(identity, replicated border, saturation), the reference's cameraToScreen expression, the binding, and what undistorting buys the sweep
(oracle sweep on lens frames as they are, undistorted, and pinhole)."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import lens_mirror
import lens_scenes
import mvs_amd
from mvs_amd import synth


# ---- scalar restatement: Python floats (double) rounded to float32 after every operation; ints for the sampler --------------------------
def r32(x):
    """round a double to the nearest float32 (ties to even).  For one +, -, * or / of two float32 values the double result rounded again
    to float32 equals the correctly rounded float32 result (53 >= 2 * 24 + 2)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def fma32(a, b, c):
    """RN32(a b + c), exactly: the rational value, then the nearer of the float32 neighbours of its double rounding (ties to even)"""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    guess = np.float32(float(exact))
    cands = {float(guess), float(np.nextafter(guess, np.float32(-np.inf))), float(np.nextafter(guess, np.float32(np.inf)))}
    def key(v):
        even = (struct.unpack("I", struct.pack("f", v))[0] & 1) == 0
        return (abs(Fraction(v) - exact), 0 if even else 1)
    return min(cands, key=key)


def scalar_position(W, H, k, center, row, col):
    cx, cy = lens_mirror.center_of(W, H, center)
    k1, k2, k3 = [float(v) for v in lens_mirror.k_of(k)]
    a = r32(float(H) / float(W))
    hc = r32(float(H) - r32(cy))
    xn = fma32(float(2 * col + 1), r32(1.0 / W), -1.0)
    yn = fma32(-float(2 * row + 1), r32(1.0 / H), 1.0)
    r2 = r32(r32(r32(xn * xn) + r32(r32(r32(yn * yn) * a) * a)) * 0.25)
    kf = r32(1.0 + r32(r2 * r32(k1 + r32(r2 * r32(k2 + r32(r2 * k3))))))
    X = r32(r32(cx) + r32(r32(r32(xn * kf) * float(W)) * 0.5))
    Y = r32(hc - r32(r32(r32(yn * kf) * float(H)) * 0.5))
    return r32(X - 0.5), r32(Y - 0.5)


def round_half_even(v):
    f = int(np.floor(v))
    d = v - f
    return f + (1 if d > 0.5 or (d == 0.5 and (f & 1)) else 0)


def scalar_sample(frame, table, mx, my):
    H, W = frame.shape
    qx, qy = round_half_even(mx * 32.0), round_half_even(my * 32.0)
    sx, sy = (qx >> 5) - 1, (qy >> 5) - 1
    w = table[(qy & 31) * 32 + (qx & 31)]
    total = 0
    for k1 in range(4):
        for k2 in range(4):
            yy, xx = min(max(sy + k1, 0), H - 1), min(max(sx + k2, 0), W - 1)
            total += int(frame[yy, xx]) * int(w[k1 * 4 + k2])
    return min(max((total + (1 << 14)) >> 15, 0), 255)


def test_the_mirrors_table_is_the_oracles(oracle):
    np.testing.assert_array_equal(lens_mirror.cubic_table(), oracle.cubic_table())
    t = lens_mirror.cubic_table().astype(np.int64)
    assert (t.sum(axis=1) == 32768).all()
    # fraction (0, 0): the pixel itself -- 32767 (int16 saturates) on it and the missing 1 on its diagonal neighbour, which cannot move
    # the result: (32767 p + p' + 16384) >> 15 = p for any two bytes p, p'
    assert t[0].tolist() == [0] * 5 + [32767] + [0] * 4 + [1] + [0] * 5
    p, q = np.mgrid[0:256, 0:256]
    assert (((32767 * p + q + 16384) >> 15) == p).all()


@pytest.mark.parametrize("lens", lens_scenes.LENS_NAMES)
def test_mirror_equals_the_scalar_restatement(lens):
    W, H = 23, 17
    k, c = lens_scenes.lenses(W, H)[lens]
    frame = lens_scenes.noise(W, H, seed=11)
    mx, my = lens_mirror.positions(W, H, k, c)
    out = lens_mirror.sample(frame, mx, my)
    table = lens_mirror.cubic_table()
    for r in range(H):
        for col in range(W):
            sx, sy = scalar_position(W, H, k, c, r, col)
            assert (sx, sy) == (float(mx[r, col]), float(my[r, col])), (r, col)
            assert scalar_sample(frame, table, sx, sy) == int(out[r, col]), (r, col)


def test_the_fma_restatements_agree_where_double_rounding_would_not():
    """a product-sum that lands next to a float32 midpoint: the array form (sgm_mirror._fma32) and the exact scalar form agree"""
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.integers(1, 40000, 2000).astype(np.float32)
    b = (np.float32(1) / rng.integers(3, 9000, 2000).astype(np.float32)).astype(np.float32)
    got = lens_mirror._fma32(a, b, np.full_like(a, np.float32(-1)))
    for i in range(2000):
        assert float(got[i]) == fma32(float(a[i]), float(b[i]), -1.0)


@pytest.mark.parametrize("size", [(23, 17), (67, 35), (640, 480)])
def test_identity_lens_returns_the_input(size):
    W, H = size
    frame = lens_scenes.noise(W, H)
    np.testing.assert_array_equal(lens_mirror.undistort(frame, (0.0, 0.0, 0.0)), frame)


def test_rule_3_without_k3_is_camera_to_screen_bit_for_bit():
    """configuration.cpp:248-259: radSquared = (x x + y y aspect aspect) / 4; k = 1 + radSquared (k0 + radSquared k1), in float"""
    rng = np.random.Generator(np.random.PCG64(17))
    n = 10000
    x = rng.uniform(-1.2, 1.2, n).astype(np.float32)
    y = rng.uniform(-1.2, 1.2, n).astype(np.float32)
    k0 = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    k1 = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    aspect = np.float32(480) / np.float32(640)
    rad = (x * x + y * y * aspect * aspect) / np.float32(4)
    ref = np.float32(1) + rad * (k0 + rad * k1)
    r2 = (x * x + ((y * y) * aspect) * aspect) * np.float32(0.25)
    np.testing.assert_array_equal(r2, rad)
    got = np.float32(1) + r2 * (k0 + r2 * (k1 + r2 * np.float32(0)))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, ref)
    for i in range(0, n, 997):
        assert float(lens_mirror.radial_factor(r2[i], (k0[i], k1[i], 0.0))) == float(ref[i])


def test_replicated_border_on_a_pincushion_frame():
    """all four sides of the pincushion's map lie outside the frame; the sampler equals an unclamped one on an edge-padded frame, and a
    constant frame stays constant (a zero border would darken its rim)"""
    W, H = 67, 35
    k, c = lens_scenes.lenses(W, H)["pincushion"]
    mx, my = lens_mirror.positions(W, H, k, c)
    assert mx.min() < 0 and mx.max() > W - 1 and my.min() < 0 and my.max() > H - 1
    assert (mx[:, 0] < 0).all() and (mx[:, -1] > W - 1).all() and (my[0] < 0).all() and (my[-1] > H - 1).all()
    frame = lens_scenes.noise(W, H, seed=3)
    out = lens_mirror.sample(frame, mx, my)
    pad = 8
    padded = np.pad(frame, pad, mode="edge")
    np.testing.assert_array_equal(lens_mirror.sample(padded, mx + np.float32(pad), my + np.float32(pad)), out)
    zero = np.pad(frame, pad, mode="constant")
    assert (lens_mirror.sample(zero, mx + np.float32(pad), my + np.float32(pad)) != out).any(), "the zero border must be distinguishable"
    np.testing.assert_array_equal(lens_mirror.undistort(np.full((H, W), 200, np.uint8), k, c), 200)
    np.testing.assert_array_equal(lens_mirror.undistort(np.full((H, W), 255, np.uint8), k, c), 255)


@pytest.mark.parametrize("lens", lens_scenes.LENS_NAMES)
def test_saturation_both_ways_on_the_checkerboard(lens):
    W, H = 67, 35
    k, c = lens_scenes.lenses(W, H)[lens]
    board = lens_scenes.checkerboard(W, H)
    mx, my = lens_mirror.positions(W, H, k, c)
    raw = lens_mirror.sample(board, mx, my, raw=True)
    assert raw.min() < 0 and raw.max() > 255, (raw.min(), raw.max())
    out = lens_mirror.sample(board, mx, my)
    np.testing.assert_array_equal(out, np.clip(raw, 0, 255))
    assert (out[raw < 0] == 0).all() and (out[raw > 255] == 255).all()


def test_centre_is_measured_from_the_bottom():
    """moving the centre up (a larger center-y) moves the sampled positions up (smaller rows)"""
    W, H = 67, 35
    _, my0 = lens_mirror.positions(W, H, (0, 0, 0), (W / 2.0, H / 2.0))
    _, my1 = lens_mirror.positions(W, H, (0, 0, 0), (W / 2.0, H / 2.0 + 3.0))
    np.testing.assert_allclose(my1 - my0, -3.0, atol=1e-4)


def test_fold_over_rule():
    assert not lens_mirror.folds_over(640, 480, (0.0, 0.0, 0.0))
    for name, (k, _) in lens_scenes.lenses(640, 480).items():
        assert not lens_mirror.folds_over(640, 480, k), name
    assert lens_mirror.folds_over(640, 480, (-1.0, 0.0, 0.0))          # 1 - 3 rho^2 < 0 from rho^2 = 1/3, the corner is at 0.39
    assert not lens_mirror.folds_over(640, 480, (-0.85, 0.0, 0.0))     # 1 - 2.55 * 0.390625 > 0


def test_constants_and_binding():
    lib = mvs_amd.load_library()
    names = ("mvs_set_lens", "mvs_lens", "mvs_undistort", "mvs_undistort_device", "mvs_undistort_map", "mvs_frame_upload_lens",
             "mvs_frame_upload_lens_device")
    for name in names:
        assert getattr(lib, name).argtypes is not None
    assert lib.mvs_set_lens(None, None, 0.0, 0.0) == -1                 # MVS_EINVAL for a NULL context, no GPU needed
    assert lib.mvs_lens(None, None, None, None) == -1
    assert lib.mvs_undistort(None, None, None) == -1
    assert lib.mvs_undistort_device(None, None, None, 1) == -1
    assert lib.mvs_undistort_map(None, None) == -1
    assert lib.mvs_frame_upload_lens(None, 0, None) == -1
    assert lib.mvs_frame_upload_lens_device(None, 0, None) == -1
    for name in ("set_lens", "lens", "undistort", "undistort_device", "undistort_map"):
        assert callable(getattr(mvs_amd.Context, name))
    import inspect
    assert inspect.signature(mvs_amd.Context.frame_upload).parameters["lens"].default is False
    assert inspect.signature(mvs_amd.Context.frame_upload_device).parameters["lens"].default is False
    header = open(mvs_amd.PKG_ROOT + "/../include/mvs.h").read()
    assert "#define MVS_LENS_MAX_COEFFICIENT 16" in header


def test_tracks_loader_exposes_the_lens():
    import tracks_yaml
    t = tracks_yaml.load("koberec.yaml")
    assert t["distortion"] == pytest.approx([-0.19075068831443787, 0.18270176649093628, 0.0], abs=0)
    assert (t["center_x"], t["center_y"], t["width"], t["height"]) == (320.0, 240.0, 640, 480)
    assert tracks_yaml.load("koule-tr.yaml")["distortion"] == [0.0, 0.0, 0.0]


def test_lens_frames_render_the_scene_where_the_lens_puts_it():
    """tests/lens_scenes.py against the mirror, which maps the other way: undistorting the lens's render gives the pinhole render up to
    resampling.  The bound of 3 grey levels: the lens's render is rounded to integers (+-0.5), the bicubic weights have an absolute sum
    of at most 1.25 per axis (1.5625 in 2-D), so that rounding moves the sample by up to 0.78; the sample is rounded again (0.5) and the
    1/32-pixel position grid moves it by at most 1/64 px times the texture's slope; the cubic's own interpolation error on a texture
    whose shortest wavelength is 22 px stays below one level.  Together below 3."""
    W, H = 160, 120
    sc = synth.Scene(synth.SEED_SCENE, W / 1920.0)
    pin = sc.render([0.05, -0.1, 0.0], W, H).astype(np.int64)
    for name in ("koberec", "zatisi"):
        k, c = lens_scenes.lenses(W, H)[name]
        dist = lens_scenes.render_through_lens(sc, [0.05, -0.1, 0.0], W, H, k, c)
        und = lens_mirror.undistort(dist, k, c).astype(np.int64)
        assert np.abs(dist.astype(np.int64) - pin).max() > 20, "premise: the lens moves the image"
        assert np.abs(und - pin).max() <= 3, (name, np.abs(und - pin).max())


def test_undistorting_buys_back_the_sweeps_bad_pixels(oracle):
    """160 x 120, 32 planes over ground truth +- 0.002, 4 views at radius 0.3, fixed sampler, winner-take-all (the scene of
    test_aggregation_halves_the_bad_pixels_of_winner_take_all), koberec's lens: bad_share on pinhole renders, on the lens's frames as
    they are, and on the mirror's undistorted frames.  DESIGN.md section 17 carries the figures for all three lenses."""
    from test_aggregate_cpu import bad_share
    W, H, D, V = 160, 120, 32, 4
    k, c = lens_scenes.lenses(W, H)["koberec"]
    main_cam, main_img, side_cams, sides, gt = synth.make_views(W, H, V, radius=0.3)
    _, d_main, _, d_sides, _ = lens_scenes.make_views(W, H, V, k, c, radius=0.3)
    z_lo, z_hi = float(gt.min()) - 0.002, float(gt.max()) + 0.002
    z = oracle.plane_table(D, z_lo, z_hi)

    def bad(m, s):
        _, _, idx = oracle.sweep(main_cam, m, side_cams, s, D, z_lo, z_hi, nthreads=4, sampler="fixed")[:3]
        return bad_share(idx, gt, z)

    b_pin = bad(main_img, sides)
    b_dist = bad(d_main, d_sides)
    b_und = bad(lens_mirror.undistort(d_main, k, c), [lens_mirror.undistort(s, k, c) for s in d_sides])
    print("bad pixels: pinhole %.4f, lens frames as they are %.4f, undistorted %.4f" % (b_pin, b_dist, b_und))
    assert b_dist >= 3 * b_pin, "premise: the lens costs the sweep its pixels"
    assert b_und - b_pin <= 0.25 * (b_dist - b_pin)
