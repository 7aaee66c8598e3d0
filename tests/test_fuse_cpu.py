"""Depth-map fusion without a GPU: the contract's float32 restatement (tests/fuse_mirror.py) against the analytic height field of
synth.Scene, and the new entry points' argument checks through the library."""
import ctypes as C

import numpy as np
import pytest

import fuse_mirror as fm
import mvs_amd
from mvs_amd import synth

W, H = 320, 240
RING = 0.15


def _centres():
    return [(0.0, 0.0, 0.0)] + [(RING * np.cos(a), RING * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(4) / 4]


@pytest.fixture(scope="module")
def views():
    """five axis-parallel cameras: the centre (slot 0) and a ring of radius 0.15; exact NDC depth maps of the height field"""
    sc = synth.Scene()
    cams, depths, mats = {}, {}, {}
    for s, c in enumerate(_centres()):
        cams[s] = synth.camera_at(c, W, H)
        depths[s] = sc.render(c, W, H, want_depth=True)[1]
        mats[s] = fm.slot_matrices(cams[s])
    return cams, depths, mats


def _f32(mats):
    return {s: tuple(np.asarray(m, np.float32) for m in v) for s, v in mats.items()}


def _analytic_normal(x, y):
    dhx = -0.4 * 1.3 * np.cos(1.3 * x + 0.7) * np.cos(1.1 * y - 0.2)
    dhy = 0.4 * 1.1 * np.sin(1.3 * x + 0.7) * np.sin(1.1 * y - 0.2)
    n = np.stack([-dhx, -dhy, np.ones_like(x)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def test_exact_maps_keep_what_two_neighbours_see_on_the_surface(views):
    _, depths, mats = views
    r = fm.fuse(depths, {}, _f32(mats), 0, [1, 2, 3, 4], min_consistent=2)
    r64 = fm.fuse(depths, {}, mats, 0, [1, 2, 3, 4], min_consistent=2, dtype=np.float64)
    # pixels at least two neighbours see: the float64 back-projection lands inside the neighbour's frame on a valid depth
    X = r64["X"].reshape(-1, 3)
    seen = np.zeros(H * W, np.int32)
    for j in (1, 2, 3, 4):
        P = mats[j][0]
        q = X @ P[:3, :3].T + P[:3, 3]
        qw = X @ P[3, :3] + P[3, 3]
        u = (q[:, 0] / qw + 1) * W / 2 - 0.5
        v = (1 - q[:, 1] / qw) * H / 2 - 0.5
        seen += (qw > 0) & (u >= 0.5) & (u < W - 1.5) & (v >= 0.5) & (v < H - 1.5)
    seen = (seen >= 2).reshape(H, W)
    frac = r["keep"][seen].mean()
    assert seen.sum() > 0.8 * H * W
    assert frac >= 0.99, frac
    assert (r["keep"] == r64["keep"]).mean() > 0.999
    pts = r["rows"]
    assert np.all(pts[:, 3] == 1.0)
    xyz = pts[:, :3].astype(np.float64)
    depth = -xyz[:, 2]   # the centre camera looks down -z from the origin
    err = np.abs(xyz[:, 2] - synth.Scene.height(xyz[:, 0], xyz[:, 1]))
    assert np.all(err <= 1e-4 * depth), err.max()
    n_ref = _analytic_normal(xyz[:, 0], xyz[:, 1])
    ang = np.degrees(np.arccos(np.clip((pts[:, 4:7].astype(np.float64) * n_ref).sum(1), -1, 1)))
    assert ang.max() <= 1.0, ang.max()
    assert np.allclose(np.linalg.norm(pts[:, 4:7], axis=1), 1.0, atol=1e-6)


def test_seeded_outliers_in_the_reference_are_rejected(views):
    cams, depths, mats = views
    rng = np.random.Generator(np.random.PCG64(0xF05E))
    d0 = depths[0].copy()
    idx = rng.choice(np.arange(H * W).reshape(H, W)[8:-8, 8:-8].ravel(), 400, replace=False)
    # move each outlier 20 % farther along its ray: NDC z of w' = 1.2 w
    P = cams[0].astype(np.float64)
    A, B = P[2, 2] * -1.0, P[2, 3]   # z_ndc = (A w + B) / w for an axis-parallel camera at the origin (z_cam = -w)
    z = d0.ravel()[idx].astype(np.float64)
    w = B / (z - A)
    d0.ravel()[idx] = ((A * 1.2 * w + B) / (1.2 * w)).astype(np.float32)
    dd = dict(depths)
    dd[0] = d0
    r = fm.fuse(dd, {}, _f32(mats), 0, [1, 2, 3, 4], min_consistent=2)
    assert not r["keep"].ravel()[idx].any()
    assert r["keep"].sum() > 0.8 * H * W


def test_no_neighbours_keeps_every_valid_pixel_with_a_normal(views):
    _, depths, mats = views
    rng = np.random.Generator(np.random.PCG64(7))
    d0 = depths[0].copy()
    holes = rng.random((H, W)) < 0.3
    d0[holes & (rng.random((H, W)) < 0.5)] = 1.0
    d0[holes & ~(d0 == 1.0)] = np.nan
    r = fm.fuse({0: d0}, {}, _f32(mats), 0, [], min_consistent=0)
    valid = ~holes
    pad = np.pad(valid, 1)
    expect = valid & (pad[1:-1, :-2] | pad[1:-1, 2:]) & (pad[:-2, 1:-1] | pad[2:, 1:-1])
    assert np.array_equal(r["keep"], expect)
    assert len(r["rows"]) == expect.sum()
    # K = 0: the point is the pixel's own back-projection
    assert np.array_equal(r["rows"][:, :3], r["X"][expect])


def test_pixel_centres_restate_the_sweep_fmaf():
    """fmaf((float)(2 c + 1), 1/W, -1): float64 product and sum are exact, one rounding to float32"""
    for n in (241, 322, 480, 640, 1080, 1920):
        i = np.arange(n)
        inv = np.float32(1.0) / np.float32(n)
        exact = [float(np.float32((2 * k + 1) * float(inv) - 1.0)) for k in (0, n // 3, n - 1)]
        assert list(fm.pixel_xn(i, n)[[0, n // 3, n - 1]]) == exact
        assert np.all(np.abs(fm.pixel_xn(i, n).astype(np.float64) - ((2 * i + 1) / n - 1.0)) < 2e-7)
        assert np.array_equal(fm.pixel_yn(i, n), -fm.pixel_xn(i, n))


def test_new_entry_points_refuse_a_null_context():
    """every fusion entry point reports MVS_EINVAL for a NULL context -- no GPU needed"""
    lib = mvs_amd.load_library()
    EINVAL = -1
    cam = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    buf = (C.c_float * 36)()
    n = C.c_int(-5)
    assert lib.mvs_depth_store(None, 4) == EINVAL
    assert lib.mvs_depth_upload(None, 0, cam, buf, None) == EINVAL
    assert lib.mvs_depth_upload_device(None, 0, cam, C.cast(buf, C.c_void_p), None) == EINVAL
    assert lib.mvs_fuse_depth(None, 0, 0, None, 0, 1.0, 0.01, float("inf"), None, C.byref(n)) == EINVAL
    assert lib.mvs_depth_slot_matrices(None, 0, buf) == EINVAL
    assert lib.mvs_fuse_points_device(None) is None
    assert b"null context" in lib.mvs_last_error(None) or b"null argument" in lib.mvs_last_error(None)
    assert mvs_amd.MVS_K_FUSE == 6 and mvs_amd.MVS_K_COUNT == 8
