"""The TSDF volume's appearance without a GPU: the argument checks that need no device, the numpy mirror
(tests/appearance_mirror.py) against a scalar loop written from the rules, the properties rule B promises, the premises of the crafted cases
of tests/appearance_cases.py, and the accuracy of shaded ray-casts of exact maps against the frames (the acceptance case)."""
import ctypes as C
import math

import numpy as np
import pytest

import appearance_cases as ac
import appearance_mirror as am
import mvs_amd
import raycast_mirror as rm
import tsdf_mirror as tm
from mvs_amd import synth

f32 = np.float32
u32 = np.uint32
fm = tm.fm


def _mats(cam):
    P, Pi, Cc = fm.slot_matrices(cam)
    return P.astype(f32), Pi.astype(f32), Cc.astype(f32)


def test_entry_points_refuse_null_arguments():
    lib = mvs_amd.load_library()
    one_i = np.zeros(1, np.int32)
    ip = one_i.ctypes.data_as(C.POINTER(C.c_int32))
    cells = np.zeros(1, u32).ctypes.data_as(C.POINTER(C.c_uint32))
    pts = np.ones(4, f32).ctypes.data_as(C.POINTER(C.c_float))
    cam = synth.camera_at((0.0, 0.0, 0.0), 64, 48).ctypes.data_as(C.POINTER(C.c_float))
    assert lib.mvs_tsdf_integrate_frames(None, 1, ip, ip, float("inf")) == -1
    assert lib.mvs_tsdf_appearance_fetch(None, cells) == -1 and lib.mvs_tsdf_appearance_upload(None, cells) == -1
    assert lib.mvs_tsdf_shade(None, cam, C.c_void_p(16)) == -1
    assert lib.mvs_tsdf_shade_fetch(None, np.zeros(2, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))) == -1
    assert lib.mvs_tsdf_sample_appearance(None, pts, 1, pts) == -1
    assert not lib.mvs_tsdf_shade_device(None) and not lib.mvs_depth_slot_device(None, 0)


# ---- the mirror against a scalar loop ---------------------------------------------------------------------------------------------------
SW, SH, SG = 24, 18, 16


@pytest.fixture(scope="module")
def small():
    """three ring cameras at 24 x 18 with exact maps (one with holes) and their frames, G = 16 over tests/test_tsdf_gpu.py's cube"""
    sc = synth.Scene(freq_scale=SW / 1920.0)
    rng = np.random.Generator(np.random.PCG64(0x5CA1))
    mats, maps, frames = {}, {}, {}
    for s, c in enumerate(ac.ring_centres()[:3]):
        img, d = sc.render(c, SW, SH, want_depth=True)
        if s == 1:
            d = d.copy()
            d[rng.random(d.shape) < 0.2] = np.nan
        mats[s] = _mats(synth.camera_at(c, SW, SH))
        maps[s] = tm.wmap(d, None, mats[s])
        frames[s + 4] = img
    frames[3] = (255 - frames[4]).astype(np.uint8)
    pairs = [(0, 4), (1, 5), (2, 6), (0, 3), (1, 5)]
    origin, h = ac.cube(SG)
    return mats, maps, frames, pairs, origin, h


def _scalar_integrate(G, origin, h, inv_tau, maps, mats, frames, pairs):
    """section 12 rules 2-4 and section 15 rule B, one node and one pair at a time"""
    total = np.zeros((G, G, G), f32)
    count = np.zeros((G, G, G), np.int32)
    asum = np.zeros((G, G, G), np.int64)
    acount = np.zeros((G, G, G), np.int64)
    one, half = f32(1.0), f32(0.5)
    for k in range(G):
        for j in range(G):
            for i in range(G):
                x, y, z = origin[0] + h * f32(i), origin[1] + h * f32(j), origin[2] + h * f32(k)
                for s, fs in pairs:
                    P = mats[s][0]
                    H, W = maps[s].shape
                    qx, qy, qw = (P[r, 0] * x + ((P[r, 1] * y + P[r, 2] * z) + P[r, 3]) for r in (0, 1, 3))
                    if not qw > 0:
                        continue
                    inv = one / qw
                    u = (qx * inv + one) * (f32(W) * half) - half
                    v = (one - qy * inv) * (f32(H) * half) - half
                    c, r = math.floor(u + half), math.floor(v + half)
                    if not (0 <= c < W and 0 <= r < H):
                        continue
                    wd = maps[s][r, c]
                    if wd != wd:
                        continue
                    t = (wd - qw) * inv_tau
                    if t >= -1:
                        total[k, j, i] = total[k, j, i] + (t if t < 1 else one)
                        count[k, j, i] += 1
                        if t < 1 and acount[k, j, i] < 255:
                            asum[k, j, i] += int(frames[fs][r, c])
                            acount[k, j, i] += 1
    return total, count, ac.pack(acount, asum)


def _scalar_appearance(vol, X):
    """rule C at one point -> value or None"""
    G = vol.G
    inv_h = f32(1.0) / vol.h
    g = [(f32(X[a]) - vol.origin[a]) * inv_h for a in range(3)]
    if not all(0 <= ga <= f32(G - 1) for ga in g):
        return None
    idx, fr = [], []
    for ga in g:
        i = min(max(int(math.floor(ga)), 0), G - 2)
        idx.append(i)
        fr.append(min(max(ga - f32(i), f32(0.0)), f32(1.0)))
    num, den = f32(0.0), f32(0.0)
    for d in range(8):
        di, dj, dk = d & 1, (d >> 1) & 1, d >> 2
        w = f32(f32((fr[0] if di else f32(1.0) - fr[0]) * (fr[1] if dj else f32(1.0) - fr[1])) * (fr[2] if dk else f32(1.0) - fr[2]))
        cell = int(vol.cells[idx[2] + dk, idx[1] + dj, idx[0] + di])
        n, s = cell >> 24, cell & 0xFFFFFF
        if n > 0:
            num = f32(num + f32(w * f32(f32(s) / f32(n))))
            den = f32(den + w)
    return f32(num / den) if den > 0 else None


def test_mirror_equals_a_scalar_loop(small):
    mats, maps, frames, pairs, origin, h = small
    vol = am.Volume(SG, origin, h, 4 * h).integrate_frames(maps, mats, frames, pairs)
    with np.errstate(all="ignore"):
        total, count, cells = _scalar_integrate(SG, origin, h, vol.inv_tau, maps, mats, frames, pairs)
    n, s = am.split(vol.cells)
    assert (n > 0).sum() > 100 and n.max() >= 3 and (vol.count > n).any()   # votes fell, and fewer than updates: the band is narrower
    assert np.array_equal(vol.count, count) and vol.sum.tobytes() == total.tobytes()
    assert np.array_equal(vol.cells, cells)
    # rules C-E: shading the first camera's exact map, and sampling points in and around the box
    sc = synth.Scene(freq_scale=SW / 1920.0)
    depth = sc.render(ac.ring_centres()[0], SW, SH, want_depth=True)[1].copy()
    depth[2, 3], depth[5, 7] = np.nan, 1.0
    got = am.shade(vol, mats[0], depth)
    P, Pi = mats[0][:2]
    shaded = 0
    with np.errstate(all="ignore"):
        for r in range(SH):
            for c in range(SW):
                zz = depth[r, c]
                exp = (0, 0)
                if -1 < zz < 1:
                    X = fm._unproject(Pi, fm.pixel_xn(c, SW), fm.pixel_yn(r, SH), zz)
                    val = _scalar_appearance(vol, X) if fm._prow(P, 3, X) > 0 else None
                    if val is not None:
                        exp = (min(int(math.floor(val + f32(0.5))), 255), 255)
                        shaded += 1
                assert tuple(got[r, c]) == exp, (r, c, got[r, c], exp)
    assert shaded > 0.8 * SW * SH and tuple(got[2, 3]) == (0, 0) and tuple(got[5, 7]) == (0, 0)
    rng = np.random.Generator(np.random.PCG64(0x9A3E))
    pts = np.concatenate([origin + (rng.random((400, 3)) * 1.2 - 0.1) * float(h) * (SG - 1), rng.choice([1.0, 2.0, 0.5, 0.0], (400, 1))], 1).astype(f32)
    pts[:, :3] *= pts[:, 3:]
    vals = am.sample(vol, pts)
    with np.errstate(all="ignore"):
        for row, val in zip(pts, vals):
            exp = _scalar_appearance(vol, [row[a] / row[3] for a in range(3)])
            assert (val != val) if exp is None else (f32(val).tobytes() == f32(exp).tobytes()), (row, val, exp)
    assert 20 < np.isfinite(vals).sum() < 380


def test_tsdf_fields_equal_the_plain_integration(small):
    mats, maps, frames, pairs, origin, h = small
    a = am.Volume(SG, origin, h, 4 * h).integrate_frames(maps, mats, frames, pairs)
    b = tm.Volume(SG, origin, h, 4 * h).integrate(maps, mats, [s for s, _ in pairs])
    assert a.sum.tobytes() == b.sum.tobytes() and np.array_equal(a.count, b.count) and b.count.max() >= 4


def test_split_lists_repeats_and_saturation(small):
    mats, maps, frames, pairs, origin, h = small
    new = lambda: am.Volume(SG, origin, h, 4 * h)   # noqa: E731
    one = new().integrate_frames(maps, mats, frames, pairs)
    parts = new()
    for p in pairs:
        parts.integrate_frames(maps, mats, frames, [p])
    assert np.array_equal(one.cells, parts.cells) and one.sum.tobytes() == parts.sum.tobytes()
    # a pair listed twice votes twice; the same depth slot with another frame votes that frame
    once = new().integrate_frames(maps, mats, frames, [(0, 4)])
    twice = new().integrate_frames(maps, mats, frames, [(0, 4), (0, 4)])
    other = new().integrate_frames(maps, mats, frames, [(0, 4), (0, 3)])
    n1, s1 = am.split(once.cells)
    n2, s2 = am.split(twice.cells)
    n3, s3 = am.split(other.cells)
    assert n1.max() == 1 and np.array_equal(n2, 2 * n1) and np.array_equal(s2, 2 * s1)
    assert np.array_equal(n3, n2) and np.array_equal(s3, 255 * n1) and (s1 != 255 * n1 - s1).any()
    # saturation: 260 votes leave count 255 and 255 intensities, the TSDF count goes on to 260
    full = new().integrate_frames(maps, mats, frames, [(0, 4)] * 260)
    nf, sf = am.split(full.cells)
    band = n1 == 1
    assert band.sum() > 50 and np.array_equal(nf, 255 * n1) and np.array_equal(sf, 255 * s1)
    assert np.array_equal(full.count[band], np.full(band.sum(), 260))


# ---- rule C on crafted cells: the premises of the cases the GPU test compares bit for bit ----------------------------------------------
POINT_SETS = ac.point_sets()
DEPTH_MAPS = ac.depth_maps()


@pytest.mark.parametrize("name", sorted(POINT_SETS))
def test_crafted_points(name):
    cells, pts, expect = POINT_SETS[name]
    vals = am.sample(ac.crafted_volume(cells), pts)
    have = vals == vals
    if expect == "all":
        assert have.all(), np.nonzero(~have)[0]
    elif expect == "none":
        assert not have.any(), np.nonzero(have)[0]
    else:
        assert have.any() and (~have).any()
    if name == "single_corner":    # the one present corner's own value, whatever its weight: renormalised, not blended with zeros
        assert np.abs(vals - 301.0 / 3.0).max() < 1e-4
    if name == "rounding":
        assert np.abs(vals - 254.5).max() < 1e-4
    if name == "upper_faces":      # a point on a node is that node's value
        n, s = am.split(cells)
        assert vals[3] == f32(s[16, 16, 16]) / f32(n[16, 16, 16]) and vals[4] == f32(s[0, 0, 0]) / f32(n[0, 0, 0])


@pytest.mark.parametrize("name", sorted(DEPTH_MAPS))
def test_crafted_depth_maps(name):
    cells, cam, depth, least_shaded, least_empty = DEPTH_MAPS[name]
    out = am.shade(ac.crafted_volume(cells), _mats(cam), depth)
    have = out[..., 1] == 255
    assert set(np.unique(out[..., 1])) <= {0, 255} and not out[..., 0][~have].any()
    assert have.sum() >= least_shaded and (~have).sum() >= least_empty, (int(have.sum()), int((~have).sum()))
    grey = out[..., 0][have]
    if name == "value_254_5":      # 254.5 up to an ulp either way: both roundings are legitimate, truncation's 254 alone is not
        assert set(np.unique(grey)) <= {254, 255} and (grey == 255).any()
    if name in ("value_255", "clamp_above_255"):
        assert (grey == 255).all()
    if name == "single_flat":
        assert (grey == 100).all()   # 301 / 3 = 100.33
    if name == "random_holes":
        assert not have[~((depth > -1) & (depth < 1))].any()


# ---- accuracy (the acceptance case) ------------------------------------------------------------------------------------------------------
def test_shaded_raycasts_of_exact_maps_match_the_frames():
    """five exact ring maps at 160 x 120 with frames whose texture wavelengths are fixed in pixels, G = 64, truncation 4 h; the ray-casts of
    ring cameras 0 and 1 at step 0.5, shaded, against those cameras' frames.  Required: shaded / hit >= 0.999; |shaded - frame| over the
    shaded pixels: median <= 2, 99th percentile <= 8, maximum <= 16 (the frames' standard deviation is 28)"""
    cams, depths, frames = ac.accuracy_inputs()
    G = ac.ACC_G
    origin, h = ac.cube(G)
    mats = {s: _mats(cams[s]) for s in range(5)}
    maps = {s: tm.wmap(depths[s], None, mats[s]) for s in range(5)}
    vol = am.Volume(G, origin, h, 4 * h).integrate_frames(maps, mats, dict(enumerate(frames)), [(s, s) for s in range(5)])
    for s in (0, 1):
        ray_depth, _ = rm.raycast(vol, mats[s], ac.ACC_W, ac.ACC_H, 1, 0.5)
        f = ac.accuracy_figures(ray_depth, am.shade(vol, mats[s], ray_depth), frames[s])
        print("shaded ray-cast, mirror, camera %d: %s (frame: standard deviation %.1f)" % (s, f, frames[s].std()))
        ac.assert_accuracy_figures(f)
