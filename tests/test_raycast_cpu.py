"""The TSDF ray-cast without a GPU: the entry points' argument checks through the library, the contract's numpy restatement
(tests/raycast_mirror.py) against a scalar per-ray loop written from DESIGN.md section 14, analytic fields, exact maps of synth.Scene's
height field, and the premises of every crafted case tests/test_raycast_gpu.py compares on the GPU."""
import ctypes as C

import numpy as np
import pytest

import mvs_amd
import raycast_mirror as rm
import raycast_volumes as rv
import tsdf_mirror as tm
from mvs_amd import synth

f32 = np.float32
fm = tm.fm


def _mats(cam):
    return tuple(m.astype(f32) for m in fm.slot_matrices(cam))


def test_entry_points_refuse_a_null_context():
    lib = mvs_amd.load_library()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    s, c = np.zeros(1, f32), np.zeros(1, np.int32)
    cam = np.eye(4, dtype=f32)
    assert lib.mvs_tsdf_upload(None, fp(s), c.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert lib.mvs_tsdf_raycast(None, fp(cam), 1, 0.5) == -1
    assert lib.mvs_tsdf_raycast_fetch(None, None, None) == -1
    assert not lib.mvs_tsdf_raycast_depth_device(None)
    assert not lib.mvs_tsdf_raycast_normals_device(None)


def test_kernel_kind_count_is_unchanged():
    assert mvs_amd.MVS_K_COUNT == 8 and mvs_amd.MVS_K_TSDF == 7


# ---- the contract, one ray at a time, in np.float32 scalars (not from the mirror) ----
def _axis(g, G):
    fl = np.floor(g)
    if fl >= 0:
        i = int(fl) if fl <= G - 2 else G - 2
    else:
        i = 0
    r = f32(g - f32(i))
    if r > 0:
        fr = r if r < 1 else f32(1.0)
    else:
        fr = f32(0.0)
    return i, f32(fr)


def _cell(X, origin, inv_h, G):
    out = [_axis(f32(f32(X[a] - origin[a]) * inv_h), G) for a in range(3)]
    return [o[0] for o in out], [o[1] for o in out]


def _lerp(a, b, f):
    return f32(a + f32(f * f32(b - a)))


def _eight(F, i):
    return [F[i[2] + (c >> 2), i[1] + ((c >> 1) & 1), i[0] + (c & 1)] for c in range(8)]


def _value(F, mask, X, origin, inv_h, G):
    i, (fx, fy, fz) = _cell(X, origin, inv_h, G)
    v = _eight(F, i)
    c0 = _lerp(_lerp(v[0], v[1], fx), _lerp(v[2], v[3], fx), fy)
    c1 = _lerp(_lerp(v[4], v[5], fx), _lerp(v[6], v[7], fx), fy)
    return bool(mask[i[2], i[1], i[0]]), _lerp(c0, c1, fz)


def _row(P, r, X):
    return f32(f32(f32(f32(P[r, 0] * X[0]) + f32(P[r, 1] * X[1])) + f32(P[r, 2] * X[2])) + P[r, 3])


def _scalar_pixel(F, mask, origin, h, mats, W, H, row, col, step):
    """-> (z, (nx, ny, nz)) or None (empty)"""
    P, Pi, Cc = mats
    G = F.shape[0]
    inv_h = f32(1.0) / h
    delta = f32(f32(step) * h)
    K = int(np.floor(1.75 * (G - 1) / float(f32(step)))) + 2
    xn = f32(float(2 * col + 1) * float(f32(1.0) / f32(W)) - 1.0)
    yn = f32(-float(2 * row + 1) * float(f32(1.0) / f32(H)) + 1.0)
    z0 = f32(0.0)
    hh = [f32(f32(f32(f32(Pi[r, 0] * xn) + f32(Pi[r, 1] * yn)) + f32(Pi[r, 2] * z0)) + Pi[r, 3]) for r in range(4)]
    X1 = [f32(hh[a] / hh[3]) for a in range(3)]
    if not _row(P, 3, X1) > 0:
        return None
    d = [f32(X1[a] - Cc[a]) for a in range(3)]
    ln = np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])))
    if not (ln > 0 and np.isfinite(ln)):
        return None
    d = [f32(x / ln) for x in d]
    t_in, t_out = f32(0.0), f32(np.inf)
    for a in range(3):
        lo, hi = origin[a], f32(origin[a] + f32(h * f32(G - 1)))
        if d[a] != 0:
            t1, t2 = f32(f32(lo - Cc[a]) / d[a]), f32(f32(hi - Cc[a]) / d[a])
            t_in, t_out = max(t_in, min(t1, t2)), min(t_out, max(t1, t2))
        elif not (lo <= Cc[a] <= hi):
            return None
    if not t_in <= t_out:
        return None
    point = lambda t: [f32(Cc[a] + f32(t * d[a])) for a in range(3)]   # noqa: E731
    before = None
    t_star = None
    for k in range(K + 1):
        t = f32(t_in + f32(delta * f32(k)))
        if not t <= t_out:
            break
        now = _value(F, mask, point(t), origin, inv_h, G)
        if before is not None and before[0] and before[1] > 0 and now[0] and now[1] <= 0:
            t_star = f32(before[2] + f32(delta * f32(before[1] / f32(before[1] - now[1]))))
            break
        before = (now[0], now[1], t)
    if t_star is None:
        return None
    Xs = point(t_star)
    i, (fx, fy, fz) = _cell(Xs, origin, inv_h, G)
    if not mask[i[2], i[1], i[0]]:
        return None
    v = _eight(F, i)
    D = lambda p, q: f32(v[p] - v[q])   # noqa: E731
    gx = _lerp(_lerp(D(1, 0), D(3, 2), fy), _lerp(D(5, 4), D(7, 6), fy), fz)
    gy = _lerp(_lerp(D(2, 0), D(3, 1), fx), _lerp(D(6, 4), D(7, 5), fx), fz)
    gz = _lerp(_lerp(D(4, 0), D(5, 1), fx), _lerp(D(6, 2), D(7, 3), fx), fy)
    gl = np.sqrt(f32(f32(f32(gx * gx) + f32(gy * gy)) + f32(gz * gz)))
    if not (gl > 0 and np.isfinite(gl)):
        return None
    z = f32(_row(P, 2, Xs) / _row(P, 3, Xs))
    if not (-1 < z < 1):
        return None
    return z, (f32(gx / gl), f32(gy / gl), f32(gz / gl))


@pytest.mark.parametrize("case", ["shell_oblique", "holes_front", "tiny_graze"])
def test_mirror_equals_a_scalar_loop_bit_for_bit(case):
    name, vname, G, (W, H), cam, step, mo, _, _ = next(c for c in rv.CASES if c[0] == case)
    vol = rv.volume(vname, G)
    mats = _mats(rv.camera(cam, W, H))
    depth, normals = rm.raycast(vol, mats, W, H, mo, step)
    F, mask = vol.field(mo)
    rng = np.random.Generator(np.random.PCG64(7))
    hit_px = np.flatnonzero(depth.ravel() < 1)
    empty_px = np.flatnonzero(depth.ravel() == 1)
    pick = np.concatenate([rng.choice(hit_px, min(len(hit_px), 160), replace=False), rng.choice(empty_px, 60, replace=False)])
    if case == "tiny_graze":
        pick = np.union1d(pick, np.arange(22 * W, 23 * W))   # the grazing row
    assert len(pick) >= 100
    with np.errstate(all="ignore"):
        for p in pick:
            r, c = divmod(int(p), W)
            got = _scalar_pixel(F, mask, vol.origin, vol.h, mats, W, H, r, c, step)
            if got is None:
                assert depth[r, c] == 1 and not normals[r, c].any(), (r, c)
            else:
                assert f32(got[0]).tobytes() == depth[r, c].tobytes(), (r, c, got[0], depth[r, c])
                assert np.array(got[1], f32).tobytes() == normals[r, c].tobytes(), (r, c, got[1], normals[r, c])


# ---- analytic fields ----
@pytest.mark.parametrize("step", [0.25, 0.5, 1.0, 1.7])
def test_a_half_space_is_hit_on_its_plane(step):
    """a linear field: the trilinear interpolant and the crossing's linear interpolation are exact up to rounding"""
    G = 25
    h = rv.spacing(G)
    n = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    x, y, z = rv.nodes(G)
    F = ((x - rv.CENTRE[0]) * n[0] + (y - rv.CENTRE[1]) * n[1] + (z - rv.CENTRE[2]) * n[2]).astype(f32)   # in world units: |F| < 2
    mask = np.zeros((G, G, G), bool)
    mask[:G - 1, :G - 1, :G - 1] = True
    alive, O, d = rm.pixel_rays(_mats(rv.camera("front", 67, 45)), 67, 45)
    m = rm.march(F, mask, rv.ORIGIN, h, O, d, step)
    assert alive.all() and m["ok"].sum() >= 0.5 * len(O)
    off = np.abs((m["X"][m["ok"]].astype(np.float64) - rv.CENTRE) @ n)
    print("half space, step %.2f: %d hits, largest distance to the plane %.3g" % (step, m["ok"].sum(), off.max()))
    assert off.max() <= 1e-5 * 2.0
    cosang = m["normal"][m["ok"]].astype(np.float64) @ n
    assert cosang.min() >= 1 - 1e-5


@pytest.mark.parametrize("G", [25, 50])
def test_a_sphere_is_hit_on_its_surface(G):
    vol = rv.volume("sphere", G)
    F, mask = vol.field(1)
    alive, O, d = rm.pixel_rays(_mats(rv.camera("front", 67, 45)), 67, 45)
    m = rm.march(F, mask, vol.origin, vol.h, O, d, 0.5)
    assert m["ok"].sum() >= 600
    X = m["X"][m["ok"]].astype(np.float64)
    off = np.abs(np.linalg.norm(X - rv.CENTRE, axis=1) - rv.R) / float(vol.h)
    print("sphere, G = %d: %d hits, distance to the sphere: median %.4f h, largest %.4f h" % (G, m["ok"].sum(), np.median(off), off.max()))
    assert off.max() <= 0.05
    out = (X - rv.CENTRE) / np.linalg.norm(X - rv.CENTRE, axis=1, keepdims=True)
    # the interpolant's gradient blends secants over one cell, across which the sphere's own normal turns by h / R
    ang = np.degrees(np.arccos(np.clip((m["normal"][m["ok"]] * out).sum(1), -1, 1)))
    assert ang.max() <= np.degrees(float(vol.h) / rv.R), ang.max()


def test_a_direction_component_of_zero_takes_the_slab_rule():
    vol = rv.volume("sphere", 25)
    F, mask = vol.field(1)
    O = np.array([[0.3, 0.2, 0.0], [1.0, -1.0, 0.0], [1.5, 0.0, 0.0], [0.0, -1.01, 0.0], [0.3, 0.2, -3.0]], f32)
    d = np.array([[0, 0, -1]] * 4 + [[1, 0, 0]], f32)
    m = rm.march(F, mask, vol.origin, vol.h, O, d, 0.5)
    assert m["inside"].tolist() == [True, True, False, False, True]
    assert m["ok"].tolist() == [True, False, False, False, False]     # (the last ray starts inside the solid)
    assert abs(float(m["X"][0, 2]) - (-3.0 + np.sqrt(rv.R ** 2 - 0.13))) <= 0.05 * float(vol.h)
    assert m["X"][0, 0] == f32(0.3) and m["X"][0, 1] == f32(0.2)
    assert m["t_in"][0] == 2.0 and m["t_out"][0] == 4.0 and m["t_in"][4] == 0.0 and m["t_out"][4] == f32(0.7)


def test_the_sample_count_is_bounded_where_t_stops_growing():
    vol = rv.volume("sphere", 16)
    F, mask = vol.field(1)
    m = rm.march(F, mask, vol.origin, vol.h, np.array([[0.0, 0.0, 1e30]], f32), np.array([[0.0, 0.0, -1.0]], f32), 0.5)
    assert m["inside"][0] and m["t_in"][0] == f32(1e30) and m["t_out"][0] == f32(1e30)
    assert m["samples"] == rm.k_max(16, 0.5) + 1 == int(1.75 * 15 / 0.5) + 3
    assert not m["hit"][0]


# ---- exact maps ----
@pytest.fixture(scope="module")
def ring_volume():
    sc = synth.Scene()
    W, H = rv.RING_W, rv.RING_H
    maps, mats, cams, exact = {}, {}, {}, {}
    for s, c in enumerate(rv.ring_centres()):
        cams[s] = synth.camera_at(c, W, H)
        mats[s] = _mats(cams[s])
        exact[s] = sc.render(c, W, H, want_depth=True)[1]
        maps[s] = tm.wmap(exact[s], None, mats[s])
    vol = tm.Volume(rv.RING_G, rv.RING_ORIGIN, rv.RING_H_NODE, 4 * rv.RING_H_NODE).integrate(maps, mats, range(5))
    return vol, cams, mats, exact


@pytest.mark.parametrize("slot", [0, 1])
def test_mirror_raycasts_exact_maps_onto_the_height_field(ring_volume, slot):
    """five ring cameras at 320 x 240, G = 64, truncation 4 h, step 0.5, cast into ring cameras 0 and 1.  Measured with this mirror:
    printed by the test (the bounds are the issue's table)"""
    vol, cams, mats, exact = ring_volume
    depth, normals = rm.raycast(vol, mats[slot], rv.RING_W, rv.RING_H, 1, 0.5)
    f = rv.exact_map_figures(depth, normals, cams[slot], rv.ring_centres()[slot], exact[slot])
    print("exact maps, mirror, camera %d: %s" % (slot, f))
    rv.assert_exact_map_figures(f)


# ---- the premises of the GPU cases ----
@pytest.mark.parametrize("case", rv.CASES, ids=[c[0] for c in rv.CASES])
def test_case_premises(case):
    name, vname, G, (W, H), cam, step, mo, least_hits, least_empty = case
    vol = rv.volume(vname, G)
    mats = _mats(rv.camera(cam, W, H))
    depth, normals, info = rm.raycast(vol, mats, W, H, mo, step, want_info=True)
    hits, empty = int((depth < 1).sum()), int((depth == 1).sum())
    print("%s: %d hit, %d empty of %d" % (name, hits, empty, W * H))
    assert hits + empty == W * H and hits >= least_hits and empty >= least_empty
    assert ((depth == 1) == ~normals.any(-1)).all()
    assert np.abs(np.linalg.norm(normals[depth < 1].astype(np.float64), axis=1) - 1).max(initial=0) <= 1e-6
    if cam == "in_box_default_near":
        assert info["ok"].sum() >= 2500 and not info["final"].any()      # hits, every one in front of the near plane
    who = np.flatnonzero(info["final"])
    F, mask = vol.field(mo)
    if vname == "last":
        idx, _ = rm._locate([info["X"][who, a] for a in range(3)], vol.origin, f32(1.0) / vol.h, G)
        assert (np.stack(idx).max(0) == G - 2).mean() >= 0.9
        assert all((idx[a] == G - 2).sum() >= 100 for a in ((0, 2) if cam == "oblique" else (2,) if cam == "front" else (1,)))
    if vname == "tiny":
        # the hits of the grazing row: the hit's current sample lies in a cell -- in a whole brick -- without a corner <= 0
        hitk = np.flatnonzero(info["hit"])
        alive, O, d = rm.pixel_rays(mats, W, H)
        px = info["pixels"][hitk]
        tk = (info["t_in"][hitk] + (f32(step) * vol.h) * info["k"][hitk].astype(f32)).astype(f32)
        idx, fr = rm._locate(rm._point(O[px], d[px], tk), vol.origin, f32(1.0) / vol.h, G)
        corner = np.stack(rm._corners(F, idx))
        graze = (corner > 0).all(0)
        assert graze.sum() >= 40 and (px[graze] // W == 22).all() and info["final"][hitk][graze].all()
        assert (fr[1][graze] == 1).all() and (corner[:, graze].min(0) == rv.TINY).all()
        assert (F[:9, 8:, :] > 0).all() and (idx[1][graze] >= 8).all() and (idx[2][graze] <= 7).all()   # bricks (*, 1, 0): cells j 8..15, k 0..7
