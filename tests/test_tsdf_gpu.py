"""TSDF fusion on the GPU (csrc/tsdf.hip): mvs_tsdf_fetch against tests/tsdf_mirror.py bit for bit, mvs_tsdf_surface against the surface-nets
oracle, exact maps end to end, the swept sequence of tests/test_fuse_gpu.py, and the error cases."""
import ctypes as C

import numpy as np
import pytest

import mvs_amd
import tsdf_mirror as tm
from mvs_amd import synth

pytestmark = pytest.mark.gpu
mo = tm.mo
RING = 0.15
EINVAL, ESTATE = -1, -3
inf = float("inf")


def _ring(n, radius):
    return [(radius * np.cos(a), radius * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(n) / n]


def _cube(G, side=3.4, low=(-1.7, -1.7, -4.7)):
    return np.asarray(low, np.float32), np.float32(side / (G - 1))


def _mats(ctx, slot):
    P, Pi, Cc = ctx.depth_slot_matrices(slot)
    return P, Pi, Cc


@pytest.fixture(scope="module")
def store160():
    """160 x 120: slots 0-4 the ring's exact maps, 5 a camera facing away, 6 an empty map, 7 ring camera 1 with NaN and 1.0 holes, 8 ring
    camera 2 with its exact map; every slot with a cost map (uniform in [0, 1))"""
    W, H = 160, 120
    sc = synth.Scene()
    rng = np.random.Generator(np.random.PCG64(0x75DF))
    centres = [(0.0, 0.0, 0.0)] + _ring(4, RING)
    cams, depths = [], []
    for c in centres:
        cams.append(synth.camera_at(c, W, H))
        depths.append(sc.render(c, W, H, want_depth=True)[1])
    cams.append(synth.camera_at((0.0, 0.0, 0.0), W, H, rot=np.diag([-1.0, 1.0, -1.0])))
    depths.append(depths[0].copy())
    cams.append(cams[0])
    depths.append(np.ones((H, W), np.float32))
    holes = depths[1].copy()
    pick = rng.random((H, W))
    holes[pick < 0.1] = np.nan
    holes[(pick >= 0.1) & (pick < 0.2)] = 1.0
    cams.append(cams[1])
    depths.append(holes)
    cams.append(cams[2])
    depths.append(depths[2].copy())
    costs = [rng.random((H, W)).astype(np.float32) for _ in depths]
    return W, H, cams, depths, costs


LIST_A = [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 7, 2, 3, 1, 0, 8]   # 19 entries: two launch chunks
LIST_B = [8, 0, 4]                                                 # under a finite max_cost
MAX_COST = 0.5


def _mirror(ctx, W, H, depths, costs, G):
    origin, h = _cube(G)
    mats = {s: _mats(ctx, s) for s in range(len(depths))}
    vol = tm.Volume(G, origin, h, 4 * h)
    maps = {s: tm.wmap(depths[s], costs[s], mats[s]) for s in mats}
    vol.integrate(maps, mats, LIST_A)
    maps_c = {s: tm.wmap(depths[s], costs[s], mats[s], MAX_COST) for s in set(LIST_B)}
    vol.integrate(maps_c, mats, LIST_B)
    return vol


@pytest.mark.parametrize("G", [50, 128])
def test_fields_match_the_mirror_bit_for_bit(store160, G):
    W, H, cams, depths, costs = store160
    origin, h = _cube(G)
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(len(depths))
        for s in range(len(depths)):
            ctx.depth_upload(s, cams[s], depths[s], costs[s])
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate(LIST_A)
        ctx.tsdf_integrate(LIST_B, max_cost=MAX_COST)
        s1, c1 = ctx.tsdf_fetch()
        ref = _mirror(ctx, W, H, depths, costs, G)
        assert c1.max() >= 10 and (c1 > 0).mean() > 0.05
        assert np.array_equal(c1, ref.count), int((c1 != ref.count).sum())
        assert s1.tobytes() == ref.sum.tobytes(), int((s1.view(np.int32) != ref.sum.view(np.int32)).sum())
        # one call per slot, and a second run of the same calls: the same bytes
        ctx.tsdf_volume(G, origin, h, 4 * h)
        for s in LIST_A:
            ctx.tsdf_integrate([s])
        for s in LIST_B:
            ctx.tsdf_integrate([s], max_cost=MAX_COST)
        s2, c2 = ctx.tsdf_fetch()
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate(LIST_A)
        ctx.tsdf_integrate(LIST_B, max_cost=MAX_COST)
        s3, c3 = ctx.tsdf_fetch()
        assert s2.tobytes() == s1.tobytes() and np.array_equal(c2, c1)
        assert s3.tobytes() == s1.tobytes() and np.array_equal(c3, c1)


@pytest.mark.parametrize("min_obs", [1, 3])
def test_surface_matches_surface_nets(store160, min_obs):
    W, H, cams, depths, costs = store160
    G = 128
    origin, h = _cube(G)
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(len(depths))
        for s in range(len(depths)):
            ctx.depth_upload(s, cams[s], depths[s], costs[s])
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate(LIST_A)
        s1, c1 = ctx.tsdf_fetch()
        v, f = ctx.tsdf_surface(min_obs)
    vol = tm.Volume(G, origin, h, 4 * h)
    vol.sum, vol.count = s1, c1
    rv, rf = vol.surface(min_obs)
    assert len(f) > 1000
    assert np.array_equal(f, rf) and len(v) == len(rv)
    assert np.abs(v - rv).max() <= 2e-6 * float(np.abs(origin).max() + G * h)


def _face_normals(v, f):
    p = v[:, :3].astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    n = np.cross(b - a, c - a)
    return (a + b + c) / 3.0, n / np.linalg.norm(n, axis=1, keepdims=True)


def test_exact_maps_end_to_end():
    """the CPU mirror test's setup on the GPU: five exact maps at 320 x 240, G = 64, truncation 4 h; then the facet criteria accept the mesh"""
    W, H, G = 320, 240, 64
    sc = synth.Scene()
    origin, h = _cube(G)
    lib = mvs_amd.load_library()
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(5)
        for s, c in enumerate([(0.0, 0.0, 0.0)] + _ring(4, RING)):
            ctx.depth_upload(s, synth.camera_at(c, W, H), sc.render(c, W, H, want_depth=True)[1])
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate(range(5))
        v, f = ctx.tsdf_surface(1)
        surf = C.c_void_p()
        assert lib.mvs_tsdf_surface(ctx.h, 1, C.byref(surf)) == 0
    try:
        spacing, node = C.c_float(), C.c_float()
        assert lib.mvs_surface_spacing(surf, C.byref(spacing), C.byref(node), None) == 0
        assert spacing.value == h and node.value == h
        nv, nf = C.c_int(), C.c_int()
        lib.mvs_surface_counts(surf, C.byref(nv), C.byref(nf))
        assert (nv.value, nf.value) == (len(v), len(f))
        rep = mvs_amd.CriteriaReport()
        crit = mvs_amd.REFERENCE_FACET_CRITERIA
        assert lib.mvs_surface_enforce_criteria(surf, crit[0], crit[1] * h, crit[2] * h, C.byref(rep)) == 0
        lib.mvs_surface_counts(surf, C.byref(nv), C.byref(nf))
        assert nf.value > 0.5 * len(f)
    finally:
        lib.mvs_surface_free(surf)
    d = np.abs(v[:, 2].astype(np.float64) - synth.Scene.height(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64))) / float(h)
    print("exact maps, GPU: %d vertices, %d faces; median %.4f h, 99th percentile %.4f h; criteria: min angle %.2f deg"
          % (len(v), len(f), np.median(d), np.percentile(d, 99), rep.min_angle_deg))
    assert np.median(d) <= 0.1 and np.percentile(d, 99) <= 0.5
    ctr, n = _face_normals(v, f)
    assert ((n * -ctr).sum(1) > 0).mean() >= 0.99


def _normal_error_deg(p, n):
    dhx = -0.52 * np.cos(1.3 * p[:, 0] + 0.7) * np.cos(1.1 * p[:, 1] - 0.2)
    dhy = 0.44 * np.sin(1.3 * p[:, 0] + 0.7) * np.sin(1.1 * p[:, 1] - 0.2)
    nr = np.stack([-dhx, -dhy, np.ones_like(dhx)], 1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return np.degrees(np.arccos(np.clip((n * nr).sum(1), -1, 1)))


def test_swept_sequence_tsdf_normals_beat_fused_points():
    """tests/test_fuse_gpu.py's swept sequence (640 x 480, five ring cameras, 128 planes, stored device to device), all five slots into a
    256^3 cube over the centre view's frustum between w = 2.45 and 3.55, truncation 4 h: the mesh's median face-normal error must be under
    half the fused points' (measured here on the same store), and its median distance to the height field within one plane step"""
    W, H, D, G = 640, 480, 128, 256
    sc = synth.Scene(freq_scale=W / 1920.0)
    centres = [(0.0, 0.0, 0.0)] + _ring(4, RING)
    cams = [synth.camera_at(c, W, H) for c in centres]
    frames = [sc.render(c, W, H) for c in centres]
    P = cams[0].astype(np.float64)
    A, B = -P[2, 2], P[2, 3]
    ndc = lambda w: (A * w + B) / w   # noqa: E731
    z_lo, z_hi = ndc(2.45), ndc(3.55)
    step_w = (z_hi - z_lo) / D * 3.0 ** 2 / abs(B)   # one plane step in linear depth at w = 3
    half_x = 3.55 / P[0, 0]                          # the centre frustum's half width at w = 3.55 (x / w = 1 / P[0][0])
    side = 2.0 * half_x * 1.01
    origin = np.array([-side / 2, -side / 2, -3.55 - 0.05], np.float32)
    h = np.float32(side / (G - 1))
    with mvs_amd.Context(W, H) as ctx:
        ctx.frame_store(5)
        ctx.depth_store(5)
        for s in range(5):
            ctx.frame_upload(s, frames[s])
        for s in range(5):
            others = [o for o in range(5) if o != s]
            ctx.sweep_handles(s, cams[s], others, np.stack([cams[o] for o in others]), D, z_lo, z_hi)
            dptr, cptr, _ = ctx.sweep_result_pointers()
            ctx.depth_upload_device(s, cams[s], dptr, cptr)
        fused = ctx.fuse_depth(0, [1, 2, 3, 4], min_consistent=2)
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate(range(5))
        v, f = ctx.tsdf_surface(1)
    fp = fused.astype(np.float64)
    fused_err = float(np.median(_normal_error_deg(fp[:, :3], fp[:, 4:7])))
    ctr, n = _face_normals(v, f)
    mesh_err = float(np.median(_normal_error_deg(ctr, n)))
    vd = np.abs(v[:, 2].astype(np.float64) - synth.Scene.height(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)))
    print("swept sequence: h %.5f (%.2f plane steps of %.5f); TSDF mesh %d vertices, %d faces, median face-normal error %.2f deg, median "
          "distance %.5f (%.3f steps); fused points %d, median normal error %.2f deg"
          % (h, h / step_w, step_w, len(v), len(f), mesh_err, np.median(vd), np.median(vd) / step_w, len(fused), fused_err))
    assert len(f) > 10000
    assert np.median(vd) <= step_w
    assert mesh_err < 0.5 * fused_err


def test_errors_and_clearing():
    lib = mvs_amd.load_library()
    W, H = 64, 48
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    cam = synth.camera_at((0.0, 0.0, 0.0), W, H)
    d = np.full((H, W), 0.5, np.float32)
    o = np.array([-1.0, -1.0, -4.0], np.float32)
    with mvs_amd.Context(W, H) as ctx:
        h = ctx.h
        sl = lambda *s: np.asarray(s if s else [0], np.int32)   # noqa: E731
        surf = C.c_void_p()
        s0 = sl(0)
        # before mvs_tsdf_volume
        assert lib.mvs_tsdf_integrate(h, 1, ip(s0), inf) == ESTATE
        assert lib.mvs_tsdf_fetch(h, None, None) == ESTATE
        assert lib.mvs_tsdf_surface(h, 1, C.byref(surf)) == ESTATE
        # mvs_tsdf_volume's arguments
        assert lib.mvs_tsdf_volume(h, 15, fp(o), 0.1, 0.4) == EINVAL and lib.mvs_tsdf_volume(h, 513, fp(o), 0.1, 0.4) == EINVAL
        assert lib.mvs_tsdf_volume(h, 32, None, 0.1, 0.4) == EINVAL
        assert lib.mvs_tsdf_volume(h, 32, fp(np.array([0.0, np.nan, 0.0], np.float32)), 0.1, 0.4) == EINVAL
        assert lib.mvs_tsdf_volume(h, 32, fp(np.array([0.0, np.inf, 0.0], np.float32)), 0.1, 0.4) == EINVAL
        for bad in (0.0, -0.1, inf, float("nan")):
            assert lib.mvs_tsdf_volume(h, 32, fp(o), bad, 0.4) == EINVAL
            assert lib.mvs_tsdf_volume(h, 32, fp(o), 0.1, bad) == EINVAL
        assert lib.mvs_tsdf_fetch(h, None, None) == ESTATE       # (still no volume)
        ctx.tsdf_volume(32, o, 0.1, 0.4)
        assert lib.mvs_tsdf_integrate(h, 1, ip(s0), inf) == EINVAL   # no depth store: slot 0 is outside it
        assert lib.mvs_depth_store(h, 4) == 0
        assert lib.mvs_tsdf_integrate(h, 1, ip(s0), inf) == ESTATE   # unfilled slot
        assert lib.mvs_depth_upload(h, 0, fp(cam), fp(d), fp(d)) == 0
        assert lib.mvs_depth_upload(h, 1, fp(cam), fp(d), None) == 0
        assert lib.mvs_tsdf_integrate(h, 1, None, inf) == EINVAL
        assert lib.mvs_tsdf_integrate(h, 0, ip(s0), inf) == EINVAL
        assert lib.mvs_tsdf_integrate(h, 1, ip(sl(4)), inf) == EINVAL and lib.mvs_tsdf_integrate(h, 1, ip(sl(-1)), inf) == EINVAL
        assert lib.mvs_tsdf_integrate(h, 1, ip(s0), -1.0) == EINVAL and lib.mvs_tsdf_integrate(h, 1, ip(s0), float("nan")) == EINVAL
        assert lib.mvs_tsdf_integrate(h, 2, ip(sl(0, 2)), inf) == ESTATE
        assert lib.mvs_tsdf_integrate(h, 2, ip(sl(0, 1)), 0.5) == ESTATE   # slot 1 has no cost map
        assert lib.mvs_tsdf_integrate(h, 2, ip(sl(0, 1)), inf) == 0
        assert lib.mvs_tsdf_integrate(h, 1, ip(s0), 0.75) == 0
        assert lib.mvs_tsdf_surface(h, 0, C.byref(surf)) == EINVAL
        assert lib.mvs_tsdf_surface(h, 1, None) == EINVAL
        s, c = ctx.tsdf_fetch()
        assert c.max() == 3 and (c > 0).any()
        # re-sizing the depth store leaves the volume alone; mvs_tsdf_volume clears it
        assert lib.mvs_depth_store(h, 2) == 0
        s2, c2 = ctx.tsdf_fetch()
        assert s2.tobytes() == s.tobytes() and np.array_equal(c2, c)
        ctx.tsdf_volume(32, o, 0.1, 0.4)
        s3, c3 = ctx.tsdf_fetch()
        assert not s3.any() and not c3.any()
        # an empty volume meshes to nothing
        assert lib.mvs_tsdf_surface(h, 1, C.byref(surf)) == 0
        try:
            nv, nf = C.c_int(-1), C.c_int(-1)
            assert lib.mvs_surface_counts(surf, C.byref(nv), C.byref(nf)) == 0 and (nv.value, nf.value) == (0, 0)
        finally:
            lib.mvs_surface_free(surf)
