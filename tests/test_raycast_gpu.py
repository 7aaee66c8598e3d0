"""The TSDF ray-cast on the GPU (csrc/raycast.hip): depth bytes, normal bytes and the empty mask against tests/raycast_mirror.py with the
matrices of mvs_depth_slot_matrices -- crafted volumes through mvs_tsdf_upload (tests/raycast_volumes.py), an integrated volume, exact maps
end to end, the map as an input of the depth store, state and order, the error cases.  Every crafted case also runs the plain march (the
library's test hook): the march with the brick mask must give the same bytes."""
import ctypes as C

import numpy as np
import pytest

import mvs_amd
import raycast_mirror as rm
import raycast_volumes as rv
import tsdf_mirror as tm
from mvs_amd import synth

pytestmark = pytest.mark.gpu
fm = tm.fm
f32 = np.float32
EINVAL, ESTATE = -1, -3
inf = float("inf")

_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def _context(W, H):
    """one context per map size, with a one-slot depth store for the camera's matrices"""
    if (W, H) not in _ctx:
        c = mvs_amd.Context(W, H)
        c.depth_store(1)
        _ctx[(W, H)] = c
    return _ctx[(W, H)]


def _mats(ctx, cam):
    """the kernel's matrices of `cam`: a dummy map stored with it, read back with mvs_depth_slot_matrices"""
    ctx.depth_upload(0, cam, np.ones((ctx.H, ctx.W), f32))
    return ctx.depth_slot_matrices(0)


def _same(got, exp, what):
    d, n = got
    ed, en = exp
    assert np.array_equal(d == 1, ed == 1), "%s: empty masks differ at %d pixels" % (what, int(((d == 1) != (ed == 1)).sum()))
    bad = d.view(np.uint32) != ed.view(np.uint32)
    assert not bad.any(), "%s: %d depths differ; first %s: %r vs %r" % (what, int(bad.sum()), np.argwhere(bad)[0], d[bad][0], ed[bad][0])
    badn = (n.view(np.uint32) != en.view(np.uint32)).any(-1)
    assert not badn.any(), "%s: %d normals differ; first %s: %r vs %r" % (what, int(badn.sum()), np.argwhere(badn)[0], n[badn][0], en[badn][0])


def _plain(ctx, on):
    assert ctx.lib.mvs_test_raycast_plain(ctx.h, int(on)) == 0


@pytest.mark.parametrize("case", rv.CASES, ids=[c[0] for c in rv.CASES])
def test_crafted_volume_matches_the_mirror_bit_for_bit(case):
    name, vname, G, (W, H), camname, step, mo, least_hits, least_empty = case
    ctx = _context(W, H)
    vol = rv.volume(vname, G)
    cam = rv.camera(camname, W, H)
    ctx.tsdf_volume(G, vol.origin, vol.h, 4 * vol.h)
    ctx.tsdf_upload(vol.sum, vol.count)
    exp = rm.raycast(vol, _mats(ctx, cam), W, H, mo, step)
    got = ctx.tsdf_raycast(cam, mo, step)
    assert int((got[0] < 1).sum()) >= least_hits and int((got[0] == 1).sum()) >= least_empty
    _same(got, exp, name)
    _plain(ctx, True)
    try:
        _same(ctx.tsdf_raycast(cam, mo, step), exp, name + " (plain march)")
    finally:
        _plain(ctx, False)


def test_upload_fetch_integrate_and_clear():
    W, H, G = 67, 45, 25
    ctx = _context(W, H)
    vol = rv.volume("random", G)
    ctx.tsdf_volume(G, vol.origin, vol.h, 4 * vol.h)
    ctx.tsdf_upload(vol.sum, vol.count)
    s, c = ctx.tsdf_fetch()
    assert s.tobytes() == vol.sum.tobytes() and np.array_equal(c, vol.count)
    # integrate a map on top of the uploaded fields
    cam = rv.camera("front", W, H)
    depth = np.full((H, W), 0.2, f32)
    depth[::3, ::2] = 1.0
    ctx.depth_upload(0, cam, depth)
    mats = ctx.depth_slot_matrices(0)
    ctx.tsdf_integrate([0])
    s2, c2 = ctx.tsdf_fetch()
    vol.integrate({0: tm.wmap(depth, None, mats)}, {0: mats}, [0])
    assert (c2 != c).any()
    assert s2.tobytes() == vol.sum.tobytes() and np.array_equal(c2, vol.count)
    ctx.tsdf_volume(G, vol.origin, vol.h, 4 * vol.h)
    s3, c3 = ctx.tsdf_fetch()
    assert not s3.any() and not c3.any()


def _turn_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])


@pytest.fixture(scope="module")
def store160():
    """tests/test_tsdf_gpu.py's kind of store at 160 x 120: five ring cameras' exact maps, one of them with NaN and 1.0 holes"""
    W, H = 160, 120
    sc = synth.Scene()
    rng = np.random.Generator(np.random.PCG64(0x8A7C))
    centres = rv.ring_centres()
    cams = [synth.camera_at(c, W, H) for c in centres]
    depths = [sc.render(c, W, H, want_depth=True)[1] for c in centres]
    pick = rng.random((H, W))
    depths[1][pick < 0.1] = np.nan
    depths[1][(pick >= 0.1) & (pick < 0.2)] = 1.0
    return W, H, cams, depths


def _integrated(ctx, store, G, slots):
    W, H, cams, depths = store
    origin, h = np.array([-1.7, -1.7, -4.7], f32), f32(3.4 / (G - 1))
    ctx.depth_store(len(depths) + 1)
    for s in range(len(depths)):
        ctx.depth_upload(s, cams[s], depths[s])
    ctx.tsdf_volume(G, origin, h, 4 * h)
    ctx.tsdf_integrate(slots)
    mats = {s: ctx.depth_slot_matrices(s) for s in range(len(depths))}
    vol = tm.Volume(G, origin, h, 4 * h)
    vol.integrate({s: tm.wmap(depths[s], None, mats[s]) for s in mats}, mats, slots)
    return vol, mats


def _cam_mats(ctx, cam, slot):
    ctx.depth_upload(slot, cam, np.ones((ctx.H, ctx.W), f32))
    return ctx.depth_slot_matrices(slot)


def test_integrated_volume_from_a_stored_and_a_turned_camera(store160):
    W, H, cams, depths = store160
    G = 50
    with mvs_amd.Context(W, H) as ctx:
        vol, mats = _integrated(ctx, store160, G, [0, 1, 2, 3, 4, 1])
        for mo in (1, 3):
            got = ctx.tsdf_raycast(cams[2], mo, 0.5)
            assert (got[0] < 1).mean() > 0.5
            _same(got, rm.raycast(vol, mats[2], W, H, mo, 0.5), "stored camera, min_observations %d" % mo)
        turned = synth.camera_at((0.9, 0.0, -0.2), W, H, rot=_turn_y(20.0))
        tm_ = _cam_mats(ctx, turned, 5)
        got = ctx.tsdf_raycast(turned, 1, 1.0)
        assert (got[0] < 1).mean() > 0.3 and (got[0] == 1).any()
        _same(got, rm.raycast(vol, tm_, W, H, 1, 1.0), "turned camera")


def test_exact_maps_end_to_end():
    """the CPU test's setup and bounds on the GPU: five ring cameras at 320 x 240, G = 64, truncation 4 h, step 0.5, into cameras 0 and 1"""
    W, H, G = rv.RING_W, rv.RING_H, rv.RING_G
    sc = synth.Scene()
    centres = rv.ring_centres()
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(5)
        cams, exact = [], []
        for s, c in enumerate(centres):
            cams.append(synth.camera_at(c, W, H))
            exact.append(sc.render(c, W, H, want_depth=True)[1])
            ctx.depth_upload(s, cams[s], exact[s])
        ctx.tsdf_volume(G, rv.RING_ORIGIN, rv.RING_H_NODE, 4 * rv.RING_H_NODE)
        ctx.tsdf_integrate(range(5))
        for s in (0, 1):
            depth, normals = ctx.tsdf_raycast(cams[s], 1, 0.5)
            f = rv.exact_map_figures(depth, normals, cams[s], centres[s], exact[s])
            print("exact maps, GPU, camera %d: %s" % (s, f))
            rv.assert_exact_map_figures(f)


def test_the_raycast_map_is_an_input_of_the_depth_store(store160):
    """the map goes device to device into a slot; mvs_fuse_depth with that slot as reference and mvs_tsdf_integrate of it into a fresh volume
    equal their mirrors fed with the mirror's map"""
    W, H, cams, depths = store160
    G = 50
    with mvs_amd.Context(W, H) as ctx:
        vol, mats = _integrated(ctx, store160, G, [0, 1, 2, 3, 4])
        cam = cams[0]
        ctx.tsdf_raycast(cam, 1, 0.5, fetch=False)
        dptr, nptr = ctx.tsdf_raycast_pointers()
        assert dptr and nptr
        ctx.depth_upload_device(5, cam, dptr)
        mats[5] = ctx.depth_slot_matrices(5)
        ray_depth, _ = rm.raycast(vol, mats[5], W, H, 1, 0.5)
        assert (ray_depth < 1).mean() > 0.9
        kw = dict(min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01)
        got = ctx.fuse_depth(5, [2, 3, 4], **kw)
        all_depths = dict(enumerate(depths))
        all_depths[5] = ray_depth
        exp = fm.fuse(all_depths, {}, mats, 5, [2, 3, 4], **kw)
        assert len(got) > 0.5 * W * H and got.shape == exp["rows"].shape
        assert np.array_equal(got.view(np.uint32), exp["rows"].view(np.uint32))
        ctx.tsdf_volume(G, vol.origin, vol.h, 4 * vol.h)
        ctx.tsdf_integrate([5])
        s, c = ctx.tsdf_fetch()
        fresh = tm.Volume(G, vol.origin, vol.h, 4 * vol.h).integrate({5: tm.wmap(ray_depth, None, mats[5])}, mats, [5])
        assert c.max() == 1 and np.array_equal(c, fresh.count) and s.tobytes() == fresh.sum.tobytes()


def test_state_and_order(store160):
    import torch
    W, H, cams, depths = store160
    G = 50
    lib = mvs_amd.load_library()
    with mvs_amd.Context(W, H) as ctx:
        vol, mats = _integrated(ctx, store160, G, [0, 1, 2])
        cam = cams[3]
        # integrate, then raycast, nothing synchronising in between (_integrated's mirror work aside: queue both again)
        ctx.tsdf_integrate([3])
        ctx.tsdf_raycast(cam, 1, 0.5, fetch=False)
        vol.integrate({3: tm.wmap(depths[3], None, mats[3])}, mats, [3])
        exp = rm.raycast(vol, mats[3], W, H, 1, 0.5)
        first = ctx.tsdf_raycast(cam, 1, 0.5, fetch=True)   # (the second identical call; the fetch returns its maps)
        _same(first, exp, "integrate then raycast")
        d0, n0 = np.empty((H, W), f32), np.empty((H, W, 3), f32)
        ctx._check(lib.mvs_tsdf_raycast_fetch(ctx.h, d0.ctypes.data_as(C.POINTER(C.c_float)), None))
        ctx._check(lib.mvs_tsdf_raycast_fetch(ctx.h, None, n0.ctypes.data_as(C.POINTER(C.c_float))))
        assert d0.tobytes() == first[0].tobytes() and n0.tobytes() == first[1].tobytes()
        assert (first[0] < 1).mean() > 0.5
        again = ctx.tsdf_raycast(cam, 1, 0.5)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        # a camera facing away leaves all-empty maps: every pixel is written
        away = synth.camera_at((0.0, 0.0, 0.0), W, H, rot=rv.HALF_TURN)
        d, n = ctx.tsdf_raycast(away, 1, 0.5)
        assert (d == 1).all() and not n.any()
        # mvs_tsdf_volume and mvs_depth_store do not touch the maps; raycast, integrate more, raycast again
        ctx.tsdf_raycast(cam, 1, 0.5, fetch=False)
        ctx.tsdf_integrate([4])
        vol.integrate({4: tm.wmap(depths[4], None, mats[4])}, mats, [4])
        _same(ctx.tsdf_raycast(cam, 1, 0.5), rm.raycast(vol, mats[3], W, H, 1, 0.5), "after integrating more")
        # mvs_tsdf_surface with another min_observations between two raycasts changes nothing, and still equals surface_nets
        exp1 = rm.raycast(vol, mats[3], W, H, 1, 1.0)
        _same(ctx.tsdf_raycast(cam, 1, 1.0), exp1, "before the surface")
        v, f = ctx.tsdf_surface(3)
        _same(ctx.tsdf_raycast(cam, 1, 1.0), exp1, "after the surface")
        rv_, rf = vol.surface(3)
        assert len(f) > 100 and np.array_equal(f, rf) and np.abs(v - rv_).max() <= 2e-6 * float(np.abs(vol.origin).max() + G * vol.h)
        v1, f1 = ctx.tsdf_surface(1)
        assert np.array_equal(f1, vol.surface(1)[1])
        # a caller's stream
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        try:
            ctx.tsdf_integrate([0])
            vol.integrate({0: tm.wmap(depths[0], None, mats[0])}, mats, [0])
            _same(ctx.tsdf_raycast(cam, 2, 0.5), rm.raycast(vol, mats[3], W, H, 2, 0.5), "on the caller's stream")
        finally:
            ctx.set_stream(0)
        # the maps survive a new volume and a new depth store
        last = ctx.tsdf_raycast(cam, 2, 0.5)
        ctx.tsdf_volume(16, vol.origin, vol.h, 4 * vol.h)
        ctx.depth_store(2)
        ctx._check(lib.mvs_tsdf_raycast_fetch(ctx.h, d0.ctypes.data_as(C.POINTER(C.c_float)), n0.ctypes.data_as(C.POINTER(C.c_float))))
        assert d0.tobytes() == last[0].tobytes() and n0.tobytes() == last[1].tobytes()
        # an empty volume: nothing is observed, nothing is hit
        d, n = ctx.tsdf_raycast(cam, 1, 0.5)
        assert (d == 1).all() and not n.any()


def test_errors():
    lib = mvs_amd.load_library()
    W, H = 64, 48
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    cam = synth.camera_at((0.0, 0.0, 0.0), W, H)
    o = np.array([-1.0, -1.0, -4.0], f32)
    s, c = np.zeros((16, 16, 16), f32), np.zeros((16, 16, 16), np.int32)
    d, n = np.empty((H, W), f32), np.empty((H, W, 3), f32)
    with mvs_amd.Context(W, H) as ctx:
        h = ctx.h
        # before mvs_tsdf_volume
        assert lib.mvs_tsdf_upload(h, fp(s), ip(c)) == ESTATE
        assert lib.mvs_tsdf_raycast(h, fp(cam), 1, 0.5) == ESTATE
        assert lib.mvs_tsdf_raycast_fetch(h, fp(d), fp(n)) == ESTATE
        assert not lib.mvs_tsdf_raycast_depth_device(h) and not lib.mvs_tsdf_raycast_normals_device(h)
        assert ctx.tsdf_raycast_pointers() == (0, 0)
        with pytest.raises(mvs_amd.MvsError):
            ctx.tsdf_upload(s, c)
        ctx.tsdf_volume(16, o, 2.0 / 15, 8.0 / 15)
        assert lib.mvs_tsdf_raycast_fetch(h, fp(d), fp(n)) == ESTATE     # no raycast yet
        assert lib.mvs_tsdf_upload(h, None, ip(c)) == EINVAL and lib.mvs_tsdf_upload(h, fp(s), None) == EINVAL
        assert lib.mvs_tsdf_raycast(h, None, 1, 0.5) == EINVAL
        assert lib.mvs_tsdf_raycast(h, fp(cam), 0, 0.5) == EINVAL and lib.mvs_tsdf_raycast(h, fp(cam), -2, 0.5) == EINVAL
        for bad in (0.0, 0.06, 4.01, -0.5, inf, float("nan")):
            assert lib.mvs_tsdf_raycast(h, fp(cam), 1, bad) == EINVAL, bad
        nan_cam = cam.copy()
        nan_cam[1, 2] = np.nan
        inf_cam = cam.copy()
        inf_cam[0, 0] = np.inf
        singular = cam.copy()
        singular[2] = singular[3]
        affine = np.eye(4, dtype=f32)                                    # rows x, y, w = e0, e1, e3: the centre lies at infinity
        for bad in (nan_cam, inf_cam, singular, np.zeros((4, 4), f32), affine):
            assert lib.mvs_tsdf_raycast(h, fp(np.ascontiguousarray(bad)), 1, 0.5) == EINVAL
        assert lib.mvs_tsdf_raycast_fetch(h, fp(d), fp(n)) == ESTATE     # refused calls did not count as a raycast
        for ok in (0.0625, 4.0):
            assert lib.mvs_tsdf_raycast(h, fp(cam), 1, ok) == 0
        assert lib.mvs_tsdf_raycast_fetch(h, None, None) == 0
        assert lib.mvs_tsdf_raycast_fetch(h, fp(d), fp(n)) == 0 and (d == 1).all() and not n.any()
        assert lib.mvs_tsdf_raycast_depth_device(h) and lib.mvs_tsdf_raycast_normals_device(h)
        assert lib.mvs_tsdf_upload(h, fp(s), ip(c)) == 0
