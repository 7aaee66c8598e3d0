"""The TSDF volume's appearance on the GPU (csrc/tsdf.hip: mvs_tsdf_integrate_frames; csrc/appearance.hip: mvs_tsdf_shade,
mvs_tsdf_sample_appearance): cells, shaded maps and sampled values against tests/appearance_mirror.py bit for bit, with the matrices of
mvs_depth_slot_matrices -- pairing, chunks and batches; the TSDF fields against mvs_tsdf_integrate's; split lists and repeats; saturation;
crafted cells through mvs_tsdf_appearance_upload; depth maps from three sources; life cycle and stream order; the accuracy bounds of
tests/test_appearance_cpu.py; the error cases.  The inputs are tests/appearance_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import appearance_cases as ac
import appearance_mirror as am
import mvs_amd
import raycast_mirror as rm
import tsdf_mirror as tm
from mvs_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
EINVAL, ESTATE = -1, -3
inf = float("inf")


def _fill(ctx, st):
    """the depth store and the frame store of appearance_cases.store -> the kernels' matrices per depth slot"""
    ctx.depth_store(ac.DEPTH_CAP)
    ctx.frame_store(ac.FRAME_CAP)
    for s in range(ac.DEPTH_CAP):
        ctx.depth_upload(s, st["cams"][s], st["depths"][s], st["costs"][s])
    for fs, img in st["frames"].items():
        ctx.frame_upload(fs, img)
    return {s: ctx.depth_slot_matrices(s) for s in range(ac.DEPTH_CAP)}


def _integrate(ctx, pairs, **kw):
    ctx.tsdf_integrate_frames([d for d, _ in pairs], [f for _, f in pairs], **kw)


def _same_cells(got, exp, what):
    bad = got != exp
    assert not bad.any(), "%s: %d cells differ; first %s: %#x vs %#x" % (what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], exp[bad][0])


def _same_fields(got, exp_sum, exp_count, what):
    s, c = got
    assert np.array_equal(c, exp_count), "%s: %d counts differ" % (what, int((c != exp_count).sum()))
    assert s.tobytes() == exp_sum.tobytes(), "%s: %d sums differ" % (what, int((s.view(u32) != exp_sum.view(u32)).sum()))


def _same_values(got, exp, what):
    assert np.array_equal(got != got, exp != exp), "%s: NaN masks differ at %s" % (what, np.nonzero((got != got) != (exp != exp))[0][:8])
    bad = got.view(u32) != exp.view(u32)
    assert not bad.any(), "%s: %d values differ; first %d: %r vs %r" % (what, int(bad.sum()), np.nonzero(bad)[0][0], got[bad][0], exp[bad][0])


def _same_map(got, exp, what):
    bad = (got != exp).any(-1)
    assert not bad.any(), "%s: %d pixels differ; first %s: %r vs %r" % (what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], exp[bad][0])


@pytest.mark.parametrize("size", ac.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("G", ac.GRIDS)
def test_pairing_chunks_and_batches(G, size):
    """every prefix length of the pair list from a cleared volume, then a list under a finite max_cost on top: cells and TSDF fields equal the
    mirror's; the TSDF fields equal mvs_tsdf_integrate's on the same depth slots; one pair per call and a second run give the same bytes"""
    W, H = size
    st = ac.store(W, H)
    origin, h = ac.cube(G)
    with mvs_amd.Context(W, H) as ctx:
        mats = _fill(ctx, st)
        snaps, final = ac.mirror_snapshots(st, mats, G)
        for n in ac.LENGTHS:
            ctx.tsdf_volume(G, origin, h, 4 * h)
            _integrate(ctx, ac.PAIRS[:n])
            cells = ctx.tsdf_appearance_fetch()
            es, ec, ecells = snaps[n]
            _same_cells(cells, ecells, "%d pairs" % n)
            _same_fields(ctx.tsdf_fetch(), es, ec, "%d pairs" % n)
        votes, _ = am.split(cells)
        assert votes.max() >= 8 and (votes > 0).mean() > 0.01 and (ec > votes).any()
        _integrate(ctx, ac.PAIRS_COST, max_cost=ac.MAX_COST)
        cells = ctx.tsdf_appearance_fetch()
        fields = ctx.tsdf_fetch()
        assert (cells != ecells).any()
        _same_cells(cells, final.cells, "finite max_cost")
        _same_fields(fields, final.sum, final.count, "finite max_cost")
        # mvs_tsdf_integrate on the same depth slots: the same TSDF bytes, and no appearance
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate([d for d, _ in ac.PAIRS])
        ctx.tsdf_integrate([d for d, _ in ac.PAIRS_COST], max_cost=ac.MAX_COST)
        plain = ctx.tsdf_fetch()
        assert plain[0].tobytes() == fields[0].tobytes() and np.array_equal(plain[1], fields[1])
        with pytest.raises(mvs_amd.MvsError):
            ctx.tsdf_appearance_fetch()
        # one pair per call, and a second run of the same calls
        for _ in range(2):
            ctx.tsdf_volume(G, origin, h, 4 * h)
            for p in ac.PAIRS:
                _integrate(ctx, [p])
            for p in ac.PAIRS_COST:
                _integrate(ctx, [p], max_cost=ac.MAX_COST)
            _same_cells(ctx.tsdf_appearance_fetch(), final.cells, "one pair per call")
            _same_fields(ctx.tsdf_fetch(), final.sum, final.count, "one pair per call")


def test_saturation():
    """one pair listed 260 times at G = 16: the band's cells read 255 << 24 | 255 I while the TSDF count reads 260"""
    W, H = ac.SIZES[0]
    G = 16
    st = ac.store(W, H)
    origin, h = ac.cube(G)
    pair = (0, ac.FRAME_OF[0])
    with mvs_amd.Context(W, H) as ctx:
        mats = _fill(ctx, st)
        ctx.tsdf_volume(G, origin, h, 4 * h)
        _integrate(ctx, [pair])
        once = ctx.tsdf_appearance_fetch()
        ctx.tsdf_volume(G, origin, h, 4 * h)
        _integrate(ctx, [pair] * 260)
        full = ctx.tsdf_appearance_fetch()
        _, count = ctx.tsdf_fetch()
    n1, s1 = am.split(once)
    band = n1 == 1
    assert band.sum() > 50 and n1.max() == 1
    assert np.array_equal(full, ac.pack(255 * n1, 255 * s1))
    assert (count[band] == 260).all()
    maps = {0: tm.wmap(st["depths"][0], None, mats[0])}
    exp = am.Volume(G, origin, h, 4 * h).integrate_frames(maps, mats, st["frames"], [pair])
    _same_cells(once, exp.cells, "one vote")


POINT_SETS = ac.point_sets()
DEPTH_MAPS = ac.depth_maps()


@pytest.fixture(scope="module")
def crafted_ctx():
    with mvs_amd.Context(ac.CRAFT_W, ac.CRAFT_H) as ctx:
        ctx.depth_store(2)
        yield ctx


def _upload_crafted(ctx, cells):
    ctx.tsdf_volume(ac.CG, ac.CORIGIN, ac.CH, 4 * ac.CH)
    ctx.tsdf_appearance_upload(cells)
    assert np.array_equal(ctx.tsdf_appearance_fetch(), cells)


@pytest.mark.parametrize("name", sorted(POINT_SETS))
def test_sample_on_crafted_cells(crafted_ctx, name):
    cells, pts, expect = POINT_SETS[name]
    ctx = crafted_ctx
    _upload_crafted(ctx, cells)
    got = ctx.tsdf_sample_appearance(pts)
    if expect == "all":
        assert (got == got).all()
    elif expect == "none":
        assert (got != got).all()
    _same_values(got, am.sample(ac.crafted_volume(cells), pts), name)


@pytest.mark.parametrize("name", sorted(DEPTH_MAPS))
def test_shade_on_crafted_cells(crafted_ctx, name):
    import torch
    cells, cam, depth, least_shaded, least_empty = DEPTH_MAPS[name]
    ctx = crafted_ctx
    _upload_crafted(ctx, cells)
    ctx.depth_upload(0, cam, depth)
    mats = ctx.depth_slot_matrices(0)
    dev = torch.as_tensor(depth, device="cuda")
    torch.cuda.synchronize()
    got = ctx.tsdf_shade(cam, dev.data_ptr())
    have = got[..., 1] == 255
    assert have.sum() >= least_shaded and (~have).sum() >= least_empty
    _same_map(got, am.shade(ac.crafted_volume(cells), mats, depth), name)
    # the stored copy of the same map, through its device address
    assert ctx.depth_slot_pointer(0) and not ctx.depth_slot_pointer(1) and not ctx.depth_slot_pointer(2)
    again = ctx.tsdf_shade(cam, ctx.depth_slot_pointer(0))
    assert again.tobytes() == got.tobytes()


def test_shading_maps_from_three_sources_and_sampling_the_mesh():
    """an integrated volume: the ray-cast's map shaded device to device, a map in the sweep's convention uploaded by the test (a stored camera's
    exact map with holes), a depth-store slot's map by its device address; and the grey levels of mvs_tsdf_surface's vertices"""
    import torch
    W, H = ac.SIZES[1]
    G = 50
    st = ac.store(W, H)
    origin, h = ac.cube(G)
    with mvs_amd.Context(W, H) as ctx:
        mats = _fill(ctx, st)
        _, vol = ac.mirror_snapshots(st, mats, G)
        ctx.tsdf_volume(G, origin, h, 4 * h)
        _integrate(ctx, ac.PAIRS)
        _integrate(ctx, ac.PAIRS_COST, max_cost=ac.MAX_COST)
        cam = st["cams"][3]
        ctx.tsdf_raycast(cam, 1, 0.5, fetch=False)
        got = ctx.tsdf_shade(cam, ctx.tsdf_raycast_pointers()[0])
        ray_depth, _ = rm.raycast(vol, mats[3], W, H, 1, 0.5)
        assert (got[..., 1] == 255).mean() > 0.5
        _same_map(got, am.shade(vol, mats[3], ray_depth), "the ray-cast's map")
        ptr = ctx.tsdf_shade_pointer()
        assert ptr
        on_dev = torch.as_tensor(mvs_amd._DeviceArray(ptr, (H, W, 2), "|u1"), device="cuda").cpu().numpy()
        assert on_dev.tobytes() == got.tobytes()
        holes = np.array(st["depths"][7])          # (a writable copy: the store's arrays are read-only)
        dev = torch.as_tensor(holes, device="cuda")
        torch.cuda.synchronize()
        got = ctx.tsdf_shade(st["cams"][7], dev.data_ptr())
        exp = am.shade(vol, mats[7], holes)
        assert 0.5 < (exp[..., 1] == 255).mean() < 0.9
        _same_map(got, exp, "an uploaded map with holes")
        got = ctx.tsdf_shade(st["cams"][2], ctx.depth_slot_pointer(2))
        _same_map(got, am.shade(vol, mats[2], st["depths"][2]), "a depth-store slot's map")
        v, f = ctx.tsdf_surface(1)
        grey = ctx.tsdf_sample_appearance(v)
        assert len(v) > 1000 and (grey == grey).mean() > 0.9
        _same_values(grey, am.sample(vol, v), "the mesh's vertices")


def test_life_cycle_and_stream_order():
    W, H = ac.SIZES[0]
    G = 50
    st = ac.store(W, H)
    origin, h = ac.cube(G)
    lib = mvs_amd.load_library()
    with mvs_amd.Context(W, H) as ctx:
        mats = _fill(ctx, st)
        maps = {s: tm.wmap(st["depths"][s], None, mats[s]) for s in range(ac.DEPTH_CAP)}
        vol = am.Volume(G, origin, h, 4 * h)
        ctx.tsdf_volume(G, origin, h, 4 * h)
        # integrate, raycast and shade queued back to back, nothing synchronising in between
        cam = st["cams"][1]
        _integrate(ctx, ac.PAIRS[:5])
        ctx.tsdf_raycast(cam, 1, 0.5, fetch=False)
        ctx.tsdf_shade(cam, ctx.tsdf_raycast_pointers()[0], fetch=False)
        _integrate(ctx, ac.PAIRS[5:9])                      # (queued behind the shade: it must not show in the map)
        vol.integrate_frames(maps, mats, st["frames"], ac.PAIRS[:5])
        exp = am.shade(vol, mats[1], rm.raycast(vol, mats[1], W, H, 1, 0.5)[0])
        got = np.empty((H, W, 2), np.uint8)
        ctx._check(lib.mvs_tsdf_shade_fetch(ctx.h, got.ctypes.data_as(C.POINTER(C.c_uint8))))
        assert (got[..., 1] == 255).mean() > 0.5
        _same_map(got, exp, "integrate, raycast, shade")
        vol.integrate_frames(maps, mats, st["frames"], ac.PAIRS[5:9])
        _same_cells(ctx.tsdf_appearance_fetch(), vol.cells, "integrated behind the shade")
        # mvs_tsdf_integrate and mvs_tsdf_upload leave the appearance as it is
        before = ctx.tsdf_appearance_fetch()
        ctx.tsdf_integrate([2, 3])
        assert np.array_equal(ctx.tsdf_appearance_fetch(), before)
        s, c = ctx.tsdf_fetch()
        ctx.tsdf_upload(np.zeros_like(s), np.zeros_like(c))
        assert np.array_equal(ctx.tsdf_appearance_fetch(), before)
        pts = np.concatenate([origin + np.random.Generator(np.random.PCG64(3)).random((500, 3)) * 3.4, np.ones((500, 1))], 1).astype(f32)
        vals = ctx.tsdf_sample_appearance(pts)
        assert 10 < (vals == vals).sum() < 490
        _same_values(vals, am.sample(vol, pts), "independent of the TSDF fields")
        # checkpoint and resume: upload into a fresh volume, integrate on top
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_appearance_upload(before)
        _integrate(ctx, ac.PAIRS[9:12])
        vol.integrate_frames(maps, mats, st["frames"], ac.PAIRS[9:12])
        _same_cells(ctx.tsdf_appearance_fetch(), vol.cells, "resumed")
        # mvs_tsdf_volume drops the appearance; the next integration starts from zero; the shaded map survives
        ctx.tsdf_volume(G, origin, h, 4 * h)
        with pytest.raises(mvs_amd.MvsError):
            ctx.tsdf_appearance_fetch()
        assert lib.mvs_tsdf_shade(ctx.h, cam.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(ctx.depth_slot_pointer(0))) == ESTATE
        kept = np.empty((H, W, 2), np.uint8)
        ctx._check(lib.mvs_tsdf_shade_fetch(ctx.h, kept.ctypes.data_as(C.POINTER(C.c_uint8))))
        assert kept.tobytes() == got.tobytes()
        _integrate(ctx, ac.PAIRS[:2])
        fresh = am.Volume(G, origin, h, 4 * h).integrate_frames(maps, mats, st["frames"], ac.PAIRS[:2])
        _same_cells(ctx.tsdf_appearance_fetch(), fresh.cells, "after a new volume")
        # a smaller volume after a larger one
        o16, h16 = ac.cube(16)
        ctx.tsdf_volume(16, o16, h16, 4 * h16)
        _integrate(ctx, ac.PAIRS[:3])
        small = am.Volume(16, o16, h16, 4 * h16).integrate_frames(maps, mats, st["frames"], ac.PAIRS[:3])
        _same_cells(ctx.tsdf_appearance_fetch(), small.cells, "a smaller volume")


def test_exact_maps_end_to_end():
    """tests/test_appearance_cpu.py's acceptance case on the GPU, with the same bounds"""
    cams, depths, frames = ac.accuracy_inputs()
    W, H, G = ac.ACC_W, ac.ACC_H, ac.ACC_G
    origin, h = ac.cube(G)
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(5)
        ctx.frame_store(5)
        for s in range(5):
            ctx.depth_upload(s, cams[s], depths[s])
            ctx.frame_upload(s, frames[s])
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate_frames(range(5), range(5))
        for s in (0, 1):
            ray_depth, _ = ctx.tsdf_raycast(cams[s], 1, 0.5)
            shaded = ctx.tsdf_shade(cams[s], ctx.tsdf_raycast_pointers()[0])
            f = ac.accuracy_figures(ray_depth, shaded, frames[s])
            print("shaded ray-cast, GPU, camera %d: %s" % (s, f))
            ac.assert_accuracy_figures(f)


def test_errors():
    lib = mvs_amd.load_library()
    W, H = 64, 48
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))     # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))     # noqa: E731
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))    # noqa: E731
    bp = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))     # noqa: E731
    sl = lambda *s: np.asarray(s, np.int32)                   # noqa: E731
    cam = synth.camera_at((0.0, 0.0, 0.0), W, H)
    d = np.full((H, W), 0.5, f32)
    img = np.full((H, W), 7, np.uint8)
    o = np.array([-1.0, -1.0, -4.0], f32)
    cells = np.zeros((16, 16, 16), u32)
    pts = np.ones((3, 4), f32)
    out = np.zeros(3, f32)
    shaded = np.zeros((H, W, 2), np.uint8)
    with mvs_amd.Context(W, H) as ctx:
        h = ctx.h
        ctx.depth_store(4)
        ctx.frame_store(3)
        assert lib.mvs_depth_upload(h, 0, fp(cam), fp(d), fp(d)) == 0 and lib.mvs_depth_upload(h, 1, fp(cam), fp(d), None) == 0
        ctx.frame_upload(0, img)
        ctx.frame_upload(2, img)
        dptr = C.c_void_p(ctx.depth_slot_pointer(0))
        s0 = sl(0)
        # before mvs_tsdf_volume
        assert lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), ip(s0), inf) == ESTATE
        assert lib.mvs_tsdf_appearance_fetch(h, up(cells)) == ESTATE and lib.mvs_tsdf_appearance_upload(h, up(cells)) == ESTATE
        assert lib.mvs_tsdf_shade(h, fp(cam), dptr) == ESTATE
        assert lib.mvs_tsdf_sample_appearance(h, fp(pts), 3, fp(out)) == ESTATE
        assert lib.mvs_tsdf_shade_fetch(h, bp(shaded)) == ESTATE and not lib.mvs_tsdf_shade_device(h) and ctx.tsdf_shade_pointer() == 0
        with pytest.raises(mvs_amd.MvsError):
            ctx.tsdf_appearance_fetch()
        with pytest.raises(mvs_amd.MvsError):
            ctx.tsdf_appearance_upload(cells)
        ctx.tsdf_volume(16, o, 2.0 / 15, 8.0 / 15)
        # a volume, but no appearance yet
        assert lib.mvs_tsdf_appearance_fetch(h, up(cells)) == ESTATE
        assert lib.mvs_tsdf_shade(h, fp(cam), dptr) == ESTATE
        assert lib.mvs_tsdf_sample_appearance(h, fp(pts), 3, fp(out)) == ESTATE
        # mvs_tsdf_integrate_frames' arguments
        assert lib.mvs_tsdf_integrate_frames(h, 1, None, ip(s0), inf) == EINVAL and lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), None, inf) == EINVAL
        assert lib.mvs_tsdf_integrate_frames(h, 0, ip(s0), ip(s0), inf) == EINVAL and lib.mvs_tsdf_integrate_frames(h, -3, ip(s0), ip(s0), inf) == EINVAL
        assert lib.mvs_tsdf_integrate_frames(h, 1, ip(sl(4)), ip(s0), inf) == EINVAL and lib.mvs_tsdf_integrate_frames(h, 1, ip(sl(-1)), ip(s0), inf) == EINVAL
        assert lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), ip(sl(3)), inf) == EINVAL and lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), ip(sl(-1)), inf) == EINVAL
        assert lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), ip(s0), -1.0) == EINVAL and lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), ip(s0), float("nan")) == EINVAL
        assert lib.mvs_tsdf_integrate_frames(h, 2, ip(sl(0, 2)), ip(sl(0, 0)), inf) == ESTATE     # depth slot 2 is unfilled
        assert lib.mvs_tsdf_integrate_frames(h, 2, ip(sl(0, 1)), ip(sl(0, 1)), inf) == ESTATE     # frame slot 1 is unfilled
        assert lib.mvs_tsdf_integrate_frames(h, 2, ip(sl(0, 1)), ip(sl(0, 2)), 0.5) == ESTATE     # depth slot 1 has no cost map
        assert lib.mvs_tsdf_appearance_fetch(h, up(cells)) == ESTATE                                # refused calls made no appearance
        assert lib.mvs_tsdf_appearance_upload(h, None) == EINVAL
        assert lib.mvs_tsdf_integrate_frames(h, 2, ip(sl(0, 1)), ip(sl(0, 2)), inf) == 0
        assert lib.mvs_tsdf_integrate_frames(h, 1, ip(s0), ip(sl(2)), 0.75) == 0
        assert lib.mvs_tsdf_appearance_fetch(h, None) == EINVAL
        assert lib.mvs_tsdf_appearance_fetch(h, up(cells)) == 0
        n, s = am.split(cells)
        assert n.max() == 3 and np.array_equal(s, 7 * n)
        # mvs_tsdf_shade, _shade_fetch, _sample_appearance
        assert lib.mvs_tsdf_shade_fetch(h, bp(shaded)) == ESTATE     # no shade yet
        assert lib.mvs_tsdf_shade(h, None, dptr) == EINVAL and lib.mvs_tsdf_shade(h, fp(cam), None) == EINVAL
        nan_cam = cam.copy()
        nan_cam[1, 2] = np.nan
        singular = cam.copy()
        singular[2] = singular[3]
        for bad in (nan_cam, singular, np.zeros((4, 4), f32), np.eye(4, dtype=f32)):
            assert lib.mvs_tsdf_shade(h, fp(np.ascontiguousarray(bad)), dptr) == EINVAL
        assert lib.mvs_tsdf_shade_fetch(h, bp(shaded)) == ESTATE     # refused calls did not count as a shade
        assert lib.mvs_tsdf_shade(h, fp(cam), dptr) == 0
        assert lib.mvs_tsdf_shade_fetch(h, None) == EINVAL
        assert lib.mvs_tsdf_shade_fetch(h, bp(shaded)) == 0 and lib.mvs_tsdf_shade_device(h)
        assert lib.mvs_tsdf_sample_appearance(h, None, 3, fp(out)) == EINVAL and lib.mvs_tsdf_sample_appearance(h, fp(pts), 3, None) == EINVAL
        assert lib.mvs_tsdf_sample_appearance(h, fp(pts), 0, fp(out)) == EINVAL and lib.mvs_tsdf_sample_appearance(h, fp(pts), -1, fp(out)) == EINVAL
        assert lib.mvs_tsdf_sample_appearance(h, fp(pts), 3, fp(out)) == 0
        assert lib.mvs_depth_slot_device(h, -1) is None and lib.mvs_depth_slot_device(h, 4) is None and lib.mvs_depth_slot_device(h, 2) is None
