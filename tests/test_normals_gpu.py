"""DESIGN.md section 31 on the device (csrc/normals.hip), bit for bit against tests/normals_mirror.py: mvs_propagate_normals on the state the
stage holds (fetched, so the propagation's own mirror is not in the loop), the normal planes of the depth store, mvs_fuse_depth_normals on
every crafted case of tests/normals_cases.py with its identities against the device's own mvs_fuse_depth_masked / mvs_fuse_depth, and the
Python layer through propagate_two_stage(normals=True)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fusion_cases as fc
import mvs_amd
import normals_cases as nc
import normals_mirror as nm

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
f32 = np.float32
u32 = np.uint32
INF = float("inf")
_fp = C.POINTER(C.c_float)


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, f32), np.ascontiguousarray(ref, f32)
    assert got.shape == ref.shape, what
    bad = np.argwhere(got.view(u32) != ref.view(u32))
    assert len(bad) == 0, "%s: %d of %d values differ; first at %s: %r, expected %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


# ---- mvs_propagate_normals ------------------------------------------------------------------------------------------------------------------
def _start_map(W, H, seed):
    """a noisy ramp with a depth step down the middle and fusion_cases' blocks of Z_TIES"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    start = (-0.3 + 0.3 * x / W + 0.004 * y + rng.uniform(-0.02, 0.02, (H, W)) + 0.35 * (x >= W // 2)).astype(f32)
    return fc.place_z_ties(start)


@pytest.mark.parametrize("W,H", [(64, 32), (200, 20), (131, 67)])   # 2 x 2 propagation tiles; ragged; the fusion's odd size
def test_propagate_normals_equal_rule_n1_on_the_fetched_state(W, H):
    cams = fc.cameras(W, H)
    rng = np.random.Generator(np.random.PCG64(0x31A + W))
    frames = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)]
    start = _start_map(W, H, 0x31B + H)
    assert sum(bool(np.any(start.view(u32) == np.asarray(z, f32).view(u32))) for z in fc.Z_TIES) == len(fc.Z_TIES)
    for main in (fc.TILTED, fc.ROLLED, fc.SHIFTED):
        sides = [c for c in fc.VOTING if c != main][:2]
        what = "%d x %d, camera %d" % (W, H, main)
        with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
            lib, h = ctx.lib, ctx.h
            cam = np.ascontiguousarray(cams[main], f32)
            out = np.empty((H, W, 3), f32)
            assert lib.mvs_propagate_normals(h, cam.ctypes.data_as(_fp)) == ESTATE and b"mvs_propagate_init first" in lib.mvs_last_error(h)
            assert ctx.propagate_normals_pointer() == 0 and lib.mvs_propagate_normals_fetch(h, out.ctypes.data_as(_fp)) == ESTATE
            ctx.depth_store(1)
            ctx.depth_upload(0, cam, start)
            P, _, centre = ctx.depth_slot_matrices(0)          # the centre as mvs_depth_slot_matrices derives it
            ctx.sweep_set_main(cam, frames[0])
            ctx.sweep_set_views(np.stack([cams[s] for s in sides]), frames[1:])
            ctx.propagate_init(_device(start).data_ptr(), mvs_amd.MVS_COST_ABSDIFF, 1, 2, slopes=True)
            assert lib.mvs_propagate_normals(h, None) == EINVAL
            bad = cam.copy()
            bad[1, 2] = np.nan
            assert lib.mvs_propagate_normals(h, bad.ctypes.data_as(_fp)) == EINVAL and ctx.propagate_normals_pointer() == 0, "a refused call makes nothing"
            seen = []
            for runs in (2, 1):
                ctx.propagate_run(runs, 0.04, 0.01, 2, 17)
                got = ctx.propagate_normals(cam)
                z, gx, gy, _ = ctx.propagate_fetch()
                _same_bits(got, nm.hypothesis_normals(z, gx, gy, P, centre), what)
                valid = (z > -1) & (z < 1)
                assert nm.usable(got[valid]).all() and not got[~valid].any() and valid.sum() > W * H // 2, what
                assert (gx[valid] != 0).any() and (gy[valid] != 0).any(), what
                seen.append(got)
            assert seen[0].tobytes() != seen[1].tobytes(), what + ": the map follows the state"
            assert ctx.propagate_normals_pointer() != 0 and lib.mvs_propagate_normals_fetch(h, None) == EINVAL


# ---- the crafted store ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _context(W, H):
    """fusion_cases.store(W, H) on the device with normals_cases' support planes -> (context, the kernels' matrices per slot)"""
    st, pl = fc.store(W, H), nc.planes(W, H)
    ctx = mvs_amd.Context(W, H)
    ctx.depth_store(fc.DEPTH_CAP)
    for s in range(fc.DEPTH_CAP):
        ctx.depth_upload(s, st["cams"][s], st["depths"][s], st["costs"][s])
        ctx.depth_support_upload(s, pl["support"][s])
    return ctx, {s: ctx.depth_slot_matrices(s) for s in range(fc.DEPTH_CAP)}


def _set_planes(ctx, normals):
    for s in range(fc.DEPTH_CAP):
        if s in normals:
            ctx.depth_normals_upload(s, normals[s])
        else:
            ctx.depth_normals_drop(s)


def _rows(ctx, ref, nbrs, kw, cos):
    return ctx.fuse_depth(ref, nbrs, min_normal_cos=cos, **kw)


@pytest.mark.parametrize("case", nc.CASES, ids=[c[0] for c in nc.CASES])
def test_fusion_case(case):
    """rows and counts equal the mirror's, the premise holds with the kernels' matrices, the identities hold against the mirror and against
    the device's own masked and plain calls, with a call over another reference in between"""
    name, (W, H), ref, nbrs, kinds, kw, _, _ = case
    ctx, mats = _context(W, H)
    exp = nc.check_premise(case, mats)
    cos = nc.min_cos_of(case, mats)
    _, _, _, normals = nc.case_inputs(case)
    _set_planes(ctx, normals)
    got = _rows(ctx, ref, nbrs, kw, cos)
    assert len(got) == int(exp["keep"].sum()), name
    _same_bits(got, exp["rows"], name)
    other = _rows(ctx, fc.WIDE if ref != fc.WIDE else fc.AXIS, [fc.TILTED], dict(min_consistent=0), -INF)   # another reference in between
    assert len(other) > 0
    off = _rows(ctx, ref, nbrs, kw, -INF)
    _same_bits(off, nc.expected(case, mats, min_normal_cos=nc.NO_TEST)["rows"], name + ", test off")
    again = _rows(ctx, ref, nbrs, kw, cos)
    assert again.tobytes() == got.tobytes(), name
    # the identities: planes of zeros, then no planes
    masked = ctx.fuse_depth(ref, nbrs, **kw)
    assert masked.tobytes() != got.tobytes(), name
    _set_planes(ctx, {s: np.zeros((H, W, 3), f32) for s in kinds})
    _rows(ctx, fc.AXIS if ref != fc.AXIS else fc.WIDE, [], dict(min_consistent=0), -INF)
    assert _rows(ctx, ref, nbrs, kw, 0.5).tobytes() == masked.tobytes(), name + ": planes of zeros"
    _set_planes(ctx, {})
    _rows(ctx, fc.AXIS if ref != fc.AXIS else fc.WIDE, [], dict(min_consistent=0), -INF)
    assert _rows(ctx, ref, nbrs, kw, -INF).tobytes() == masked.tobytes(), name + ": no planes"
    plain = dict(kw, min_support=0)
    assert _rows(ctx, ref, nbrs, plain, -INF).tobytes() == ctx.fuse_depth(ref, nbrs, **plain).tobytes(), name + ": mvs_fuse_depth's bytes"
    assert ctx.fuse_points_device() != 0


def test_store_planes_and_refusals():
    W, H = fc.SIZES[2]
    st, pl = fc.store(W, H), nc.planes(W, H)
    plane, other = pl["noisy_holey"][fc.ROLLED], pl["exact"][fc.TILTED]
    out = np.empty((H, W, 3), f32)
    p = out.ctypes.data_as(_fp)
    with mvs_amd.Context(W, H) as ctx:
        lib, h = ctx.lib, ctx.h
        assert lib.mvs_depth_normals_upload(h, 0, p) == EINVAL and b"mvs_depth_store first" in lib.mvs_last_error(h)
        ctx.depth_store(3)
        assert lib.mvs_depth_normals_upload(h, 0, p) == ESTATE and b"holds no depth map" in lib.mvs_last_error(h)
        ctx.depth_upload(0, st["cams"][fc.ROLLED], st["depths"][fc.ROLLED])
        ctx.depth_upload(1, st["cams"][fc.TILTED], st["depths"][fc.TILTED])
        assert lib.mvs_depth_normals_upload(h, 3, p) == EINVAL and lib.mvs_depth_normals_upload(h, -1, p) == EINVAL
        assert lib.mvs_depth_normals_upload(h, 0, None) == EINVAL and lib.mvs_depth_normals_upload_device(h, 0, None) == EINVAL
        assert lib.mvs_depth_normals_fetch(h, 0, p) == ESTATE and b"no normal plane" in lib.mvs_last_error(h)
        assert lib.mvs_depth_normals_fetch(h, 0, None) == EINVAL and lib.mvs_depth_normals_fetch(h, 7, p) == EINVAL
        assert lib.mvs_depth_normals_drop(h, 3) == EINVAL
        # round trips from the host and from the device; planes are per slot
        ctx.depth_normals_upload(0, plane)
        assert ctx.depth_normals_fetch(0).tobytes() == plane.tobytes() and lib.mvs_depth_normals_fetch(h, 1, p) == ESTATE
        dev = _device(other)
        ctx.depth_normals_upload_device(1, dev.data_ptr())
        assert ctx.depth_normals_fetch(1).tobytes() == other.tobytes() and ctx.depth_normals_fetch(0).tobytes() == plane.tobytes()
        # the drop and a depth upload clear the plane; the map stays
        ctx.depth_normals_drop(1)
        assert lib.mvs_depth_normals_fetch(h, 1, p) == ESTATE and ctx.depth_slot_pointer(1) != 0
        ctx.depth_upload(0, st["cams"][fc.ROLLED], st["depths"][fc.ROLLED])
        assert lib.mvs_depth_normals_fetch(h, 0, p) == ESTATE
        # the refusals of the fusion: min_normal_cos NaN or above 1, and those of mvs_fuse_depth_masked
        n, nb = C.c_int(0), np.array([1], np.int32)

        def fuse(cos, ref=0, min_consistent=1, min_support=0):
            return lib.mvs_fuse_depth_normals(h, ref, 1, nb.ctypes.data_as(C.POINTER(C.c_int32)), min_consistent, 1.0, 0.01, INF, min_support, cos, None, C.byref(n))

        assert fuse(float("nan")) == EINVAL and b"min_normal_cos" in lib.mvs_last_error(h)
        assert fuse(float(np.nextafter(f32(1.0), f32(2.0)))) == EINVAL and fuse(INF) == EINVAL
        assert fuse(1.0) == 0 and fuse(-INF) == 0 and fuse(-2.0) == 0
        assert fuse(0.5, ref=1) == EINVAL and fuse(0.5, min_consistent=2) == EINVAL and fuse(0.5, min_support=256) == EINVAL
        assert fuse(0.5, min_support=1) == ESTATE and b"no support plane" in lib.mvs_last_error(h)
        assert lib.mvs_fuse_depth_normals(h, 0, 1, nb.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1.0, 0.01, INF, 0, 0.5, None, None) == EINVAL
        assert lib.mvs_fuse_depth_normals(h, 2, 1, nb.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1.0, 0.01, INF, 0, 0.5, None, C.byref(n)) == ESTATE
        # re-sizing the store frees the planes with it
        ctx.depth_normals_upload(0, plane)
        ctx.depth_store(2)
        ctx.depth_upload(0, st["cams"][fc.ROLLED], st["depths"][fc.ROLLED])
        assert lib.mvs_depth_normals_fetch(h, 0, p) == ESTATE
        ctx.depth_normals_upload(0, plane)
        assert ctx.depth_normals_fetch(0).tobytes() == plane.tobytes()


def test_the_raycasts_normals_go_into_a_plane():
    """mvs_tsdf_raycast_normals_device is accepted unchanged, and the fusion over that plane equals the mirror on the fetched normals"""
    W, H = fc.SIZES[2]
    ctx, mats = _context(W, H)
    st = fc.store(W, H)
    origin, h = fc.cube(50)
    ctx.tsdf_volume(50, origin, h, 4 * h)
    ctx.tsdf_integrate([fc.AXIS, fc.TILTED, fc.ROLLED, fc.WIDE])
    _, normals = ctx.tsdf_raycast(st["cams"][fc.ROLLED])
    assert nm.usable(normals).mean() > 0.05 and not normals[~nm.usable(normals)].any()
    _set_planes(ctx, {})
    ctx.depth_normals_upload_device(fc.ROLLED, ctx.tsdf_raycast_pointers()[1])
    assert ctx.depth_normals_fetch(fc.ROLLED).tobytes() == normals.tobytes()
    ctx.depth_normals_upload(fc.TILTED, nc.planes(W, H)["exact"][fc.TILTED])
    nbrs, kw = [fc.TILTED, fc.WIDE], dict(min_consistent=1)
    got = ctx.fuse_depth(fc.ROLLED, nbrs, min_normal_cos=0.9, **kw)
    exp = nm.fuse_normals(dict(enumerate(st["depths"])), {}, {}, {fc.ROLLED: normals, fc.TILTED: nc.planes(W, H)["exact"][fc.TILTED]}, mats, fc.ROLLED, nbrs,
                          min_normal_cos=0.9, **kw)
    assert len(got) > 100
    _same_bits(got, exp["rows"], "ray-cast normals")
    _set_planes(ctx, {})


# ---- Python ------------------------------------------------------------------------------------------------------------------------------------
def test_two_stage_normals():
    """the plane of slot n + i is propagate_normals of frame i's final state, fuse_depth(min_normal_cos=) on the planes equals the mirror,
    and normals=False leaves the slots without planes"""
    from mvs_amd import synth
    W, H, D, n = 64, 32, 8, 3
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, 2)
    cams, imgs = [main_cam] + list(side_cams), [main_img] + list(sides)
    cost = dict(cost="zncc", radius=1, keep=2)
    propagate = dict(iterations=1, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=9, slopes=True)
    term = dict(weight=5.0, max_px=2.0)
    frame_slots = [4, 1, 3]
    side_slots = [[frame_slots[j] for j in range(n) if j != i] for i in range(n)]
    side_cams_of = [np.stack([cams[j] for j in range(n) if j != i]) for i in range(n)]
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.frame_store(5)
        for i in range(n):
            ctx.frame_upload(frame_slots[i], imgs[i])
        ctx.depth_store(2 * n)
        args = (ctx, frame_slots, np.stack(cams), side_slots, np.stack(side_cams_of), D)
        plain = mvs_amd.propagate_two_stage(*args, cost=cost, propagate=propagate, consistency=term)
        for s in range(2 * n):
            with pytest.raises(mvs_amd.MvsError, match="no normal plane"):
                ctx.depth_normals_fetch(s)
        got = mvs_amd.propagate_two_stage(*args, cost=cost, propagate=propagate, consistency=term, normals=True)
        assert got.tobytes() == plain.tobytes()
        planes = {n + i: ctx.depth_normals_fetch(n + i) for i in range(n)}
        for i in range(n):
            with pytest.raises(mvs_amd.MvsError, match="no normal plane"):
                ctx.depth_normals_fetch(i)
        # the stage still holds the last frame's state: its plane is propagate_normals of it, and rule N1 on the fetched maps
        last = ctx.propagate_normals(cams[n - 1])
        assert planes[2 * n - 1].tobytes() == last.tobytes() and nm.usable(last).mean() > 0.9
        mats = {s: ctx.depth_slot_matrices(s) for s in range(2 * n)}
        z, gx, gy, _ = ctx.propagate_fetch()
        _same_bits(last, nm.hypothesis_normals(z, gx, gy, mats[2 * n - 1][0], mats[2 * n - 1][2]), "the last frame's plane")
        for i in range(n):
            assert nm.usable(planes[n + i]).mean() > 0.9 and (i == n - 1 or planes[n + i].tobytes() != last.tobytes())
        depths = {n + i: got[i] for i in range(n)}
        ref, nbrs = n, [n + 1, n + 2]
        rows = ctx.fuse_depth(ref, nbrs, min_consistent=1, max_reproj_px=2.0, max_rel_depth=0.05, min_normal_cos=0.8)
        exp = nm.fuse_normals(depths, {}, {}, planes, mats, ref, nbrs, min_consistent=1, max_reproj_px=2.0, max_rel_depth=0.05, min_normal_cos=0.8)
        assert len(rows) > 50
        _same_bits(rows, exp["rows"], "fuse_depth over the two-stage planes")
        assert rows.tobytes() != ctx.fuse_depth(ref, nbrs, min_consistent=1, max_reproj_px=2.0, max_rel_depth=0.05).tobytes()
