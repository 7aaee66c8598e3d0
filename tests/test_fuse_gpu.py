"""mvs_fuse_depth on the GPU (csrc/fuse.hip) against its float32 restatement (tests/fuse_mirror.py): keep masks, counts and rows bit
for bit; the depth store's life cycle and error codes; and the sequence path sweep -> depth store -> fusion -> filter -> Poisson."""
import ctypes as C
import functools

import numpy as np
import pytest

import fuse_mirror as fm
import mvs_amd
from mvs_amd import synth

pytestmark = pytest.mark.gpu

RING = 0.15
# slots of the parity contexts: 0 = centre, 1..4 = ring of four, 5 = a camera facing away (q.w <= 0 everywhere), 6 = a neighbour that sees
# nothing (all 1.0), 7 = ring view 2 with NaN and 1.0 holes, 8..23 = a ring of sixteen (small size only)
FACING_AWAY, EMPTY, HOLEY = 5, 6, 7


def _ring(n, radius):
    return [(radius * np.cos(a), radius * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(n) / n]


@functools.lru_cache(maxsize=None)
def _scene(W, H, with16):
    sc = synth.Scene()
    centres = [(0.0, 0.0, 0.0)] + _ring(4, RING)
    cams = [synth.camera_at(c, W, H) for c in centres]
    depths = [sc.render(c, W, H, want_depth=True)[1] for c in centres]
    cams.append(synth.camera_at((0.0, 0.0, 0.0), W, H, rot=np.diag([-1.0, 1.0, -1.0])))   # looks along +z: the surface is behind it
    depths.append(depths[0].copy())
    cams.append(cams[1])
    depths.append(np.full((H, W), 1.0, np.float32))
    rng = np.random.Generator(np.random.PCG64(0xF05E + W))
    holey = depths[2].copy()
    holey[rng.random((H, W)) < 0.15] = np.nan
    holey[rng.random((H, W)) < 0.15] = 1.0
    cams.append(cams[2])
    depths.append(holey)
    if with16:
        for i, c in enumerate(_ring(16, 1.0)):
            c = (c[0] * (0.08 if i % 2 else 0.2), c[1] * (0.08 if i % 2 else 0.2), 0.0)
            cams.append(synth.camera_at(c, W, H))
            depths.append(sc.render(c, W, H, want_depth=True)[1])
    costs = [rng.random((H, W), dtype=np.float32) for _ in depths]
    return cams, depths, costs


@functools.lru_cache(maxsize=None)
def _context(W, H):
    cams, depths, costs = _scene(W, H, W < 400)
    ctx = mvs_amd.Context(W, H)
    ctx.depth_store(len(depths) + 8)
    for s in range(len(depths)):
        ctx.depth_upload(s, cams[s], depths[s], costs[s])
    return ctx


def _parity(ctx, ref, nbrs, **kw):
    _, depths, costs = _scene(ctx.W, ctx.H, ctx.W < 400)
    got = ctx.fuse_depth(ref, nbrs, **kw)
    mats = {s: ctx.depth_slot_matrices(s) for s in [ref] + list(nbrs)}
    exp = fm.fuse(dict(enumerate(depths)), dict(enumerate(costs)), mats, ref, list(nbrs), **kw)
    assert got.shape == exp["rows"].shape, "count %d, mirror %d (%s)" % (len(got), len(exp["rows"]), kw)
    bad = np.nonzero((got.view(np.uint32) != exp["rows"].view(np.uint32)).any(1))[0]
    assert len(bad) == 0, "%d of %d rows differ; first: %s vs %s" % (len(bad), len(got), got[bad[0]], exp["rows"][bad[0]])
    return got, exp


SIZES = [(322, 241), (640, 480), (1920, 1080)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("nbrs,min_consistent", [([], 0), ([1], 1), ([1, 2, 3, 4], 2)])
def test_fusion_matches_the_mirror(W, H, nbrs, min_consistent):
    ctx = _context(W, H)
    got, exp = _parity(ctx, 0, nbrs, min_consistent=min_consistent)
    assert len(got) > 0.8 * W * H


@pytest.mark.parametrize("W,H", SIZES[:2])
def test_fusion_matches_the_mirror_with_holes_cost_threshold_and_useless_neighbours(W, H):
    ctx = _context(W, H)
    nbrs = [1, HOLEY, FACING_AWAY, EMPTY, 3]
    _, exp = _parity(ctx, 0, nbrs, min_consistent=1, max_cost=0.6, max_reproj_px=0.75, max_rel_depth=0.004)
    _, exp2 = _parity(ctx, 0, nbrs, min_consistent=2)
    assert 0 < exp["keep"].sum() < exp2["keep"].sum()
    # the camera facing away and the empty map never vote: only 1, HOLEY and 3 can agree
    assert exp2["agree"].max() == 3
    _parity(ctx, HOLEY, [0, 1, 2], min_consistent=1)   # holes in the reference itself


def test_sixteen_neighbours():
    ctx = _context(322, 241)
    got, exp = _parity(ctx, 0, list(range(8, 24)), min_consistent=3, max_rel_depth=0.02)
    assert exp["agree"].max() == 16 and len(got) > 0


def test_device_upload_equals_host_upload_and_runs_repeat():
    import torch
    W, H = 640, 480
    ctx = _context(W, H)
    cams, depths, costs = _scene(W, H, False)
    dev = [(torch.as_tensor(depths[s], device="cuda"), torch.as_tensor(costs[s], device="cuda")) for s in range(5)]
    torch.cuda.synchronize()
    base = len(depths)
    for s in range(5):
        ctx.depth_upload_device(base + s, cams[s], dev[s][0].data_ptr(), dev[s][1].data_ptr())
    for kw in ({"min_consistent": 2}, {"min_consistent": 1, "max_cost": 0.5}):
        host = ctx.fuse_depth(0, [1, 2, 3, 4], **kw)
        viad = ctx.fuse_depth(base, [base + 1, base + 2, base + 3, base + 4], **kw)
        assert np.array_equal(host.view(np.uint32), viad.view(np.uint32))
    for s in range(5):
        assert all(np.array_equal(a, b) for a, b in zip(ctx.depth_slot_matrices(s), ctx.depth_slot_matrices(base + s)))
    # the rows stay on the device
    n = len(viad)
    rows_dev = torch.as_tensor(mvs_amd._DeviceArray(ctx.fuse_points_device(), (n, 7), "<f4"), device="cuda")
    assert np.array_equal(rows_dev.cpu().numpy().view(np.uint32), viad.view(np.uint32))


def test_two_runs_give_identical_rows_at_1080p():
    ctx = _context(1920, 1080)
    a = ctx.fuse_depth(0, [1, 2, 3, 4])
    b = ctx.fuse_depth(0, [1, 2, 3, 4])
    assert len(a) > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_slot_matrices_are_the_camera_its_inverse_and_centre():
    ctx = _context(322, 241)
    cams, _, _ = _scene(322, 241, True)
    for s in (0, 3, FACING_AWAY, 9):
        P, Pi, Cn = ctx.depth_slot_matrices(s)
        assert np.array_equal(P, cams[s])
        P64, Pi64, C64 = fm.slot_matrices(cams[s])
        assert np.allclose(Pi, Pi64, rtol=1e-6, atol=1e-7)
        assert np.allclose(Cn, C64, atol=1e-6) and Cn[3] == 1.0


def test_error_codes():
    EINVAL, ESTATE = -1, -3
    with mvs_amd.Context(64, 48) as ctx:
        lib, h = ctx.lib, ctx.h
        cam = np.ascontiguousarray(synth.camera_at((0, 0, 0), 64, 48))
        d = np.zeros((48, 64), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
        n = C.c_int(0)
        inf = float("inf")

        def fuse(ref, nb, mc=0, rp=1.0, rel=0.01, cost=inf, count=True):
            arr = np.ascontiguousarray(nb if len(nb) else [0], np.int32)
            return lib.mvs_fuse_depth(h, ref, len(nb), arr.ctypes.data_as(C.POINTER(C.c_int32)), mc, rp, rel, cost, None, C.byref(n) if count else None)

        assert lib.mvs_depth_store(h, 0) == EINVAL and lib.mvs_depth_store(h, 8192) == EINVAL
        assert lib.mvs_depth_upload(h, 0, fp(cam), fp(d), None) == EINVAL   # no store yet
        assert fuse(0, []) == EINVAL
        assert lib.mvs_fuse_points_device(h) is None
        assert lib.mvs_depth_store(h, 20) == 0
        assert lib.mvs_depth_upload(h, 20, fp(cam), fp(d), None) == EINVAL
        assert lib.mvs_depth_upload(h, -1, fp(cam), fp(d), None) == EINVAL
        assert lib.mvs_depth_upload(h, 0, fp(cam), None, None) == EINVAL
        assert lib.mvs_depth_upload(h, 0, fp(np.zeros((4, 4), np.float32)), fp(d), None) == EINVAL   # singular camera
        assert lib.mvs_depth_slot_matrices(h, 0, fp(np.zeros(36, np.float32))) == ESTATE
        assert lib.mvs_depth_slot_matrices(h, 20, fp(np.zeros(36, np.float32))) == EINVAL
        assert fuse(0, []) == ESTATE                                          # unfilled reference
        for s in range(18):
            assert lib.mvs_depth_upload(h, s, fp(cam), fp(d), fp(d) if s != 3 else None) == 0
        assert fuse(0, [1, 19]) == ESTATE                                     # unfilled neighbour
        assert fuse(-1, [1]) == EINVAL and fuse(20, [1]) == EINVAL and fuse(0, [20]) == EINVAL
        assert fuse(0, list(range(1, 18))) == EINVAL                          # 17 neighbours
        assert fuse(0, [1, 0]) == EINVAL                                      # the reference as its own neighbour
        assert fuse(0, [1, 2], mc=3) == EINVAL and fuse(0, [1], mc=-1) == EINVAL
        assert fuse(0, [1], rp=-1.0) == EINVAL and fuse(0, [1], rel=-0.5) == EINVAL and fuse(0, [1], cost=-1.0) == EINVAL
        assert fuse(0, [1], rel=float("nan")) == EINVAL
        assert fuse(0, [1], count=False) == EINVAL
        assert fuse(0, [1, 3], cost=0.5) == ESTATE                            # slot 3 has no cost map
        assert fuse(0, [1, 3]) == 0 and n.value == 64 * 48                    # ... which an infinite max_cost never reads (one flat map: all kept)
        assert fuse(0, list(range(1, 17)), mc=16) == 0
        assert lib.mvs_fuse_points_device(h) is not None
        # re-sizing empties the store
        assert lib.mvs_depth_store(h, 2) == 0 and fuse(0, [1]) == ESTATE


def test_sequence_sweep_to_fused_points_to_mesh():
    """Five ring cameras at 640 x 480 (synth.Scene frames) go into the frame store; each is swept against the other four (128 planes over
    the scene's NDC range) and stored device to device; the centre is fused against the other four with min_consistent = 2.
    Measured on an MI355X (the sweep and the fusion are deterministic): 300770 of 307200 pixels kept; median distance to the height field
    0.00259 fused against 0.00395 for the unfused back-projection (K = 0); points off by more than three plane steps (0.0089 in linear
    depth) 0.53 % against 1.43 %, a factor 2.7.  Median normal error 42.7 degrees, fused and unfused alike: the normal comes from the
    reference map's 4-neighbours, and a swept map is piecewise constant -- one plane step is two pixel spacings, so
    every normal is either the plane's or a terrace edge's.  The 10-degree bound holds on exact maps (tests/test_fuse_cpu.py: under 1
    degree); here the assert keeps what was measured and that the normals face the camera, which Poisson needs."""
    W, H, D = 640, 480, 128
    sc = synth.Scene(freq_scale=W / 1920.0)
    centres = [(0.0, 0.0, 0.0)] + _ring(4, RING)
    cams = [synth.camera_at(c, W, H) for c in centres]
    frames = [sc.render(c, W, H) for c in centres]
    P = cams[0].astype(np.float64)
    A, B = -P[2, 2], P[2, 3]
    ndc = lambda w: (A * w + B) / w   # noqa: E731  (axis-parallel cameras: z_cam = -w)
    z_lo, z_hi = ndc(2.45), ndc(3.55)
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
        unfused = ctx.fuse_depth(0, [], min_consistent=0)
        step_w = (z_hi - z_lo) / D * 3.0 ** 2 / abs(B)   # one plane step in linear depth at w = 3

        def stats(r):
            p = r.astype(np.float64)
            err = np.abs(p[:, 2] - synth.Scene.height(p[:, 0], p[:, 1]))
            dhx = -0.52 * np.cos(1.3 * p[:, 0] + 0.7) * np.cos(1.1 * p[:, 1] - 0.2)
            dhy = 0.44 * np.sin(1.3 * p[:, 0] + 0.7) * np.sin(1.1 * p[:, 1] - 0.2)
            nr = np.stack([-dhx, -dhy, np.ones_like(dhx)], 1)
            nr /= np.linalg.norm(nr, axis=1, keepdims=True)
            ang = np.degrees(np.arccos(np.clip((p[:, 4:7] * nr).sum(1), -1, 1)))
            return np.median(err), (err > 3 * step_w).mean(), np.median(ang)

        mf, bf, af = stats(fused)
        mu, bu, au = stats(unfused)
        print("fused %d points: median error %.5f, > 3 steps %.4f, median normal error %.2f deg; unfused %d: %.5f, %.4f, %.2f deg; step %.5f"
              % (len(fused), mf, bf, af, len(unfused), mu, bu, au, step_w))
        assert len(fused) > 0.9 * W * H
        assert mf < mu
        assert bf * 2.0 <= bu
        assert af <= 45.0
        cam_dir = -fused[:, :3].astype(np.float64)   # toward the centre camera at the origin
        facing = (fused[:, 4:7].astype(np.float64) * cam_dir).sum(1)
        assert np.all(facing > -1e-6 * np.linalg.norm(cam_dir, axis=1))   # (the kernel decides the sign in f32)
        xyz = fused[:, :3]
        keep = ctx.filter_points(fused[:, :4], 0.01 * float(np.ptp(xyz, axis=0).max()))
        assert len(keep) > 0.5 * len(fused)
        v, f = mvs_amd.poisson_surface(fused[keep, :4], fused[keep, 4:7])
    assert len(v) > 100 and len(f) > 100
    vd = np.abs(v[:, 2].astype(np.float64) - synth.Scene.height(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)))
    print("mesh: %d vertices, %d faces, median distance to the height field %.5f" % (len(v), len(f), np.median(vd)))
    assert np.median(vd) < 5 * step_w
