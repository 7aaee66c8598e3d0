"""mvs_sweep_aggregate on the GPU (csrc/aggregate.hip) against the numpy mirror of DESIGN.md section 13 (tests/sgm_mirror.py): the path
sums S and the depth / cost / index maps bit for bit, the mirror running on the packed volume the GPU itself fetched.  Every case asserts
its own premises, so that a degenerate input cannot pass silently."""
import functools

import numpy as np
import pytest

import mvs_amd
import sgm_mirror as sgm
from mvs_amd import synth

pytestmark = pytest.mark.gpu

CS = {"fixed": 24, "exact": 16}


def _swept(views, D, sampler):
    """a context holding the packed volume of `views` = (main_cam, main_img, side_cams, side_imgs) -> (ctx, volume [D, H, W])"""
    main_cam, main_img, side_cams, sides = views[:4]
    H, W = main_img.shape
    ctx = mvs_amd.Context(W, H, 0, sampler=sampler)
    ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
    ctx.sweep_run(0, len(sides), mvs_amd.MVS_SWEEP_VOLUME)
    ctx.sweep_argmin()
    vol = ctx.sweep_fetch(want_volume=True)[3]
    return ctx, vol


@functools.lru_cache(maxsize=None)
def _mirror_sums(key, paths, p1, p2, cap):
    """the mirror's S for a cached volume: computed once per (volume, parameters), shared by the tests, never modified"""
    vol, cs = _VOLUMES[key]
    S = sgm.aggregate(sgm.cost16(vol, cs, cap), paths, p1, p2)
    S.setflags(write=False)
    return S


_VOLUMES = {}


def _compare(ctx, key, vol, sampler, z, paths, p1, p2, cap, refine=False):
    cs = CS[sampler]
    _VOLUMES.setdefault(key, (vol, cs))
    ctx.sweep_aggregate(paths, p1, p2, cap, refine=refine)
    S = ctx.sweep_aggregate_fetch()
    depth, cost, index, _ = ctx.sweep_fetch()
    S_ref = _mirror_sums(key, paths, p1, p2, cap)
    assert S.shape == S_ref.shape and S.dtype == np.uint16
    bad = np.argwhere(S != S_ref)
    assert len(bad) == 0, "%d of %d sums differ; first at (d, y, x) = %s: %d, mirror %d" % (len(bad), S.size, bad[0], S[tuple(bad[0])], S_ref[tuple(bad[0])])
    seen = sgm.seen_cells(vol, cs)
    d_ref, c_ref, i_ref = sgm.select(S_ref, seen, z, paths)
    np.testing.assert_array_equal(index, i_ref)
    np.testing.assert_array_equal(cost, c_ref)
    np.testing.assert_array_equal(depth, sgm.refine(S_ref, seen, z, i_ref) if refine else d_ref)
    return S, depth, cost, index


@functools.lru_cache(maxsize=None)
def _unseen_case():
    return _swept(synth.make_views(150, 70, 3, radius=0.8), 37, "fixed")


@pytest.mark.parametrize("paths,p1,p2,cap", [(8, 16, 128, 4080), (4, 16, 128, 4080), (8, 48, 4000, 320)])
def test_unseen_cells(oracle, paths, p1, p2, cap):
    """150 x 70 (W no multiple of 64), 37 planes, wide baseline: cells no view sees take part in the recurrence and are never selected"""
    ctx, vol = _unseen_case()
    seen = sgm.seen_cells(vol, 24)
    share = 1.0 - seen.mean()
    mixed = np.mean(seen.any(axis=0) & ~seen.all(axis=0))
    print("unseen cells %.3f of the volume, pixels with seen and unseen cells %.3f" % (share, mixed))
    assert 0.01 < share < 0.5 and mixed > 0.10
    _compare(ctx, "unseen", vol, "fixed", oracle.plane_table(37, -1.0, 1.0), paths, p1, p2, cap)


def test_exact_sampler(oracle):
    """cells count << 16 | sum: C = floor(16 s / n)"""
    ctx, vol = _swept(synth.make_views(150, 70, 3, radius=0.3), 37, "exact")
    assert (vol >> 16).max() >= 2 and ((vol & 0xffff) != 0).any()
    _, _, _, index = _compare(ctx, "exact", vol, "exact", oracle.plane_table(37, -1.0, 1.0), 8, 16, 128, 4080)
    assert len(np.unique(index)) > 3
    ctx.close()


@pytest.mark.parametrize("W,H,D", [(200, 66, 130), (70, 66, 2), (70, 66, 256)])
def test_adversarial_costs(oracle, W, H, D):
    """i.i.d. noise frames: no smooth surface for the penalties to follow, ties at the minimum go to the lowest plane; D just past 128
    (the plane split of the kernels changes there), the smallest and the largest D"""
    ctx, vol = _swept(synth.noise_views(W, H, 2), D, "fixed")
    S, _, _, index = _compare(ctx, "noise%d" % D, vol, "fixed", oracle.plane_table(D, -1.0, 1.0), 8, 16, 128, 4080)
    distinct = np.mean([len(np.unique(S[:, y, x])) for y in range(0, H, 5) for x in range(0, W, 7)])
    seen = sgm.seen_cells(vol, 24)
    masked = np.where(seen, S.astype(np.int64), 1 << 40)
    ties = int(np.sum(((masked == masked.min(axis=0)).sum(axis=0) > 1) & seen.any(axis=0)))
    print("D %d: %.1f distinct sums per pixel, %d pixels with a tie at the minimum" % (D, distinct, ties))
    assert distinct >= 2.0 and ties >= 1
    ctx.close()


def test_nothing_seen():
    """one side camera that faces away: every cell has count 0"""
    W, H, D, cap = 96, 40, 9, 300
    main_cam, main_img, _, _ = synth.noise_views(W, H, 1)
    away = synth.camera_at((0.0, 0.0, 0.0), W, H, rot=np.diag([-1.0, 1.0, -1.0]))
    ctx, vol = _swept((main_cam, main_img, away[None], [main_img]), D, "fixed")
    assert (vol >> 24).max() == 0
    for paths in (4, 8):
        ctx.sweep_aggregate(paths, 7, 90, cap)
        S = ctx.sweep_aggregate_fetch()
        depth, cost, index, _ = ctx.sweep_fetch()
        assert (S == paths * cap).all()
        assert (index == -1).all() and (depth == np.float32(1.0)).all() and np.isposinf(cost).all()
    ctx.close()


def test_refine_and_back_to_winner_take_all(oracle):
    ctx, vol = _unseen_case()
    z = oracle.plane_table(37, -1.0, 1.0)
    ctx.sweep_argmin()
    wta = [a.copy() for a in ctx.sweep_fetch()[:3]]
    _, d_plain, c_plain, i_plain = _compare(ctx, "unseen", vol, "fixed", z, 8, 16, 128, 4080)
    _, d_ref, c_ref, i_ref = _compare(ctx, "unseen", vol, "fixed", z, 8, 16, 128, 4080, refine=True)
    np.testing.assert_array_equal(i_ref, i_plain)
    np.testing.assert_array_equal(c_ref, c_plain)
    moved = np.mean(d_ref != d_plain)
    print("refinement moved %.3f of the depths" % moved)
    assert moved > 0.1 and np.abs(d_ref - d_plain).max() <= 0.5 * float(np.diff(z).max()) * 1.0001
    ctx.sweep_argmin()   # the volume is untouched: winner-take-all comes back exactly
    for a, b in zip(ctx.sweep_fetch()[:3], wta):
        np.testing.assert_array_equal(a, b)
    assert (wta[2] != i_plain).any(), "premise: aggregation changed the selection"


def test_determinism_and_plumbing():
    ctx, vol = _unseen_case()
    ctx.profile_enable(True)
    ctx.profile_read()
    ctx.sweep_aggregate()
    a = (ctx.sweep_aggregate_fetch(),) + ctx.sweep_fetch()[:3]
    ctx.sweep_aggregate()
    b = (ctx.sweep_aggregate_fetch(),) + ctx.sweep_fetch()[:3]
    _, launches = ctx.profile_read()
    ctx.profile_enable(False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert launches[mvs_amd.MVS_K_ARGMIN] > 0
    ptr, nbytes = ctx.sweep_aggregated_device()
    assert ptr and nbytes == 37 * 70 * 150 * 2
    # the aggregated maps feed the depth store and fusion like winner-take-all ones
    main_cam = synth.make_views(150, 70, 3, radius=0.8)[0]
    depth_ptr, cost_ptr, _ = ctx.sweep_result_pointers()
    ctx.depth_store(2)
    ctx.depth_upload_device(0, main_cam, depth_ptr, cost_ptr)
    ctx.depth_upload_device(1, main_cam, depth_ptr, cost_ptr)
    rows = ctx.fuse_depth(0, [1], min_consistent=1)
    print("fuse_depth on the aggregated maps: %d points of %d pixels" % (len(rows), 150 * 70))
    assert rows.ndim == 2 and rows.shape[1] == 7


def test_errors_leave_the_context_usable(oracle):
    ctx, vol = _unseen_case()
    lib = ctx.lib

    def code(*args):
        return lib.mvs_sweep_aggregate(ctx.h, *args)

    EINVAL, ESTATE = -1, -3
    assert lib.mvs_sweep_aggregate(None, 8, 16, 128, 4080, 0) == EINVAL
    for paths in (0, 2, 5, 16):
        assert code(paths, 16, 128, 4080, 0) == EINVAL
    assert code(8, -1, 128, 4080, 0) == EINVAL
    assert code(8, 16, 15, 4080, 0) == EINVAL
    assert code(8, 16, 128, 0, 0) == EINVAL and code(8, 16, 128, 4081, 0) == EINVAL
    assert code(8, 16, 4112, 4080, 0) == EINVAL and code(8, 16, 4111, 4080, 0) == 0     # 8 (4080 + 4111) = 65528
    assert code(4, 16, 12304, 4080, 0) == EINVAL and code(4, 16, 12303, 4080, 0) == 0   # 4 (4080 + 12303) = 65532
    assert code(8, 16, 128, 4080, 2) == EINVAL and code(8, 16, 128, 4080, 0x80000001) == EINVAL
    assert b"flag" in lib.mvs_last_error(ctx.h)
    with mvs_amd.Context(64, 48) as fresh:
        assert lib.mvs_sweep_aggregate(fresh.h, 8, 16, 128, 4080, 0) == ESTATE
        assert b"no cost volume" in lib.mvs_last_error(fresh.h)
        assert lib.mvs_sweep_aggregate_fetch(fresh.h, None) == ESTATE
        with pytest.raises(mvs_amd.MvsError):
            fresh.sweep_aggregate_fetch()
        with pytest.raises(mvs_amd.MvsError):
            fresh.sweep_aggregated_device()
        fresh.sweep_set_planes(16)
        assert lib.mvs_sweep_aggregate(fresh.h, 8, 16, 128, 4080, 0) == ESTATE   # planes, but no volume
    for D in (1, 257):
        ctx.sweep_set_planes(D)
        assert code(8, 16, 128, 4080, 0) == EINVAL
        assert b"planes outside" in lib.mvs_last_error(ctx.h)
    ctx.sweep_set_planes(37)
    # still usable: the same bytes as before the errors
    _compare(ctx, "unseen", vol, "fixed", oracle.plane_table(37, -1.0, 1.0), 8, 16, 128, 4080)
