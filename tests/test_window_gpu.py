"""mvs_sweep_window on the device (csrc/window.hip), bit-identical to the numpy mirror (tests/window_mirror.py)
throughout: Wv on the crafted volumes of tests/window_volumes.py at every frame, plane count, radius and tolerance that takes the kernel
down another path; the fused selection against the two-step form and against the oracle on the mirror's Wv; the readers behind
mvs_sweep_set_volume_source; behind a real sweep; on recycled memory; and every error of the list.  Volumes go in through
mvs_sweep_use_volume + mvs_sweep_set_planes, as in tests/test_aggregate_edges_gpu.py."""
import numpy as np
import pytest
import torch

import clean_mirror as cm
import mvs_amd
import sgm_mirror as sgm
import window_mirror as wm
import window_volumes as wv
from mvs_amd import synth
from test_aggregate_edges_gpu import _untouched, inject

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
CAM = np.eye(4, dtype=np.float32)


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _same_cells(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.uint32
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "%s: %d of %d cells differ; first at (d, y, x) = %s: 0x%08x, mirror 0x%08x" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def _same_maps(got, ref, what):
    for g, r, name in zip(got, ref, ("depth", "cost", "index")):
        np.testing.assert_array_equal(g, r, err_msg="%s: %s" % (what, name))


def _oracle_maps(oracle, Wv, z, sampler, refine):
    depth, cost, index = oracle.argmin(Wv, z, sampler=sampler)
    if refine:
        depth = oracle.refine_depth(Wv, z, index, sampler=sampler)
    return depth, cost, index


def _all_ways(ctx, oracle, vol, sampler, z, radius, tau, guide, guide_ptr, what):
    """one (volume, radius, tau): Wv against the mirror; the maps of the fused pass, of mvs_sweep_argmin + mvs_sweep_refine_depth under
    source WINDOWED, and of the oracle on the mirror's Wv, with and without the refinement"""
    ref = wm.window(vol, wv.CS[sampler], radius, tau, guide)
    for refine in (True, False):
        ctx.sweep_window(radius, tau, guide_ptr, select=True, refine=refine)
        fused = ctx.sweep_fetch()[:3]
        _same_cells(ctx.sweep_window_fetch(), ref, what)
        _same_maps(fused, _oracle_maps(oracle, ref, z, sampler, refine), what + " fused, refine %s" % refine)
    ctx.set_volume_source("windowed")
    try:
        ctx.sweep_argmin()
        _same_maps(ctx.sweep_fetch()[:3], fused, what + " two steps")
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], _oracle_maps(oracle, ref, z, sampler, True), what + " two steps, refined")
    finally:
        ctx.set_volume_source("raw")
    return ref


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("W,H", wv.FRAMES)
def test_crafted_volumes(oracle, W, H, sampler):
    cs = wv.CS[sampler]
    guide, staged = wv.guide_levels(W, H), wv.guide_levels(W, H, seed=1)
    gt = _device(guide)
    with mvs_amd.Context(W, H, 0, sampler=sampler) as ctx:
        ctx.sweep_set_main(CAM, staged)
        k = 0
        for D in wv.PLANES:
            vol = wv.noise(W, H, D, cs)
            t = inject(ctx, vol, D)
            z = oracle.plane_table(D, -1.0, 1.0)
            for radius in wv.RADII:
                for tau in wv.TAUS:
                    k += 1
                    by_pointer = k % 2 == 0     # the guide as a device pointer, or NULL and the staged main image
                    _all_ways(ctx, oracle, vol, sampler, z, radius, tau, guide if by_pointer else staged, gt.data_ptr() if by_pointer else None,
                              "%dx%dx%d r %d tau %d %s" % (W, H, D, radius, tau, sampler))
            assert _untouched(t, vol), "the window wrote into the volume"
            assert ctx.sweep_windowed_device()[1] == D * H * W * 4
            del t


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_extremes_and_radius_3(oracle, sampler):
    W, H, D, cs = 65, 9, 2, wv.CS[sampler]
    guide = wv.guide_checkerboard(W, H)
    gt = _device(guide)
    z = oracle.plane_table(D, -1.0, 1.0)
    with mvs_amd.Context(W, H, 0, sampler=sampler) as ctx:
        for vol in (wv.full(W, H, D, cs), wv.constant(W, H, D, cs)):
            t = inject(ctx, vol, D)
            for radius, tau in ((4, 255), (4, 0), (1, 255), (3, 255), (3, 20)):
                ref = _all_ways(ctx, oracle, vol, sampler, z, radius, tau, guide, gt.data_ptr(), "extreme r %d tau %d" % (radius, tau))
                _same_cells(ref, vol, "the mean of equal cells is the cell")
            assert (ctx.sweep_fetch()[2] == 0).all()     # every plane ties
            del t
        vol = wv.noise(W, H, 5, cs, seed=3)
        t = inject(ctx, vol, 5)
        z5 = oracle.plane_table(5, -1.0, 1.0)
        for tau in (255, 20, 0):
            _all_ways(ctx, oracle, vol, sampler, z5, 3, tau, guide, gt.data_ptr(), "noise r 3 tau %d" % tau)
        del t


def test_step_case(oracle):
    vol, guide, truth, near = wv.step_case()
    D, H, W = vol.shape
    gt = _device(guide)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        t = inject(ctx, vol, D)
        z = oracle.plane_table(D, -1.0, 1.0)
        _all_ways(ctx, oracle, vol, "fixed", z, 2, 255, guide, gt.data_ptr(), "step box")
        _all_ways(ctx, oracle, vol, "fixed", z, 2, 20, guide, gt.data_ptr(), "step gated")
        ctx.sweep_window(2, 20, gt.data_ptr(), select=True)
        bad = ctx.sweep_fetch()[2] != truth
        assert bad[near].mean() < 0.05 and bad[~near].mean() <= 0.01
        del t


def _readers(ctx, clean):
    """what the four readers leave: argmin + refine maps, S and the aggregation's maps, the cleaned maps with report and sizes"""
    ctx.sweep_argmin()
    ctx.sweep_refine_depth()
    wta = ctx.sweep_fetch()[:3]
    ctx.sweep_clean(**clean)
    cleaned = ctx.sweep_fetch()[:3] + (ctx.sweep_clean_report(), ctx.sweep_clean_sizes())
    ctx.sweep_aggregate(8, 16, 128, 4080, refine=True)
    return wta, cleaned, ctx.sweep_aggregate_fetch(), ctx.sweep_fetch()[:3]


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_readers_under_source_windowed(oracle, sampler):
    W, H, D, cs = 130, 19, 33, wv.CS[sampler]
    vol, guide = wv.noise(W, H, D, cs, seed=5), wv.guide_levels(W, H)
    gt = _device(guide)
    z = oracle.plane_table(D, -1.0, 1.0)
    clean = dict(min_views=2, uniqueness=10, speckle_min_size=6, speckle_max_diff=1)
    with mvs_amd.Context(W, H, 0, sampler=sampler) as ctx:
        assert ctx.volume_source() == mvs_amd.MVS_VOLUME_RAW
        t = inject(ctx, vol, D)
        before = _readers(ctx, clean)
        ctx.sweep_window(2, 20, gt.data_ptr(), select=False)
        _same_maps(ctx.sweep_fetch()[:3], before[3], "a window without MVS_WINDOW_SELECT leaves the maps alone")
        ref = wm.window(vol, cs, 2, 20, guide)
        ctx.set_volume_source("windowed")
        assert ctx.volume_source() == mvs_amd.MVS_VOLUME_WINDOWED
        wta, cleaned, S, agg = _readers(ctx, clean)
        _same_maps(wta, _oracle_maps(oracle, ref, z, sampler, True), "argmin + refine on Wv")
        d_ref, c_ref, i_ref, report, sizes = cm.clean(*wta, vol=ref, cs=cs, **clean)
        _same_maps(cleaned[:3], (d_ref, c_ref, i_ref), "clean on Wv")
        assert cleaned[3] == report and report[1] > 0 and report[2] > 0 and report[3] > 0, report
        np.testing.assert_array_equal(cleaned[4], sizes)
        seen = sgm.seen_cells(ref, cs)
        S_ref = sgm.aggregate(sgm.cost16(ref, cs, 4080), 8, 16, 128)
        np.testing.assert_array_equal(S, S_ref)
        _, c_ref, i_ref = sgm.select(S_ref, seen, z, 8)
        _same_maps(agg, (sgm.refine(S_ref, seen, z, i_ref), c_ref, i_ref), "aggregate on Wv")
        assert (S != before[2]).any() and (wta[2] != before[0][2]).any()
        # the raw volume is what it was, and so is everything that keeps meaning it
        assert _untouched(t, vol)
        np.testing.assert_array_equal(ctx.sweep_fetch(want_volume=True)[3], vol)
        assert ctx.sweep_volume_device()[0] == t.data_ptr()
        _same_cells(ctx.sweep_window_fetch(), ref, "Wv after its readers")
        # a sweep-side call keeps the source; only the setter changes it
        ctx.sweep_set_planes(D)
        assert ctx.volume_source() == mvs_amd.MVS_VOLUME_WINDOWED
        ctx.set_volume_source("raw")
        again = _readers(ctx, clean)
        _same_maps(again[0], before[0], "raw again: argmin + refine")
        _same_maps(again[1][:3], before[1][:3], "raw again: clean")
        assert again[1][3] == before[1][3]
        np.testing.assert_array_equal(again[2], before[2])
        _same_maps(again[3], before[3], "raw again: aggregate")
        del t


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_behind_a_real_sweep(oracle, sampler):
    W, H, V, D = 130, 19, 3, 17
    main_cam, main_img, side_cams, sides = synth.make_views(W, H, V, radius=0.3)[:4]
    vol = oracle.sweep(main_cam, main_img, side_cams, sides, D, want_volume=True, sampler=sampler)[3]
    assert 0.0 < sgm.seen_cells(vol, wv.CS[sampler]).mean()
    z = oracle.plane_table(D, -1.0, 1.0)
    with mvs_amd.Context(W, H, 0, sampler=sampler) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, mvs_amd.MVS_SWEEP_VOLUME)
        ctx.sweep_window(2, 20, None, select=True, refine=True)      # right behind the sweep, on its stream; the staged main image gates
        ref = wm.window(vol, wv.CS[sampler], 2, 20, main_img)
        _same_cells(ctx.sweep_window_fetch(), ref, "behind a sweep")
        _same_maps(ctx.sweep_fetch()[:3], _oracle_maps(oracle, ref, z, sampler, True), "behind a sweep")
        ctx.sweep_window(4, 255)
        _same_cells(ctx.sweep_window_fetch(), wm.window(vol, wv.CS[sampler], 4), "behind a sweep, box")


def test_every_cell_is_written(oracle, monkeypatch):
    """nobody zeroes Wv: on memory a larger, destroyed context has used, on a poisoned fresh allocation, and over an earlier window of
    another radius on the same context, every cell must be this call's"""
    big = wv.noise(200, 40, 9, 24, seed=9)
    with mvs_amd.Context(200, 40, 0, sampler="fixed") as ctx:
        t = inject(ctx, big, 9)
        ctx.sweep_window(4, 255)
        _same_cells(ctx.sweep_window_fetch(), wm.window(big, 24, 4), "the larger context")
        del t
    W, H, D = 130, 19, 5
    vol, guide = wv.noise(W, H, D, 24, seed=2), wv.guide_levels(W, H)
    gt = _device(guide)
    for poison in (False, True):
        if poison:
            monkeypatch.setenv("MVS_POISON_ALLOC", "1")
        with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
            t = inject(ctx, vol, D)
            ctx.sweep_window(1, 20, gt.data_ptr(), select=False)
            _same_cells(ctx.sweep_window_fetch(), wm.window(vol, 24, 1, 20, guide), "first window, poison %s" % poison)
            ctx.sweep_window(4, 255, None, select=False)
            _same_cells(ctx.sweep_window_fetch(), wm.window(vol, 24, 4), "second window, another radius")
            ctx.sweep_window(0, 0, None, select=False)
            _same_cells(ctx.sweep_window_fetch(), wm.window(vol, 24, 0), "third window, radius 0")
            # fewer planes of the same volume, then more again: Wv follows the plane count
            ctx.sweep_set_planes(2)
            ctx.sweep_window(2, 255)
            _same_cells(ctx.sweep_window_fetch(), wm.window(vol[:2], 24, 2), "two planes")
            del t


def test_errors(oracle):
    W, H, D = 65, 9, 5
    vol, guide = wv.noise(W, H, D, 24), wv.guide_levels(W, H)
    gt = _device(guide)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h
        buf = np.zeros((D, H, W), np.uint32)
        ptr = buf.ctypes.data_as(mvs_amd._u32p)
        # nothing set yet
        assert lib.mvs_sweep_window(h, 2, 255, None, 0) == ESTATE and b"planes" in lib.mvs_last_error(h)
        assert lib.mvs_sweep_window_fetch(h, ptr) == ESTATE
        assert not lib.mvs_sweep_windowed_device(h, None)
        ctx.sweep_set_planes(D)
        assert lib.mvs_sweep_window(h, 2, 255, None, 0) == ESTATE and b"volume" in lib.mvs_last_error(h)
        t = inject(ctx, vol, D)
        short = t.reshape(-1)[:D * H * W - 1]
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert lib.mvs_sweep_window(h, 2, 255, None, 0) == ESTATE
        ctx.sweep_use_volume(t.data_ptr(), t.numel() * 4)
        # a gate without a guide: no pointer and no staged main image; the box and radius 0 need none
        assert lib.mvs_sweep_window(h, 2, 254, None, 0) == ESTATE and b"guide" in lib.mvs_last_error(h)
        assert lib.mvs_sweep_window_fetch(h, ptr) == ESTATE
        ctx.sweep_window(0, 0, None, select=False)
        ctx.sweep_window(2, 20, gt.data_ptr(), select=True, refine=True)
        maps, cells = ctx.sweep_fetch()[:3], ctx.sweep_window_fetch()
        _same_cells(cells, wm.window(vol, 24, 2, 20, guide), "before the errors")

        def unchanged(what):
            _same_maps(ctx.sweep_fetch()[:3], maps, what)
            _same_cells(ctx.sweep_window_fetch(), cells, what)

        for args in ((-1, 255, 1), (5, 255, 1), (2, -1, 1), (2, 256, 1), (2, 255, 4), (2, 255, 0x80000001), (2, 255, mvs_amd.MVS_WINDOW_REFINE)):
            assert lib.mvs_sweep_window(h, args[0], args[1], gt.data_ptr(), args[2]) == EINVAL, args
            unchanged("after EINVAL %s" % (args,))
        assert lib.mvs_sweep_window(h, 2, 254, None, 1) == ESTATE
        unchanged("after the missing guide")
        assert lib.mvs_sweep_window_fetch(h, None) == EINVAL
        assert lib.mvs_sweep_set_volume_source(h, 2) == EINVAL and lib.mvs_sweep_set_volume_source(h, -1) == EINVAL
        assert ctx.volume_source() == mvs_amd.MVS_VOLUME_RAW
        # the readers under WINDOWED with a Wv of another plane count
        ctx.sweep_set_planes(D - 1)
        ctx.sweep_argmin()
        ctx.sweep_refine_depth()
        maps = ctx.sweep_fetch()[:3]
        ctx.set_volume_source("windowed")
        for call in (lambda: lib.mvs_sweep_argmin(h), lambda: lib.mvs_sweep_refine_depth(h), lambda: lib.mvs_sweep_aggregate(h, 8, 16, 128, 4080, 0),
                     lambda: lib.mvs_sweep_clean(h, 2, 10, 4, 1, 0)):
            assert call() == ESTATE and b"WINDOWED" in lib.mvs_last_error(h)
            _same_maps(ctx.sweep_fetch()[:3], maps, "after a refused reader")
        assert ctx.sweep_window_fetch().shape == (D, H, W)
        # the next valid calls succeed
        ctx.sweep_window(1, 255, None, select=False)
        _same_cells(ctx.sweep_window_fetch(), wm.window(vol[:D - 1], 24, 1), "after the errors")
        ctx.sweep_argmin()
        _same_maps(ctx.sweep_fetch()[:3], _oracle_maps(oracle, wm.window(vol[:D - 1], 24, 1), oracle.plane_table(D - 1, -1.0, 1.0), "fixed", False), "argmin on the new Wv")
        ctx.set_volume_source("raw")
        assert _untouched(t, vol)
        del t
    # a fresh context under WINDOWED: no Wv at all
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        t = inject(ctx, vol, D)
        ctx.set_volume_source("windowed")
        assert ctx.lib.mvs_sweep_argmin(ctx.h) == ESTATE and ctx.lib.mvs_sweep_aggregate(ctx.h, 8, 16, 128, 4080, 0) == ESTATE
        assert not ctx.lib.mvs_sweep_windowed_device(ctx.h, None)      # and a reader that was refused has allocated none
        del t
