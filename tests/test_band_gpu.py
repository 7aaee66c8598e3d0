"""mvs_sweep_run_band on the device (csrc/band.hip), bit-identical to the mirror (tests/band_mirror.py) throughout:
the crafted case through every combination of outputs, the identity with the ordinary sweep at a zero prior, view subsets, a prior that
is the context's own depth map, frames in the frame store, the readers behind the volume, the resolve step, every error of the list and
the coarse-to-fine helper."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_cases as bc
import band_mirror as bm
import mvs_amd
import sgm_mirror as sgm
import window_mirror as wm
from mvs_amd import synth

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
VOLUME, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOLUME | FUSED


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _same_cells(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.uint32
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "%s: %d of %d cells differ; first at (d, y, x) = %s: 0x%08x, expected 0x%08x" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def _same_maps(got, ref, what):
    for g, r, name in zip(got, ref, ("depth", "cost", "index")):
        np.testing.assert_array_equal(g, r, err_msg="%s: %s" % (what, name))


def _same_floats(got, ref, what):
    """equal as bits (the maps hold no NaN; the priors do)"""
    np.testing.assert_array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(ref, np.float32).view(np.uint32), err_msg=what)


def _crafted_context():
    c = bc.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set(*c.views(), c.D, -c.HB, c.HB)
    return c, ctx, _device(c.prior)


def test_crafted_case(oracle):
    c, ctx, prior = _crafted_context()
    ref = bc.crafted_volume()
    delta = bc.offsets(oracle, c.D, c.HB)
    maps = oracle.argmin(ref, delta, sampler="fixed")
    refined = (oracle.refine_depth(ref, delta, maps[2], sampler="fixed"),) + maps[1:]
    with ctx:
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "volume | fused")
        _same_maps(got[:3], maps, "volume | fused")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], maps[2]), "resolve")
        assert ctx.sweep_band_report() == bm.report(c.prior, maps[0], maps[2], c.D)
        prior_copy = torch.as_tensor(mvs_amd._DeviceArray(ctx.sweep_band_pointers()[1], (c.H, c.W), "<f4"), device="cuda").cpu().numpy()
        _same_floats(prior_copy, c.prior, "the context's copy of the prior")
        # the volume alone, then the two-step selection and the refinement
        ctx.sweep_run_band(prior.data_ptr(), 0, 1, BOTH)        # (other cells and maps in between)
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, VOLUME)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, "volume alone")
        ctx.sweep_argmin()
        _same_maps(ctx.sweep_fetch()[:3], maps, "volume, then mvs_sweep_argmin")
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], refined, "refined")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, refined[0], refined[2]), "resolve of the refined offsets")
        assert ctx.sweep_band_report() == bm.report(c.prior, refined[0], refined[2], c.D)
    # the selection alone, on a context that never had a volume
    c, ctx, prior = _crafted_context()
    with ctx:
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], maps, "fused alone")
        ctx.sweep_run_band(prior.data_ptr(), 0, 2, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], oracle.argmin(bc.crafted_volume((0, 1)), delta, sampler="fixed"), "fused alone, two views")


def _general_context(W, H, D, V, hb):
    views = bc.general_views(W, H, V)
    ctx = mvs_amd.Context(W, H, 0, sampler="fixed")
    ctx.sweep_set(*views[:4], D, -hb, hb)
    return views, ctx


def test_zero_prior_is_the_ordinary_sweep():
    W, H, D, V, hb = 130, 40, 33, 5, 0.3
    _, ctx = _general_context(W, H, D, V, hb)
    zero = _device(np.zeros((H, W), np.float32))
    with ctx:
        ctx.sweep_run(0, V, BOTH | mvs_amd.MVS_SWEEP_NO_RECT)
        assert ctx.plan_shape() == 3          # general cameras: the tiled general kernel
        ref = ctx.sweep_fetch(want_volume=True)
        assert (ref[3] >> 24).max() == V and (ref[2] >= 0).mean() > 0.9
        ctx.sweep_run_band(zero.data_ptr(), 0, V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref[3], "band at prior 0")
        _same_maps(got[:3], ref[:3], "band at prior 0")
        _same_floats(ctx.sweep_band_resolve(), ref[0], "0 + offset")


def test_view_subsets_add():
    W, H, D, V, hb = 130, 40, 33, 5, 0.2
    views, ctx = _general_context(W, H, D, V, hb)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    prior = _device((views[4] + 0.1 * np.sin(0.3 * x) * np.cos(0.2 * y)).astype(np.float32))
    with ctx:
        vols = []
        for first, count in ((0, 2), (2, 3), (0, 5)):
            ctx.sweep_run_band(prior.data_ptr(), first, count, VOLUME)
            vols.append(ctx.sweep_fetch(want_volume=True)[3])
        assert (vols[0] != 0).any() and (vols[1] != 0).any()
        _same_cells(vols[0] + vols[1], vols[2], "views [0, 2) + [2, 5)")


def test_prior_may_be_the_contexts_depth_map():
    W, H, V, hb = 130, 40, 5, 0.1875
    views, ctx = _general_context(W, H, 16, V, 1.0)
    with ctx:
        def coarse():
            ctx.sweep_set_planes(16, -1.0, 1.0)
            ctx.sweep_run(0, V, BOTH)
            ctx.sweep_refine_depth()
            ctx.sweep_set_planes(16, -hb, hb)
            return ctx.sweep_fetch()[0]

        separate = _device(coarse())
        ctx.sweep_run_band(separate.data_ptr(), 0, V, BOTH)
        ref = ctx.sweep_fetch(want_volume=True)
        ref_abs = ctx.sweep_band_resolve()
        assert len(np.unique(ref[2])) > 4
        _same_floats(coarse(), separate.cpu().numpy(), "the coarse map again")
        ctx.sweep_run_band(ctx.sweep_result_pointers()[0], 0, V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref[3], "aliased prior")
        _same_maps(got[:3], ref[:3], "aliased prior")
        _same_floats(ctx.sweep_band_resolve(), ref_abs, "aliased prior, resolved")


def test_frames_in_the_frame_store():
    c = bc.crafted()
    prior = _device(c.prior)
    ref = bc.crafted_volume()
    slots = [4, 0, 3, 1]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.frame_store(6)
        ctx.frame_upload(slots[0], c.main_img)
        for v in range(c.V):
            ctx.frame_upload(slots[1 + v], c.sides[v])
        ctx.sweep_handles(slots[0], c.main_cam, slots[1:], c.side_cams, 8)      # leaves the slots staged
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        stored = ctx.sweep_fetch(want_volume=True)
    c2, ctx, _ = _crafted_context()
    with ctx:
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        staged = ctx.sweep_fetch(want_volume=True)
    _same_cells(stored[3], staged[3], "frame store against set_main / set_views")
    _same_maps(stored[:3], staged[:3], "frame store against set_main / set_views")
    _same_cells(stored[3], ref, "frame store against the mirror")


def test_downstream_readers(oracle):
    c, ctx, prior = _crafted_context()
    vol = bc.crafted_volume()
    delta = bc.offsets(oracle, c.D, c.HB)
    seen = sgm.seen_cells(vol, 24)
    with ctx:
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        ctx.sweep_aggregate(8, 16, 128, 4080, refine=True)
        S = sgm.aggregate(sgm.cost16(vol, 24, 4080), 8, 16, 128)
        np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)
        _, cost, index = sgm.select(S, seen, delta, 8)
        maps = (sgm.refine(S, seen, delta, index), cost, index)
        _same_maps(ctx.sweep_fetch()[:3], maps, "aggregated")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], index), "resolve after the aggregation")
        assert ctx.sweep_band_report() == bm.report(c.prior, maps[0], index, c.D)
        ctx.sweep_window(2, 255, None, select=True)
        Wv = wm.window(vol, 24, 2)
        _same_cells(ctx.sweep_window_fetch(), Wv, "windowed")
        maps = oracle.argmin(Wv, delta, sampler="fixed")
        _same_maps(ctx.sweep_fetch()[:3], maps, "window select")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], maps[2]), "resolve after the window")
        assert ctx.sweep_band_report() == bm.report(c.prior, maps[0], maps[2], c.D)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, "the readers left the volume alone")


def test_resolve():
    c, ctx, prior = _crafted_context()
    with ctx:
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        ctx.sweep_refine_depth()
        maps = ctx.sweep_fetch()[:3]
        first = ctx.sweep_band_resolve()
        rep = ctx.sweep_band_report()
        _same_floats(ctx.sweep_band_resolve(), first, "idempotent")
        assert ctx.sweep_band_report() == rep and rep[3] == 0
        _same_maps(ctx.sweep_fetch()[:3], maps, "resolve leaves the maps")
        _same_floats(first, bm.resolve(c.prior, maps[0], maps[2]), "resolve")
        # offsets that carry a pixel out of (-1, 1), written through the device pointers: prior 0.995 + 0.25, prior -0.995 - 0.25, and a
        # pixel without a prior (1.0) that is given an index
        dptr, _, iptr = ctx.sweep_result_pointers()
        depth_t = torch.as_tensor(mvs_amd._DeviceArray(dptr, (c.H, c.W), "<f4"), device="cuda")
        index_t = torch.as_tensor(mvs_amd._DeviceArray(iptr, (c.H, c.W), "<i4"), device="cuda")
        for (r, col), off, ix in (((12, 20), 0.25, 17), ((3, 21), -0.25, 1), ((4, 8), 0.0, 9), ((1, 1), 0.125, 0)):
            depth_t[r, col] = off
            index_t[r, col] = ix
        torch.cuda.synchronize()
        crafted_maps = ctx.sweep_fetch()[:3]
        assert crafted_maps[0][12, 20] == np.float32(0.25) and crafted_maps[2][3, 21] == 1
        got = ctx.sweep_band_resolve()
        ref = bm.resolve(c.prior, crafted_maps[0], crafted_maps[2])
        _same_floats(got, ref, "crafted maps")
        assert got[12, 20] == 1.0 and got[3, 21] == 1.0 and got[4, 8] == 1.0 and got[1, 1] == np.float32(c.prior[1, 1]) + np.float32(0.125)
        rep2 = ctx.sweep_band_report()
        assert rep2 == bm.report(c.prior, crafted_maps[0], crafted_maps[2], c.D) and rep2[3] == 3
        _same_maps(ctx.sweep_fetch()[:3], crafted_maps, "resolve leaves the crafted maps")


def test_errors():
    c = bc.crafted()
    prior = _device(c.prior)
    p = C.c_void_p(prior.data_ptr())
    out_f = np.zeros((c.H, c.W), np.float32)
    fp, ip = out_f.ctypes.data_as(mvs_amd._fp), (C.c_int * 4)()
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h

        def later_calls(what):
            for fn in (lambda: lib.mvs_sweep_band_resolve(h), lambda: lib.mvs_sweep_band_fetch(h, fp), lambda: lib.mvs_sweep_band_report(h, ip)):
                assert fn() == ESTATE, what

        assert lib.mvs_sweep_run_band(None, 0, 0, p, BOTH) == EINVAL
        assert lib.mvs_sweep_band_resolve(None) == EINVAL and lib.mvs_sweep_band_fetch(None, fp) == EINVAL and lib.mvs_sweep_band_report(None, ip) == EINVAL
        assert not lib.mvs_sweep_band_depth_device(None) and not lib.mvs_sweep_band_prior_device(None)
        # nothing staged: no main view, no views, no planes
        assert lib.mvs_sweep_run_band(h, 0, 0, p, BOTH) == ESTATE
        later_calls("before anything")
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        assert lib.mvs_sweep_run_band(h, 0, 0, p, BOTH) == ESTATE
        ctx.sweep_set_main(c.main_cam, c.main_img)
        assert lib.mvs_sweep_run_band(h, 0, 0, p, BOTH) == ESTATE and b"views" in lib.mvs_last_error(h)
        ctx.sweep_set_views(c.side_cams, c.sides)
        later_calls("before a band run")
        assert not lib.mvs_sweep_band_depth_device(h) and not lib.mvs_sweep_band_prior_device(h)   # a context that never ran a band allocates nothing
        # an ordinary sweep is no band run
        ctx.sweep_run(0, c.V, BOTH)
        later_calls("after an ordinary sweep")
        ordinary = ctx.sweep_fetch(want_volume=True)

        def unchanged(ref, what):
            got = ctx.sweep_fetch(want_volume=True)
            _same_maps(got[:3], ref[:3], what)
            _same_cells(got[3], ref[3], what)

        for args in ((0, c.V, None, BOTH), (-1, 2, p, BOTH), (0, c.V + 1, p, BOTH), (2, 2, p, BOTH), (0, -1, p, BOTH), (0, c.V, p, 0),
                     (0, c.V, p, BOTH | mvs_amd.MVS_SWEEP_FORCE_GENERIC), (0, c.V, p, BOTH | mvs_amd.MVS_SWEEP_NO_RECT), (0, c.V, p, VOLUME | 0x100),
                     (0, c.V, p, 0x80000000 | FUSED)):
            assert lib.mvs_sweep_run_band(h, *args) == EINVAL, args
            unchanged(ordinary, "after EINVAL %s" % (args,))
        # a plane table that is not inside (-1, 1); the exact sampler
        ctx.sweep_set_planes(c.D, -1.0, 1.0)
        ctx.sweep_run(0, c.V, BOTH)
        ordinary = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_set_planes(c.D, -0.9, 1.06)      # the last offset is above 1
        assert lib.mvs_sweep_run_band(h, 0, c.V, p, BOTH) == ESTATE and b"(-1, 1)" in lib.mvs_last_error(h)
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        ctx.set_sampler("exact")
        assert lib.mvs_sweep_run_band(h, 0, c.V, p, BOTH) == ESTATE and b"FIXED" in lib.mvs_last_error(h)
        ctx.set_sampler("fixed")
        unchanged(ordinary, "after the refused band runs")
        later_calls("still no band run")
        # the first band run; fetch and report want the resolve
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, VOLUME)
        assert lib.mvs_sweep_band_prior_device(h) and not lib.mvs_sweep_band_depth_device(h)
        later_calls("a band volume without a selection: the index map is the ordinary sweep's")
        ctx.sweep_argmin()
        assert lib.mvs_sweep_band_fetch(h, fp) == ESTATE and lib.mvs_sweep_band_report(h, ip) == ESTATE
        good = ctx.sweep_band_resolve()
        assert lib.mvs_sweep_band_depth_device(h)
        assert lib.mvs_sweep_band_fetch(h, None) == EINVAL and lib.mvs_sweep_band_report(h, None) == EINVAL
        _same_floats(ctx.sweep_band_resolve(), good, "after the EINVALs")
        rep = ctx.sweep_band_report()
        # another plane count
        ctx.sweep_set_planes(c.D - 2, -c.HB, c.HB)
        later_calls("D changed since the band run")
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        _same_floats(ctx.sweep_band_resolve(), good, "back at the band's plane count")
        assert ctx.sweep_band_report() == rep
        # a later ordinary sweep takes the maps away from the band
        ctx.sweep_run(0, c.V, FUSED)
        later_calls("an ordinary sweep since")
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        assert lib.mvs_sweep_band_fetch(h, fp) == ESTATE     # this run is not resolved yet
        _same_floats(ctx.sweep_band_resolve(), good, "the context stays usable")
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], bc.crafted_volume(), "the context stays usable")


def test_coarse_to_fine_helper(oracle):
    W, H, V, DC, DB = 96, 64, 4, 16, 16
    main_cam, main_img, side_cams, sides, truth = synth.make_views(W, H, V)
    _, _, index, vol = oracle.sweep(main_cam, main_img, side_cams, sides, DC, want_volume=True, nthreads=4, sampler="fixed")
    coarse = oracle.refine_depth(vol, oracle.plane_table(DC, -1.0, 1.0), index, sampler="fixed")
    hb = float(np.float32(1.5 * 2.0 / DC))
    delta = bc.offsets(oracle, DB, hb)
    band = bm.band_volume(oracle, main_cam, main_img, side_cams, sides, coarse, delta)
    _, cost, index = oracle.argmin(band, delta, sampler="fixed")
    offset = oracle.refine_depth(band, delta, index, sampler="fixed")
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, 1)
        got = mvs_amd.coarse_to_fine(ctx, DC, DB)
        _same_floats(got, bm.resolve(coarse, offset, index), "coarse_to_fine")
        maps = ctx.sweep_fetch(want_volume=True)
        _same_cells(maps[3], band, "coarse_to_fine: the band's volume")
        _same_maps(maps[:3], (offset, cost, index), "coarse_to_fine: the band's maps")
        assert ctx.sweep_band_report() == bm.report(coarse, offset, index, DB)
    assert np.median(np.abs(got - truth)) < np.median(np.abs(coarse - truth))
