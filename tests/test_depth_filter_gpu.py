"""mvs_depth_filter on the device (csrc/depth_filter.hip), bit-identical to the mirror (tests/depth_filter_mirror.py)
throughout: the crafted maps (every flag combination at every radius, maps at the kernel's own edges, every kind of value, the gates at
their thresholds, the fill rule at min_members), the guide taken from the staged main image, the context's own maps as input, the
previous output as input, the state it must leave alone, every error of the list and the coarse-to-fine helper's `filter` keyword."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_cases as bc
import band_mirror as bm
import depth_filter_cases as dc
import depth_filter_mirror as dm
import mvs_amd
from mvs_amd import synth

pytestmark = pytest.mark.gpu

f32 = np.float32
EINVAL, ESTATE = -1, -3
MEDIAN, MEAN, FILL = mvs_amd.MVS_FILTER_MEDIAN, mvs_amd.MVS_FILTER_MEAN, mvs_amd.MVS_FILTER_FILL
BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
TILE = (32, 8)        # csrc/depth_filter.hip: DF_TW, DF_TH
INF = float("inf")


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32 and ref.dtype == np.float32, what
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, "%s: %d of %d pixels differ; first at (row, col) = %s: %r (0x%08x), expected %r (0x%08x)" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], got.view(np.uint32)[tuple(bad[0])], ref[tuple(bad[0])], ref.view(np.uint32)[tuple(bad[0])])


def _filter(ctx, ptr, case, guide_ptr=None, **kw):
    return ctx.depth_filter(ptr, radius=case.radius, tau=case.tau, max_step=float(case.max_step), guide_ptr=guide_ptr, median=bool(case.flags & MEDIAN),
                            mean=bool(case.flags & MEAN), fill=case.min_members if case.flags & FILL else 0, **kw)


def test_the_modules_state_the_kernels_tile():
    assert dc.TILE == TILE and (dm.MEDIAN, dm.MEAN, dm.FILL) == (MEDIAN, MEAN, FILL)
    sizes = {c.depth.shape[::-1] for c in dc.cases()}
    assert {(9, 5), TILE, (TILE[0] + 1, TILE[1]), (TILE[0] - 1, TILE[1]), (TILE[0], TILE[1] + 1), (TILE[0], TILE[1] - 1), (2 * TILE[0], 2 * TILE[1])} <= sizes


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c.name)
def test_crafted_map(case):
    """nothing is staged on the context: the guide is the caller's (tau = 255 with a NULL guide among the cases)"""
    H, W = case.depth.shape
    depth = _device(case.depth)
    guide = _device(case.guide) if case.guide is not None else None
    with mvs_amd.Context(W, H, 0) as ctx:
        assert ctx.depth_filtered_pointer() == 0
        got = _filter(ctx, depth.data_ptr(), case, guide.data_ptr() if guide is not None else None)
        _same(got, dc.reference(case), case.name)
        assert ctx.depth_filtered_pointer() != 0
    if case.flags & FILL:
        ok = dm.valid(case.depth)
        plain = dm.filter(case.depth, case.radius, case.tau, case.max_step, case.guide, case.flags & ~FILL)
        if not case.flags & MEAN:
            _same(got[ok], plain[ok], case.name + ": FILL never changes a valid pixel")


def test_guide_is_the_staged_main_image():
    case = dc.by_name("flags3_r3")
    H, W = case.depth.shape
    depth, other = _device(case.depth), _device(255 - case.guide)
    with mvs_amd.Context(W, H, 0) as ctx:
        ctx.sweep_set_main(synth.camera_at([0, 0, 0], W, H), case.guide)
        _same(_filter(ctx, depth.data_ptr(), case), dc.reference(case), "NULL guide: the staged main image")
        # a caller's guide takes precedence
        ref = dm.filter(case.depth, case.radius, case.tau, case.max_step, 255 - case.guide, case.flags)
        _same(_filter(ctx, depth.data_ptr(), case, other.data_ptr()), ref, "the caller's guide")


def test_previous_output_as_input_and_a_stable_address():
    """the filtered map of one call is the input of the next, twice in a row: with both stages (the median reads it, the mean writes it)
    and with one stage (which must not read the map it writes)"""
    case = dc.by_name("seams_both")
    H, W = case.depth.shape
    depth, guide = _device(case.depth), _device(case.guide)
    with mvs_amd.Context(W, H, 0) as ctx:
        ref = dc.reference(case)
        _same(_filter(ctx, depth.data_ptr(), case, guide.data_ptr()), ref, "first call")
        out = ctx.depth_filtered_pointer()
        for flags, name in ((MEDIAN | MEAN, "both stages"), (MEDIAN | MEAN, "both stages again"), (MEDIAN, "median alone"), (MEAN, "mean alone"), (MEAN, "mean alone again")):
            ref = dm.filter(ref, case.radius, case.tau, case.max_step, case.guide, flags)
            got = ctx.depth_filter(out, case.radius, case.tau, float(case.max_step), guide.data_ptr(), median=bool(flags & MEDIAN), mean=bool(flags & MEAN))
            _same(got, ref, "the previous output as input: " + name)
            assert ctx.depth_filtered_pointer() == out
        # fetch=False leaves the map on the device
        assert _filter(ctx, depth.data_ptr(), case, guide.data_ptr(), fetch=False) is None
        got = np.empty((H, W), np.float32)
        assert ctx.lib.mvs_depth_filter_fetch(ctx.h, got.ctypes.data_as(C.POINTER(C.c_float))) == 0
        _same(got, dc.reference(case), "fetch=False, then the fetch")


def test_the_contexts_own_maps_and_the_state_it_leaves_alone(oracle):
    """the input is the sweep's depth map, a band run's offset map and its resolved map; the sweep's maps, the selection and the band
    state are what they were: a later mvs_sweep_refine_depth / mvs_sweep_band_resolve gives what it gives without the filter"""
    W, H, V, D = 45, 23, 3, 12
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    z = oracle.plane_table(D, -1.0, 1.0)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH)
        before = ctx.sweep_fetch(want_volume=True)
        got = ctx.depth_filter(ctx.sweep_result_pointers()[0], 2, 30, float(f32(4 * 2.0 / D)))
        _same(got, dm.filter(before[0], 2, 30, f32(4 * 2.0 / D), main_img), "the sweep's depth map")
        after = ctx.sweep_fetch(want_volume=True)
        for a, b, name in zip(after, before, ("depth", "cost", "index", "volume")):
            np.testing.assert_array_equal(a, b, err_msg="the filter changed the sweep's " + name)
        assert ctx.volume_source() == mvs_amd.MVS_VOLUME_RAW
        ctx.sweep_refine_depth()
        coarse = ctx.sweep_fetch()[0]
        _same(coarse, oracle.refine_depth(before[3], z, before[2], sampler="fixed"), "mvs_sweep_refine_depth after the filter")
        # a band run on the filtered prior; its offset map and its resolved map as inputs
        prior = ctx.depth_filter(ctx.sweep_result_pointers()[0], 2, 255, INF, fill=3)
        hb = float(f32(1.5 * 2.0 / D))
        ctx.sweep_set_planes(8, -hb, hb)
        ctx.sweep_run_band(ctx.depth_filtered_pointer(), 0, V, BOTH)
        offset, _, index, _ = ctx.sweep_fetch()
        resolved = ctx.sweep_band_resolve()
        _same(resolved, bm.resolve(prior, offset, index), "the band run took the filtered map as its prior")
        report = ctx.sweep_band_report()
        _same(ctx.depth_filter(ctx.sweep_result_pointers()[0], 1, 255, float(f32(hb / 4)), median=False), dm.filter(offset, 1, 255, f32(hb / 4), None, MEAN), "the offset map")
        _same(ctx.depth_filter(ctx.sweep_band_pointers()[0], 3, 10, INF, mean=False), dm.filter(resolved, 3, 10, INF, main_img, MEDIAN), "the resolved map")
        _same(ctx.sweep_band_resolve(), resolved, "mvs_sweep_band_resolve after the filter")
        assert ctx.sweep_band_report() == report
        _same(ctx.sweep_fetch()[0], offset, "the band's offset map after the filter")


def test_a_context_that_never_filters_has_no_filtered_map():
    W, H, V, D = 45, 23, 2, 4
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH)
        ctx.sweep_window(1)
        assert ctx.depth_filtered_pointer() == 0 and ctx.lib.mvs_depth_filtered_device(None) is None
        assert ctx.lib.mvs_depth_filter_fetch(ctx.h, np.empty((H, W), np.float32).ctypes.data_as(C.POINTER(C.c_float))) == ESTATE


def test_errors():
    """every error of the list, each followed by a good call that gives the mirror's bytes: nothing was written, the context is usable"""
    case = dc.by_name("flags7_r2")
    H, W = case.depth.shape
    depth, guide = _device(case.depth), _device(case.guide)
    d, g = C.c_void_p(depth.data_ptr()), C.c_void_p(guide.data_ptr())
    with mvs_amd.Context(W, H, 0) as ctx:
        lib, h = ctx.lib, ctx.h
        call = lib.mvs_depth_filter
        out = np.empty((H, W), np.float32)
        fp = out.ctypes.data_as(C.POINTER(C.c_float))

        def good(what):
            _same(_filter(ctx, depth.data_ptr(), case, guide.data_ptr()), dc.reference(case), "after " + what)

        assert lib.mvs_depth_filter_fetch(h, fp) == ESTATE and b"no filtered map" in lib.mvs_last_error(h)      # before the first call
        assert call(h, d, None, 2, 12, 0.04, 3, MEDIAN | MEAN) == ESTATE and b"guide" in lib.mvs_last_error(h)  # tau < 255, nothing staged
        assert ctx.depth_filtered_pointer() == 0                 # an error allocates and writes nothing
        good("a missing guide")
        bad = [("a NULL context", lambda: call(None, d, g, 2, 12, 0.04, 3, MEDIAN)),
               ("a NULL map", lambda: call(h, None, g, 2, 12, 0.04, 3, MEDIAN)),
               ("a NULL fetch array", lambda: lib.mvs_depth_filter_fetch(h, None)),
               ("a NULL context in the fetch", lambda: lib.mvs_depth_filter_fetch(None, fp)),
               ("radius 0", lambda: call(h, d, g, 0, 12, 0.04, 3, MEDIAN)),
               ("radius 5", lambda: call(h, d, g, 5, 12, 0.04, 3, MEDIAN)),
               ("tau -1", lambda: call(h, d, g, 2, -1, 0.04, 3, MEDIAN)),
               ("tau 256", lambda: call(h, d, g, 2, 256, 0.04, 3, MEDIAN)),
               ("a negative max_step", lambda: call(h, d, g, 2, 12, -0.04, 3, MEAN)),
               ("a NaN max_step", lambda: call(h, d, g, 2, 12, float("nan"), 3, MEAN)),
               ("no stage", lambda: call(h, d, g, 2, 12, 0.04, 3, 0)),
               ("unknown flag bits", lambda: call(h, d, g, 2, 12, 0.04, 3, MEDIAN | 8)),
               ("FILL without MEDIAN", lambda: call(h, d, g, 2, 12, 0.04, 3, MEAN | FILL)),
               ("FILL alone", lambda: call(h, d, g, 2, 12, 0.04, 3, FILL)),
               ("min_members 0 with FILL", lambda: call(h, d, g, 2, 12, 0.04, 0, MEDIAN | FILL)),
               ("min_members 82 with FILL", lambda: call(h, d, g, 2, 12, 0.04, 82, MEDIAN | FILL))]
        for what, fn in bad:
            assert fn() == EINVAL, what
            good(what)
        # min_members is ignored without FILL; max_step 0 and +inf are legal
        assert call(h, d, g, 2, 12, 0.0, -5, MEDIAN | MEAN) == 0 and call(h, d, g, 2, 12, INF, 1000, MEDIAN) == 0
        good("the legal extremes")
        with pytest.raises(mvs_amd.MvsError, match="radius 7 outside 1..4"):
            ctx.depth_filter(depth.data_ptr(), radius=7)


def _coarse_to_fine_reference(oracle, views, DC, DB, filter):
    """coarse_to_fine as the composition of the oracle, band_mirror and the filter mirror -> (result, the band's volume)"""
    main_cam, main_img, side_cams, sides = views
    H, W = main_img.shape
    _, _, index, vol = oracle.sweep(main_cam, main_img, side_cams, sides, DC, want_volume=True, nthreads=4, sampler="fixed")
    prior = oracle.refine_depth(vol, oracle.plane_table(DC, -1.0, 1.0), index, sampler="fixed")
    smooth = lambda d, step: dm.filter(d, filter["radius"], filter["tau"], f32(filter["max_steps"] * step), main_img)
    if filter:
        prior = smooth(prior, 2.0 / DC)
    hb = float(f32(1.5 * 2.0 / DC))
    delta = bc.offsets(oracle, DB, hb)
    band = bm.band_volume(oracle, main_cam, main_img, side_cams, sides, prior, delta)
    index = oracle.argmin(band, delta, sampler="fixed")[2]
    out = bm.resolve(prior, oracle.refine_depth(band, delta, index, sampler="fixed"), index)
    return (smooth(out, 2.0 * hb / DB) if filter else out), band


def test_coarse_to_fine_with_the_filter(oracle):
    W, H, V, DC, DB = 96, 64, 4, 16, 16
    main_cam, main_img, side_cams, sides, truth = synth.make_views(W, H, V)
    views = (main_cam, main_img, side_cams, sides)
    filter = dict(radius=3, tau=40, max_steps=4.0)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, 1)
        ref, band = _coarse_to_fine_reference(oracle, views, DC, DB, None)
        _same(mvs_amd.coarse_to_fine(ctx, DC, DB, filter=None), ref, "filter=None: today's result")
        assert ctx.depth_filtered_pointer() == 0
        np.testing.assert_array_equal(ctx.sweep_fetch(want_volume=True)[3], band)
        ref, band = _coarse_to_fine_reference(oracle, views, DC, DB, filter)
        _same(mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter), ref, "coarse_to_fine(filter=...)")
        np.testing.assert_array_equal(ctx.sweep_fetch(want_volume=True)[3], band, err_msg="the band ran on the filtered prior")
        assert mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter, fetch=False) is None
        got = np.empty((H, W), np.float32)
        assert ctx.lib.mvs_depth_filter_fetch(ctx.h, got.ctypes.data_as(C.POINTER(C.c_float))) == 0
        _same(got, ref, "fetch=False: the result stays at depth_filtered_pointer()")
        with pytest.raises(ValueError, match="unknown keys"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, filter=dict(radius=2, max_step=0.1))


def test_pyramid_coarse_to_fine_with_the_filter():
    """the pyramid helper filters each level's upsampled prior on that level and the finest resolved map: the same Context calls made by
    hand give the same bytes, and filter=None the bytes of the helper as it was"""
    W, H, V, DC, DB = 96, 64, 3, 12, 8
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    filter = dict(radius=2, tau=255, max_steps=6.0)

    def levels():
        fine, half = mvs_amd.Context(W, H, 0, sampler="fixed"), mvs_amd.Context(W // 2, H // 2, 0, sampler="fixed")
        fine.sweep_set(main_cam, main_img, side_cams, sides, 1)
        return fine, half

    fine, half = levels()
    with fine, half:
        plain = mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB)
        assert fine.depth_filtered_pointer() == 0
        _same(mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, filter=None), plain, "filter=None")
        got = mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, filter=filter)
    fine, half = levels()
    with fine, half:
        fine.pyramid_stage(half)
        half.sweep_set_planes(DC, -1.0, 1.0)
        half.sweep_run(0, None, BOTH)
        half.sweep_refine_depth()
        fine.pyramid_prior(half, None, 255)
        fine.synchronize()
        upsampled = torch.as_tensor(mvs_amd._DeviceArray(fine.sweep_band_pointers()[1], (H, W), "<f4"), device="cuda").cpu().numpy()
        prior = dm.filter(upsampled, 2, 255, f32(6.0 * 2.0 / DC), None)
        _same(fine.depth_filter(fine.sweep_band_pointers()[1], 2, 255, float(f32(6.0 * 2.0 / DC))), prior, "the upsampled prior, filtered")
        hb = float(f32(1.5 * 2.0 / DC))
        fine.sweep_set_planes(DB, -hb, hb)
        fine.sweep_run_band(fine.depth_filtered_pointer(), 0, None, BOTH)
        fine.sweep_refine_depth()
        resolved = fine.sweep_band_resolve()
        _same(got, dm.filter(resolved, 2, 255, f32(6.0 * (2.0 * hb / DB)), None), "pyramid_coarse_to_fine(filter=...)")
    assert (got.view(np.uint32) != plain.view(np.uint32)).any()
