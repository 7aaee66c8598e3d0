"""mvs_depth_fit on the device (csrc/depth_fit.hip), bit-identical to the mirror (tests/depth_fit_mirror.py)
throughout -- z, gx, gy, zfit, the members and the report: the crafted maps (every radius gated and not, maps at the kernel's own edges,
every kind of value, the gates at their thresholds, min_members, collinear members, the full window, zfit at the range's ends), the guide
taken from the staged main image, the context's own maps and the previous output as input, the state it must leave alone, every error of
the list; mvs_depth_fit_normals against rule N1 and through the fusion; mvs_propagate_set_slopes against the propagation's mirror with the
slopes injected; and the helpers' `fit` key and normals="fit"."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_mirror as bm
import depth_filter_mirror as dm
import depth_fit_cases as fc
import depth_fit_mirror as fm
import fusion_cases as fuc
import mvs_amd
import normals_mirror as nm
import propagate_cases as pc
import propagate_mirror as pm
from mvs_amd import synth

pytestmark = pytest.mark.gpu

f32 = np.float32
EINVAL, ESTATE = -1, -3
BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
ABSDIFF, ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL
TILE = (32, 8)        # csrc/depth_fit.hip: FT_TW, FT_TH
INF = float("inf")
MAPS = ("z", "gx", "gy", "zfit", "members")


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _device_map(ptr, shape, dtype="<f4"):
    torch.cuda.synchronize()
    return torch.as_tensor(mvs_amd._DeviceArray(ptr, shape, dtype), device="cuda").cpu().numpy()


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    view = np.uint32 if got.dtype.itemsize == 4 else np.uint8
    bad = np.argwhere(got.view(view) != ref.view(view))
    assert len(bad) == 0, "%s: %d of %d values differ; first at (row, col, ...) = %s: %r (0x%x), expected %r (0x%x)" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], got.view(view)[tuple(bad[0])], ref[tuple(bad[0])], ref.view(view)[tuple(bad[0])])


def _same_fit(ctx, got, ref, what):
    """the five fetched maps, the maps at their device addresses and the report against the mirror's Fit"""
    for g, r, name in zip(got, ref[:5], MAPS):
        _same(g, r, "%s: %s" % (what, name))
    maps, zfit, members = ctx.depth_fit_pointers()
    H, W = ctx.H, ctx.W
    _same(_device_map(maps, (3, H, W)), np.stack(ref[:3]), what + ": z, gx, gy one behind the other on the device")
    _same(_device_map(zfit, (H, W)), ref.zfit, what + ": zfit on the device")
    _same(_device_map(members, (H, W), "|u1"), ref.members, what + ": members on the device")
    assert ctx.depth_fit_report() == list(ref.report), "%s: report %s, expected %s" % (what, ctx.depth_fit_report(), ref.report)


def _fit(ctx, ptr, case, guide_ptr=None, **kw):
    return ctx.depth_fit(ptr, radius=case.radius, tau=case.tau, max_step=float(case.max_step), min_members=case.min_members, guide_ptr=guide_ptr, **kw)


def test_the_modules_state_the_kernels_tile():
    assert fc.TILE == TILE
    sizes = {c.depth.shape[::-1] for c in fc.cases()}
    assert {(9, 5), TILE, (TILE[0] + 1, TILE[1]), (TILE[0] - 1, TILE[1]), (TILE[0], TILE[1] + 1), (TILE[0], TILE[1] - 1), (2 * TILE[0], 2 * TILE[1])} <= sizes


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c.name)
def test_crafted_map(case):
    """nothing is staged on the context: the guide is the caller's (tau = 255 with a NULL guide among the cases)"""
    H, W = case.depth.shape
    depth = _device(case.depth)
    guide = _device(case.guide) if case.guide is not None else None
    with mvs_amd.Context(W, H, 0) as ctx:
        assert ctx.depth_fit_pointers() == (0, 0, 0) and ctx.depth_fit_normals_pointer() == 0
        got = _fit(ctx, depth.data_ptr(), case, guide.data_ptr() if guide is not None else None)
        _same_fit(ctx, got, fc.reference(case), case.name)


def test_guide_is_the_staged_main_image():
    case = fc.by_name("gated_r3")
    H, W = case.depth.shape
    depth, other = _device(case.depth), _device(255 - case.guide)
    with mvs_amd.Context(W, H, 0) as ctx:
        ctx.sweep_set_main(synth.camera_at([0, 0, 0], W, H), case.guide)
        _same_fit(ctx, _fit(ctx, depth.data_ptr(), case), fc.reference(case), "NULL guide: the staged main image")
        ref = fm.fit(case.depth, case.radius, case.tau, case.max_step, case.min_members, 255 - case.guide)   # a caller's guide takes precedence
        _same_fit(ctx, _fit(ctx, depth.data_ptr(), case, other.data_ptr()), ref, "the caller's guide")


def test_previous_output_as_input_and_a_stable_address():
    """zfit of one call is the input of the next, twice in a row: the launch must not read the map it writes; then the stage's z map"""
    case = fc.by_name("seams_gated")
    H, W = case.depth.shape
    depth, guide = _device(case.depth), _device(case.guide)
    with mvs_amd.Context(W, H, 0) as ctx:
        ref = fc.reference(case)
        _same_fit(ctx, _fit(ctx, depth.data_ptr(), case, guide.data_ptr()), ref, "first call")
        addresses = ctx.depth_fit_pointers()
        for name in ("zfit as input", "zfit as input again"):
            ref = fm.fit(ref.zfit, case.radius, case.tau, case.max_step, case.min_members, case.guide)
            _same_fit(ctx, _fit(ctx, addresses[1], case, guide.data_ptr()), ref, name)
            assert ctx.depth_fit_pointers() == addresses
        ref = fm.fit(ref.z, 2, 255, INF, 4)
        _same_fit(ctx, ctx.depth_fit(addresses[0], 2, 255, INF, 4), ref, "the stage's z map as input")
        # fetch=False leaves the maps on the device; every array of the fetch is optional
        assert _fit(ctx, depth.data_ptr(), case, guide.data_ptr(), fetch=False) is None
        got = np.empty((H, W), np.float32)
        assert ctx.lib.mvs_depth_fit_fetch(ctx.h, None, None, None, got.ctypes.data_as(C.POINTER(C.c_float)), None) == 0
        _same(got, fc.reference(case).zfit, "fetch=False, then the fetch of zfit alone")


def test_the_contexts_own_maps_and_the_state_it_leaves_alone(oracle):
    """the input is the sweep's refined map, a band run's resolved map, the filtered map, the propagation's z map and a depth-store slot;
    each result is the mirror's on the fetched input; the sweep's maps and volume, the selection, the band state and report and the
    filter's map are what they were"""
    W, H, V, D = 45, 23, 3, 12
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    step = f32(2.0 / D)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH)
        ctx.sweep_refine_depth()
        before = ctx.sweep_fetch(want_volume=True)
        got = ctx.depth_fit(ctx.sweep_result_pointers()[0], 2, 30, float(4 * step), 5)
        _same_fit(ctx, got, fm.fit(before[0], 2, 30, 4 * step, 5, main_img), "the sweep's refined map")
        after = ctx.sweep_fetch(want_volume=True)
        for a, b, name in zip(after, before, ("depth", "cost", "index", "volume")):
            np.testing.assert_array_equal(a, b, err_msg="the fit changed the sweep's " + name)
        assert ctx.volume_source() == mvs_amd.MVS_VOLUME_RAW
        # the filtered map as input, and unchanged by the fit
        filtered = ctx.depth_filter(ctx.sweep_result_pointers()[0], 2, 255, INF, fill=3)
        _same_fit(ctx, ctx.depth_fit(ctx.depth_filtered_pointer(), 3, 255, float(2 * step), 6), fm.fit(filtered, 3, 255, 2 * step, 6), "the filtered map")
        _same(_device_map(ctx.depth_filtered_pointer(), (H, W)), filtered, "the filter's map after the fit")
        # a band run on the filtered prior: its resolved map as input; the band state, the report and a later resolve are as they were
        hb = float(f32(1.5 * 2.0 / D))
        ctx.sweep_set_planes(8, -hb, hb)
        ctx.sweep_run_band(ctx.depth_filtered_pointer(), 0, V, BOTH)
        offset, _, index, _ = ctx.sweep_fetch()
        resolved = ctx.sweep_band_resolve()
        _same(resolved, bm.resolve(filtered, offset, index), "the band ran on the filtered prior")
        report = ctx.sweep_band_report()
        _same_fit(ctx, ctx.depth_fit(ctx.sweep_band_pointers()[0], 4, 10, INF, 8), fm.fit(resolved, 4, 10, INF, 8, main_img), "the resolved map")
        _same(ctx.sweep_band_resolve(), resolved, "mvs_sweep_band_resolve after the fit")
        assert ctx.sweep_band_report() == report
        _same(ctx.sweep_fetch()[0], offset, "the band's offset map after the fit")
        # the propagation's z map, and a depth-store slot
        ctx.propagate_init(ctx.sweep_band_pointers()[0], ZNCC, 1, 2)
        state = ctx.propagate_fetch()
        _same_fit(ctx, ctx.depth_fit(ctx.propagate_depth_pointer(), 1, 255, float(step), 3), fm.fit(state[0], 1, 255, step, 3), "the propagation's z map")
        for g, s in zip(ctx.propagate_fetch(), state):
            np.testing.assert_array_equal(g, s, err_msg="the fit changed the propagation's state")
        ctx.depth_store(2)
        ctx.depth_upload(1, main_cam, resolved)
        _same_fit(ctx, ctx.depth_fit(ctx.depth_slot_pointer(1), 2, 255, INF), fm.fit(resolved, 2, 255, INF, 6), "a depth-store slot")


def test_a_context_that_never_fits_has_no_maps():
    W, H, V, D = 45, 23, 2, 4
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH)
        ctx.depth_filter(ctx.sweep_result_pointers()[0], 1)
        ctx.propagate_init(ctx.sweep_result_pointers()[0], ABSDIFF, 1)
        lib, h = ctx.lib, ctx.h
        assert ctx.depth_fit_pointers() == (0, 0, 0) and ctx.depth_fit_normals_pointer() == 0
        fp = np.empty((H, W, 3), np.float32).ctypes.data_as(C.POINTER(C.c_float))
        assert lib.mvs_depth_fit_fetch(h, fp, None, None, None, None) == ESTATE and lib.mvs_depth_fit_report(h, (C.c_longlong * 4)()) == ESTATE
        assert lib.mvs_depth_fit_normals(h, np.eye(4, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))) == ESTATE
        assert lib.mvs_depth_fit_normals_fetch(h, fp) == ESTATE


def test_errors():
    """every error of the list, each followed by a good call that gives the mirror's bytes: nothing was written, the context is usable"""
    case = fc.by_name("gated_r2")
    H, W = case.depth.shape
    depth, guide = _device(case.depth), _device(case.guide)
    d, g = C.c_void_p(depth.data_ptr()), C.c_void_p(guide.data_ptr())
    cam = np.ascontiguousarray(synth.camera_at([0, 0, 0], W, H), np.float32)
    cp = cam.ctypes.data_as(C.POINTER(C.c_float))
    with mvs_amd.Context(W, H, 0) as ctx:
        lib, h = ctx.lib, ctx.h
        call = lib.mvs_depth_fit
        out = np.empty((H, W, 3), np.float32)
        fp = out.ctypes.data_as(C.POINTER(C.c_float))
        lp = (C.c_longlong * 4)()

        def good(what):
            _same_fit(ctx, _fit(ctx, depth.data_ptr(), case, guide.data_ptr()), fc.reference(case), "after " + what)

        assert lib.mvs_depth_fit_fetch(h, fp, None, None, None, None) == ESTATE and b"no fitted maps" in lib.mvs_last_error(h)   # before the first call
        assert lib.mvs_depth_fit_report(h, lp) == ESTATE and lib.mvs_depth_fit_normals(h, cp) == ESTATE and lib.mvs_depth_fit_normals_fetch(h, fp) == ESTATE
        assert call(h, d, None, 2, 12, 0.04, 6) == ESTATE and b"guide" in lib.mvs_last_error(h)                   # tau < 255, nothing staged
        assert ctx.depth_fit_pointers() == (0, 0, 0)               # an error allocates and writes nothing
        good("a missing guide")
        assert lib.mvs_depth_fit_normals_fetch(h, fp) == ESTATE and b"mvs_depth_fit_normals first" in lib.mvs_last_error(h) and ctx.depth_fit_normals_pointer() == 0
        singular = np.zeros((4, 4), np.float32)
        nan_cam = cam.copy()
        nan_cam[1, 2] = np.nan
        bad = [("a NULL context", lambda: call(None, d, g, 2, 12, 0.04, 6)),
               ("a NULL map", lambda: call(h, None, g, 2, 12, 0.04, 6)),
               ("a NULL context in the fetch", lambda: lib.mvs_depth_fit_fetch(None, fp, None, None, None, None)),
               ("a NULL context in the report", lambda: lib.mvs_depth_fit_report(None, lp)),
               ("a NULL report array", lambda: lib.mvs_depth_fit_report(h, None)),
               ("radius 0", lambda: call(h, d, g, 0, 12, 0.04, 6)),
               ("radius 5", lambda: call(h, d, g, 5, 12, 0.04, 6)),
               ("tau -1", lambda: call(h, d, g, 2, -1, 0.04, 6)),
               ("tau 256", lambda: call(h, d, g, 2, 256, 0.04, 6)),
               ("a negative max_step", lambda: call(h, d, g, 2, 12, -0.04, 6)),
               ("a NaN max_step", lambda: call(h, d, g, 2, 12, float("nan"), 6)),
               ("min_members 2", lambda: call(h, d, g, 2, 12, 0.04, 2)),
               ("min_members 82", lambda: call(h, d, g, 2, 12, 0.04, 82)),
               ("a NULL camera", lambda: lib.mvs_depth_fit_normals(h, None)),
               ("a NULL context in the normals", lambda: lib.mvs_depth_fit_normals(None, cp)),
               ("a singular camera", lambda: lib.mvs_depth_fit_normals(h, singular.ctypes.data_as(C.POINTER(C.c_float)))),
               ("a camera with a NaN", lambda: lib.mvs_depth_fit_normals(h, nan_cam.ctypes.data_as(C.POINTER(C.c_float)))),
               ("a NULL normals array", lambda: lib.mvs_depth_fit_normals_fetch(h, None)),
               ("a NULL context in the normals' fetch", lambda: lib.mvs_depth_fit_normals_fetch(None, fp)),
               ("gx without gy", lambda: lib.mvs_propagate_set_slopes(h, d, None)),
               ("gy without gx", lambda: lib.mvs_propagate_set_slopes(h, None, d)),
               ("a NULL context in the setter", lambda: lib.mvs_propagate_set_slopes(None, d, d))]
        for what, fn in bad:
            assert fn() == EINVAL, what
            good(what)
        assert ctx.depth_fit_normals_pointer() == 0                # no refused normals call made a map
        # the legal extremes
        assert call(h, d, g, 1, 0, 0.0, 3) == 0 and call(h, d, g, 4, 255, INF, 81) == 0 and call(h, d, None, 4, 255, INF, 81) == 0
        good("the legal extremes")
        with pytest.raises(mvs_amd.MvsError, match="radius 7 outside 1..4"):
            ctx.depth_fit(depth.data_ptr(), radius=7)


# ---- normals ----------------------------------------------------------------------------------------------------------------------------------
def test_normals_are_rule_n1_on_the_fitted_pixels_and_go_through_the_fusion():
    """fusion_cases.store at 67 x 45: the fit of a slot's map, its normals against rule N1 with zeros at the pixels that are not fitted;
    uploaded into the slots' planes device to device and fused by mvs_fuse_depth_normals, the rows equal normals_mirror's fusion given the
    same planes"""
    W, H = fuc.SIZES[2]
    st = fuc.store(W, H)
    slots = [fuc.ROLLED, fuc.TILTED, fuc.WIDE]
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(fuc.DEPTH_CAP)
        for s in slots:
            ctx.depth_upload(s, st["cams"][s], st["depths"][s], st["costs"][s])
        mats = {s: ctx.depth_slot_matrices(s) for s in slots}
        planes = {}
        for s in slots:
            got = ctx.depth_fit(ctx.depth_slot_pointer(s), 2, 255, 0.05, 6)
            ref = fm.fit(st["depths"][s], 2, 255, f32(0.05), 6)
            _same_fit(ctx, got, ref, "slot %d" % s)
            normals = ctx.depth_fit_normals(st["cams"][s])
            exp = fm.normals(ref, mats[s][0], mats[s][2])
            _same(normals, exp, "slot %d: rule N1 on the fitted pixels, zeros elsewhere" % s)
            fitted, valid = ref.members > 0, dm.valid(st["depths"][s])
            assert fitted.sum() > 1000 and (valid & ~fitted).sum() > 0 and not normals[~fitted].any() and nm.usable(normals[fitted]).all()
            # a valid pixel that is not fitted would get the fronto-parallel plane's normal from rule N1 alone
            assert nm.usable(nm.hypothesis_normals(ref.z, ref.gx, ref.gy, mats[s][0], mats[s][2])[valid & ~fitted]).all()
            assert ctx.depth_fit_normals_pointer() != 0 and ctx.depth_fit_normals(st["cams"][s], fetch=False) == ctx.depth_fit_normals_pointer()
            ctx.depth_normals_upload_device(s, ctx.depth_fit_normals_pointer())
            _same(ctx.depth_normals_fetch(s), normals, "slot %d: the plane" % s)
            planes[s] = normals
        ref_slot, nbrs, kw = fuc.ROLLED, [fuc.TILTED, fuc.WIDE], dict(min_consistent=1)
        rows = ctx.fuse_depth(ref_slot, nbrs, min_normal_cos=0.9, **kw)
        exp = nm.fuse_normals({s: st["depths"][s] for s in slots}, {}, {}, planes, mats, ref_slot, nbrs, min_normal_cos=0.9, **kw)
        assert len(rows) > 100
        _same(rows, exp["rows"], "mvs_fuse_depth_normals over the fit's planes")


# ---- propagation seeds ----------------------------------------------------------------------------------------------------------------------
SeededState = fc.seeded_state      # propagate_mirror's init with the recorded slopes injected


def _same_state(ctx, shot, what):
    got = ctx.propagate_fetch()
    for g, r, name in zip(got, shot[:4], ("z", "gx", "gy", "cells")):
        _same(g, r, "%s: %s" % (what, name))
    _same(_device_map(ctx.propagate_cost_pointer(), (ctx.H, ctx.W)), shot[4], what + ": the cost map")
    assert tuple(ctx.propagate_report()) == tuple(shot[5]), what


def test_recorded_slopes_seed_the_next_init():
    c = pc.crafted()
    cost, r, keep = ZNCC, 2, 2
    fit = fm.fit(c.prior, 3, 255, f32(pc.MAX_STEP), 6)
    gx, gy = fit.gx.copy(), fit.gy.copy()
    live = np.argwhere(pm.inside(np.asarray(c.prior, f32)))
    for (row, col), v in zip(live[::len(live) // 6][:6], (np.nan, np.inf, -np.inf, np.nan, np.inf, -0.0)):   # non-finite seeds become 0
        gx[row, col], gy[row, col] = v, (0.01 if np.isnan(v) else v)
    assert (fit.members > 0).sum() > 500 and not np.isfinite(gx).all()
    seeded = SeededState(pc.crafted_scene(), c.prior, cost, r, keep, gx, gy)
    plain = pc.crafted_states(cost, r, keep, False, 2)[1]
    shots = [pc.snapshot(seeded)]
    for _ in range(2):
        seeded.run(1, pc.DZ, pc.DG, 2, pc.SEED)
        shots.append(pc.snapshot(seeded))
    assert shots[0][3].tobytes() != plain[0][3].tobytes(), "the seeds change no cell"
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main(c.main_cam, c.main_img)
        ctx.sweep_set_views(c.side_cams, c.sides)
        start, dgx, dgy = _device(c.prior), _device(gx), _device(gy)
        init = lambda **kw: ctx.propagate_init(start.data_ptr(), cost, r, keep, **kw)
        # nothing recorded: today's bytes
        init()
        _same_state(ctx, plain[0], "nothing recorded")
        # recorded slopes: the mirror's init with the slopes injected, and two iterations
        ctx.propagate_set_slopes(dgx.data_ptr(), dgy.data_ptr())
        init()
        _same_state(ctx, shots[0], "seeded init")
        for it in (1, 2):
            ctx.propagate_run(1, pc.DZ, pc.DG, 2, pc.SEED)
            _same_state(ctx, shots[it], "seeded, iteration %d" % it)
        # the record is consumed: a second init without a new setter gives today's bytes
        init()
        _same_state(ctx, plain[0], "the record was consumed")
        # recorded slopes with MVS_PROPAGATE_SLOPES: MVS_EINVAL, nothing is consumed and nothing written; so for any refused init
        ctx.propagate_set_slopes(dgx.data_ptr(), dgy.data_ptr())
        with pytest.raises(mvs_amd.MvsError, match="one source of slopes"):
            init(slopes=True)
        with pytest.raises(mvs_amd.MvsError, match="radius"):
            ctx.propagate_init(start.data_ptr(), cost, 9, keep)
        _same_state(ctx, plain[0], "after two refused inits")
        init()
        _same_state(ctx, shots[0], "a refused init leaves the record in place")
        # (NULL, NULL) clears the record
        ctx.propagate_set_slopes(dgx.data_ptr(), dgy.data_ptr())
        ctx.propagate_set_slopes(None, None)
        init(slopes=True, max_step=pc.MAX_STEP)
        _same_state(ctx, pc.crafted_states(cost, r, keep, True, 2)[1][0], "cleared: MVS_PROPAGATE_SLOPES is accepted again")
        # the fit's own slope maps, device to device
        ctx.depth_fit(start.data_ptr(), 3, 255, pc.MAX_STEP, 6, fetch=False)
        maps, plane = ctx.depth_fit_pointers()[0], 4 * c.W * c.H
        ctx.propagate_set_slopes(maps + plane, maps + 2 * plane)
        init()
        _same_state(ctx, pc.snapshot(SeededState(pc.crafted_scene(), c.prior, cost, r, keep, fit.gx, fit.gy)), "seeded from the fit's maps")


# ---- helpers --------------------------------------------------------------------------------------------------------------------------------
def test_coarse_to_fine_with_the_fit_key():
    """coarse_to_fine(..., propagate=dict(..., fit=...)) at 96 x 64 equals the same Context calls made by hand; fit=None and an absent key
    give the helper's bytes as they were; fit with slopes=True and unknown fit keys raise"""
    W, H, V, DC, DB = 96, 64, 3, 8, 8
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V)
    cost = dict(cost="zncc", radius=2)
    fit = dict(radius=3, tau=40, max_steps=4.0, min_members=5)
    propagate = dict(iterations=1, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=5)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, 1)
        plain = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=propagate)
        assert ctx.depth_fit_pointers() == (0, 0, 0)
        _same(mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(propagate, fit=None)), plain, "fit=None: today's result")
        assert ctx.depth_fit_pointers() == (0, 0, 0)
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(propagate, fit=fit))
        state = ctx.propagate_fetch()
        assert got.tobytes() != plain.tobytes()
        with pytest.raises(ValueError, match="slopes=True"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(propagate, fit=fit, slopes=True))
        with pytest.raises(ValueError, match="unknown keys"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(propagate, fit=dict(radius=2, max_step=0.1)))
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, 1)
        ctx.sweep_set_planes(DC, -1.0, 1.0)
        ctx.sweep_run_bestk(ZNCC, 2, KEEP_ALL, 0, None, BOTH)
        ctx.sweep_refine_depth()
        hb = float(f32(1.5 * 2.0 / DC))
        ctx.sweep_set_planes(DB, -hb, hb)
        ctx.sweep_run_band_bestk(ctx.sweep_result_pointers()[0], ZNCC, 2, KEEP_ALL, 0, None, BOTH)
        ctx.sweep_refine_depth()
        resolved = ctx.sweep_band_resolve()
        step = 2.0 * hb / DB
        final = ctx.sweep_band_pointers()[0]
        fitted = ctx.depth_fit(final, 3, 40, float(f32(4.0 * step)), 5)
        _same_fit(ctx, fitted, fm.fit(resolved, 3, 40, f32(4.0 * step), 5, main_img), "the fit of the resolved map")
        maps, plane = ctx.depth_fit_pointers()[0], 4 * W * H
        ctx.propagate_set_slopes(maps + plane, maps + 2 * plane)
        ctx.propagate_init(final, ZNCC, 2, KEEP_ALL)
        _, gx0, gy0, _ = ctx.propagate_fetch()
        _same(gx0, np.where(pm.inside(resolved), fitted[1], f32(0.0)), "init took the fit's gx")
        _same(gy0, np.where(pm.inside(resolved), fitted[2], f32(0.0)), "init took the fit's gy")
        ctx.propagate_run(1, float(f32(0.5 * step)), float(f32(0.125 * step)), 2, 5)
        for g, s, name in zip(ctx.propagate_fetch(), state, ("z", "gx", "gy", "cells")):
            _same(g, s, "coarse_to_fine(fit=...) against the calls by hand: " + name)
        _same(got, ctx.propagate_fetch()[0], "the helper's result")


def test_two_stage_with_the_fits_normals():
    """propagate_two_stage(normals="fit") stores depth_fit_normals of each stage's final z map in that stage's slot; the z maps are the
    ones normals=False gives"""
    W, H, D, n = 64, 32, 8, 3
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, 2)
    cams, imgs = [main_cam] + list(side_cams), [main_img] + list(sides)
    cost = dict(cost="zncc", radius=1, keep=2)
    propagate = dict(iterations=1, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=9)
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
        assert ctx.depth_fit_pointers() == (0, 0, 0)
        got = mvs_amd.propagate_two_stage(*args, cost=cost, propagate=propagate, consistency=term, normals="fit")
        _same(got, plain, "the z maps")
        for s in range(2 * n):
            depth = _device_map(ctx.depth_slot_pointer(s), (H, W))
            P, _, centre = ctx.depth_slot_matrices(s)
            ref = fm.fit(depth, 4, 255, INF, 6)
            _same(ctx.depth_normals_fetch(s), fm.normals(ref, P, centre), "slot %d: the normals of the fit of its map" % s)
            assert (ref.members > 0).mean() > 0.9
        _same(got[n - 1], _device_map(ctx.depth_slot_pointer(2 * n - 1), (H, W)), "the last slot holds the last z map")
