"""mvs_sweep_run_band_bestk on the device (csrc/band_bestk.hip), bit-identical to the mirror (tests/band_bestk_mirror.py, DESIGN.md
section 24) throughout: the crafted case through every combination of outputs, both costs, the radii and the keeps, then resolve and
report; frames at the kernel's own edges with holes and dead planes on the tile seams; the three identities against the sweeps it joins;
view ranges; every way of staging the frames; the three sources of a prior; the readers behind the volume; the band state; every error of
the list; and the coarse-to-fine helpers with a cost against the same composition of mirrors."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_bestk_cases as bb
import band_bestk_mirror as bbm
import band_mirror as bm
import clean_mirror as cm
import mvs_amd
import pyramid_cases as pc
import pyramid_mirror as pm
import sgm_mirror as sgm
import window_mirror as wm
import zncc_cases as zc
from test_zncc_gpu import PLANE_CHUNK, TILE, _device, _noise_views, _same_cells, _same_maps

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
VOLUME, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOLUME | FUSED
ABSDIFF, ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL
f32 = np.float32


def _same_floats(got, ref, what):
    got, ref = np.asarray(got, f32), np.asarray(ref, f32)
    assert got.shape == ref.shape
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, "%s: %d of %d values differ; first at %s: %r, expected %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def _device_map(ptr, H, W):
    torch.cuda.synchronize()
    return torch.as_tensor(mvs_amd._DeviceArray(ptr, (H, W), "<f4"), device="cuda").cpu().numpy()


def test_the_bindings_constants_are_the_mirrors():
    assert (ABSDIFF, ZNCC, KEEP_ALL) == (bbm.COST_ABSDIFF, bbm.COST_ZNCC, bbm.KEEP_ALL)


def _crafted_context():
    c = bb.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set(*c.views(), c.D, -c.HB, c.HB)
    return c, ctx, _device(c.prior)


@pytest.mark.parametrize("cost,r", bb.COST_RADII)
def test_crafted_case(oracle, cost, r):
    c, ctx, prior = _crafted_context()
    delta = c.offsets(oracle)
    with ctx:
        for keep in bb.KEEPS:
            what = "%s r = %d keep = %d: " % (bb.NAMES[cost], r, keep)
            ref = bb.crafted_volume(cost, r, keep)
            maps = bb.maps(oracle, ref, delta)
            ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what + "volume | fused")
            _same_maps(got[:3], maps, what + "volume | fused")
            _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], maps[2]), what + "resolved")
            assert ctx.sweep_band_report() == bm.report(c.prior, maps[0], maps[2], c.D)
            # the volume alone, then the two-step selection and the refinement
            ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, 1, BOTH)        # (other cells and maps in between)
            ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, what + "volume alone")
            ctx.sweep_argmin()
            _same_maps(ctx.sweep_fetch()[:3], maps, what + "volume, then mvs_sweep_argmin")
            ctx.sweep_refine_depth()
            refined = bb.maps(oracle, ref, delta, refine=True)
            _same_maps(ctx.sweep_fetch()[:3], refined, what + "refined")
            _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, refined[0], refined[2]), what + "refined, resolved")
            assert ctx.sweep_band_report() == bm.report(c.prior, refined[0], refined[2], c.D)
    # the selection alone, on a context that never had a volume
    for keep in bb.KEEPS:
        c, ctx, prior = _crafted_context()
        with ctx:
            ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, FUSED)
            _same_maps(ctx.sweep_fetch()[:3], bb.maps(oracle, bb.crafted_volume(cost, r, keep), delta), "%s r = %d keep = %d: fused alone" % (bb.NAMES[cost], r, keep))


def _seam_prior(W, H, seed):
    """a ramp with noise of a plane step, holes and dead planes on the tile seams (columns 31 / 32, rows 15 / 16) and at the frame's edge"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    prior = (-0.2 + 0.4 * x / W + 0.005 * y + rng.uniform(-0.02, 0.02, (H, W))).astype(f32)
    for row, col, v in ((3, 31, np.nan), (4, 32, 1.0), (15, 5, np.nan), (16, 6, -1.0), (15, 31, 0.9), (16, 32, -0.9), (15, 32, np.nan), (16, 31, 0.995),
                        (0, 0, np.nan), (2, 2, 0.9), (10, 31, 0.9), (11, 32, np.nan), (15, 40, 0.9), (16, 41, np.nan), (30, 30, 1.0), (4, 8, -0.9)):
        if row < H and col < W:
            prior[row, col] = v
    return prior


@pytest.mark.parametrize("cost", (ABSDIFF, ZNCC))
@pytest.mark.parametrize("W,H,r", [(9, 5, 4),                               # a frame smaller than the halo
                                   (2 * TILE[0], 2 * TILE[1], 2),           # whole tiles, both seams
                                   (2 * TILE[0], TILE[1], 1),
                                   (TILE[0] + 1, TILE[1] + 1, 3),           # one pixel into the next tile
                                   (TILE[0] - 1, 2 * TILE[1] - 1, 4)])
def test_shapes_at_the_kernels_edges(oracle, cost, W, H, r):
    views = _noise_views(W, H, 3, 0x2ACC + W)
    prior = _seam_prior(W, H, 0xBE57 + W)
    prior_t = _device(prior)
    assert PLANE_CHUNK == 2
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1, -0.2, 0.2)
        for D in (1, 2, 3):                                                 # odd plane counts against the chunk of 2
            what = "%d x %d x %d, %s r = %d" % (W, H, D, bb.NAMES[cost], r)
            delta = oracle.plane_table(D, -0.2, 0.2)
            ref = bbm.volume(oracle, cost, *views, prior, delta, r, 2)
            live = bm.planes(prior, delta)[1]
            assert (ref >> 24).max() == 2 and (ref[live] == 0).any() and not live.all(), what
            ctx.sweep_set_planes(D, -0.2, 0.2)
            ctx.sweep_run_band_bestk(prior_t.data_ptr(), cost, r, 2, 0, 3, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what)
            _same_maps(got[:3], bb.maps(oracle, ref, delta), what)


def test_identities_against_the_sweeps_it_joins():
    c = zc.crafted()
    zero = _device(np.zeros((c.H, c.W), f32))
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*c.views(), c.D, c.Z_LO, c.Z_HI)
        # (a) a zero prior: mvs_sweep_run_bestk on the same table; (c) with ZNCC and MVS_KEEP_ALL: mvs_sweep_run_zncc
        for cost, r in bb.COST_RADII:
            for keep in (KEEP_ALL, 2, 8):
                ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
                ref = ctx.sweep_fetch(want_volume=True)
                ctx.sweep_run_band_bestk(zero.data_ptr(), cost, r, keep, 0, c.V, BOTH)
                got = ctx.sweep_fetch(want_volume=True)
                _same_cells(got[3], ref[3], "(a) %s r = %d keep = %d" % (bb.NAMES[cost], r, keep))
                _same_maps(got[:3], ref[:3], "(a) %s r = %d keep = %d" % (bb.NAMES[cost], r, keep))
        for r in (1, 2, 3, 4):
            ctx.sweep_run_zncc(r, 0, c.V, VOLUME)
            ref = ctx.sweep_fetch(want_volume=True)[3]
            ctx.sweep_run_band_bestk(zero.data_ptr(), ZNCC, r, KEEP_ALL, 0, c.V, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, "(c) r = %d" % r)
    # (b) the absolute difference at radius 0 with MVS_KEEP_ALL: mvs_sweep_run_band
    c, ctx, prior = _crafted_context()
    with ctx:
        for first, count in bb.RANGES:
            ctx.sweep_run_band(prior.data_ptr(), first, count, BOTH)
            ref = ctx.sweep_fetch(want_volume=True)
            ctx.sweep_run_band_bestk(prior.data_ptr(), ABSDIFF, 0, KEEP_ALL, first, count, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref[3], "(b) views [%d, %d)" % (first, first + count))
            _same_maps(got[:3], ref[:3], "(b) views [%d, %d)" % (first, first + count))


@pytest.mark.parametrize("cost,r", [(ABSDIFF, 1), (ZNCC, 2)])
def test_view_ranges(oracle, cost, r):
    c, ctx, prior = _crafted_context()
    delta = c.offsets(oracle)
    with ctx:
        every = {}
        for first, count in bb.RANGES:
            for keep in (2, 3, KEEP_ALL):
                what = "%s r = %d keep = %d, views [%d, %d)" % (bb.NAMES[cost], r, keep, first, first + count)
                ref = bb.crafted_volume(cost, r, keep, range(first, first + count))
                ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, first, count, BOTH)
                got = ctx.sweep_fetch(want_volume=True)
                _same_cells(got[3], ref, what)
                _same_maps(got[:3], bb.maps(oracle, ref, delta), what)
                every[first, count, keep] = got[3]
        _same_cells(every[0, 2, KEEP_ALL] + every[2, 3, KEEP_ALL], every[0, 5, KEEP_ALL], "MVS_KEEP_ALL: views [0, 2) + [2, 5)")
        assert (every[0, 2, 2] + every[2, 3, 2] != every[0, 5, 2]).any()
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, 2, 2, 0, BOTH)         # no view: nothing is counted anywhere
        got = ctx.sweep_fetch(want_volume=True)
        assert not got[3].any() and (got[2] == -1).all() and (got[0] == 1.0).all() and np.isinf(got[1]).all()


def test_staged_state(oracle):
    c = bb.crafted()
    cost, r, keep = ZNCC, 2, 2
    delta = c.offsets(oracle)
    ref = bb.crafted_volume(cost, r, keep)
    maps = bb.maps(oracle, ref, delta)
    prior = _device(c.prior)
    # the _device setters
    main_t, side_t = _device(c.main_img), [_device(s) for s in c.sides]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main_device(c.main_cam, main_t.data_ptr())
        ctx.sweep_set_views_device(c.side_cams, [t.data_ptr() for t in side_t])
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "device setters")
        _same_maps(got[:3], maps, "device setters")
    # the slots left staged by mvs_sweep_handles
    slots = [4, 0, 3, 1]
    part = bb.crafted_volume(cost, r, keep, (0, 1, 2))
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.frame_store(6)
        ctx.frame_upload(slots[0], c.main_img)
        for v in range(3):
            ctx.frame_upload(slots[1 + v], c.sides[v])
        ctx.sweep_handles(slots[0], c.main_cam, slots[1:], c.side_cams[:3], 8)      # leaves the slots staged
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, 3, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], part, "frame store")
        _same_maps(got[:3], bb.maps(oracle, part, delta), "frame store")
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 1, 2, VOLUME)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], bb.crafted_volume(cost, r, keep, (1, 2)), "frame store, views [1, 3)")
    # the caller's volume
    c, ctx, prior = _crafted_context()
    with ctx:
        vol_t = torch.empty(c.D * c.H * c.W + 5, dtype=torch.int32, device="cuda")
        vol_t.fill_(-1)
        torch.cuda.synchronize()
        ctx.sweep_use_volume(vol_t.data_ptr(), vol_t.numel() * 4)
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
        got = ctx.sweep_fetch()
        mine = vol_t.cpu().numpy().view(np.uint32)
        _same_cells(mine[:-5].reshape(ref.shape), ref, "caller's volume")
        assert (mine[-5:] == 0xffffffff).all()
        _same_maps(got[:3], maps, "caller's volume")
        ctx.sweep_use_volume(0, 0)


def test_the_three_sources_of_a_prior(oracle):
    """the context's own depth map after a coarse best-K run (the copy is ordered before the kernel that overwrites the map), the prior
    buffer after mvs_pyramid_prior (no copy), and the filtered map"""
    W, H, DC, DB, r = 96, 64, 8, 4, 2
    views, _ = bb.exposure_views(W, H)
    hb = float(f32(1.5 * 2.0 / DC))
    delta = oracle.plane_table(DB, -hb, hb)
    coarse = bb.global_level(oracle, views, DC, -1.0, 1.0, ZNCC, r, KEEP_ALL)[1]
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, DC)
        ctx.sweep_run_bestk(ZNCC, r, KEEP_ALL, 0, None, BOTH)
        ctx.sweep_refine_depth()
        _same_floats(ctx.sweep_fetch()[0], coarse, "the coarse level")
        ctx.sweep_set_planes(DB, -hb, hb)
        ctx.sweep_run_band_bestk(ctx.sweep_result_pointers()[0], ZNCC, r, KEEP_ALL, 0, None, BOTH)
        ref = bbm.level(oracle, ZNCC, *views, coarse, delta, r, KEEP_ALL)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref[1], "prior = the context's own depth map")
        _same_floats(_device_map(ctx.sweep_band_pointers()[1], H, W), coarse, "the context's copy of the prior")
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], ref[2], "prior = the context's own depth map")
        _same_floats(ctx.sweep_band_resolve(), ref[0], "resolved")
        # the filtered map of that result as the next prior
        smooth = bb.filtered(ref[0], views[1], dict(radius=2, tau=40, max_steps=4.0), 2.0 * hb / DB)
        ctx.depth_filter(ctx.sweep_band_pointers()[0], radius=2, tau=40, max_step=float(f32(4.0 * (2.0 * hb / DB))), fetch=False)
        ctx.sweep_run_band_bestk(ctx.depth_filtered_pointer(), ZNCC, r, 2, 0, None, BOTH)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], bbm.volume(oracle, ZNCC, *views, smooth, delta, r, 2), "prior = the filtered map")
    # the prior buffer itself, filled by mvs_pyramid_prior from the level below
    lv = pc.levels(views[1], views[3], 2)
    half_views = (views[0], lv[1][0], views[2], lv[1][1])
    below = bb.global_level(oracle, half_views, DC, -1.0, 1.0, ZNCC, r, KEEP_ALL)[1]
    prior = pm.prior(below, 255, lv[1][0], lv[0][0])
    fine, half = mvs_amd.Context(W, H, 0, sampler="fixed"), mvs_amd.Context(W // 2, H // 2, 0, sampler="fixed")
    with fine, half:
        fine.sweep_set(*views, 1)
        fine.pyramid_stage(half)
        half.sweep_set_planes(DC, -1.0, 1.0)
        half.sweep_run_bestk(ZNCC, r, KEEP_ALL, 0, None, BOTH)
        half.sweep_refine_depth()
        fine.pyramid_prior(half, None, 255)
        fine.sweep_set_planes(DB, -hb, hb)
        fine.sweep_run_band_bestk(fine.sweep_band_pointers()[1], ZNCC, r, KEEP_ALL, 0, None, BOTH)
        _same_cells(fine.sweep_fetch(want_volume=True)[3], bbm.volume(oracle, ZNCC, *views, prior, delta, r, KEEP_ALL), "prior = the prior buffer after mvs_pyramid_prior")


def test_downstream_readers(oracle):
    c, ctx, prior = _crafted_context()
    cost, r, keep = ZNCC, 2, 2
    vol = bb.crafted_volume(cost, r, keep)
    delta = c.offsets(oracle)
    seen = sgm.seen_cells(vol, 24)
    with ctx:
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
        ctx.sweep_aggregate(4, 16, 128, 4080, refine=True)
        S = sgm.aggregate(sgm.cost16(vol, 24, 4080), 4, 16, 128)
        np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)
        _, acost, index = sgm.select(S, seen, delta, 4)
        maps = (sgm.refine(S, seen, delta, index), acost, index)
        _same_maps(ctx.sweep_fetch()[:3], maps, "aggregated")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], index), "resolve after the aggregation")
        assert ctx.sweep_band_report() == bm.report(c.prior, maps[0], index, c.D)
        ctx.sweep_window(1, 255, None, select=True)
        Wv = wm.window(vol, 24, 1)
        _same_cells(ctx.sweep_window_fetch(), Wv, "windowed")
        maps = bb.maps(oracle, Wv, delta)
        _same_maps(ctx.sweep_fetch()[:3], maps, "window select")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], maps[2]), "resolve after the window")
        ctx.sweep_argmin()
        before = bb.maps(oracle, vol, delta)
        _same_maps(ctx.sweep_fetch()[:3], before, "mvs_sweep_argmin restores the maps")
        ctx.sweep_clean(0, 10, 4, 1)
        cleaned = cm.clean(*before, vol=vol, cs=24, uniqueness=10, speckle_min_size=4, speckle_max_diff=1)
        _same_maps(ctx.sweep_fetch()[:3], cleaned[:3], "cleaned")
        assert ctx.sweep_clean_report() == list(cleaned[3])
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, cleaned[0], cleaned[2]), "resolve after the cleaning")
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, "the readers left the volume alone")


def test_state_for_later_calls(oracle):
    c, ctx, prior = _crafted_context()
    cost, r, keep = ABSDIFF, 1, 2
    delta = c.offsets(oracle)
    vol = bb.crafted_volume(cost, r, keep)
    fp, ip = (C.c_float * (c.W * c.H))(), (C.c_int * 4)()
    with ctx:
        lib, h = ctx.lib, ctx.h
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
        assert lib.mvs_sweep_band_fetch(h, fp) == ESTATE and lib.mvs_sweep_band_report(h, ip) == ESTATE, "this run is not resolved yet"
        maps = bb.maps(oracle, vol, delta)
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], maps[2]), "resolve")
        assert lib.mvs_sweep_band_fetch(h, fp) == 0 and ctx.sweep_band_report() == bm.report(c.prior, maps[0], maps[2], c.D)
        _same_floats(np.frombuffer(fp, f32).reshape(c.H, c.W), bm.resolve(c.prior, maps[0], maps[2]), "fetch")
        # no selection without MVS_SWEEP_FUSED_ARGMIN
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, VOLUME)
        assert lib.mvs_sweep_band_resolve(h) == ESTATE and lib.mvs_sweep_refine_depth(h) == ESTATE and lib.mvs_sweep_clean(h, 0, 0, 4, 1, 0) == ESTATE
        ctx.sweep_argmin()
        ctx.sweep_refine_depth()
        refined = bb.maps(oracle, vol, delta, refine=True)
        _same_maps(ctx.sweep_fetch()[:3], refined, "argmin, then the refinement")
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, refined[0], refined[2]), "resolve after the two-step selection")
        # an ordinary sweep ends the band state
        for ordinary in (lambda: ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH), lambda: ctx.sweep_run(0, c.V, BOTH), lambda: ctx.sweep_run_zncc(2, 0, c.V, BOTH)):
            ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
            ctx.sweep_band_resolve(fetch=False)
            ordinary()
            assert lib.mvs_sweep_band_resolve(h) == ESTATE and lib.mvs_sweep_band_fetch(h, fp) == ESTATE and lib.mvs_sweep_band_report(h, ip) == ESTATE
        # a band run of the other kind takes the state over
        ctx.sweep_run_band(prior.data_ptr(), 0, c.V, BOTH)
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
        assert lib.mvs_sweep_band_fetch(h, fp) == ESTATE
        _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, maps[0], maps[2]), "after mvs_sweep_run_band")


def test_errors(oracle):
    c = bb.crafted()
    cost, r, keep = ZNCC, 2, 2
    delta = c.offsets(oracle)
    ref = bb.crafted_volume(cost, r, keep)
    maps = bb.maps(oracle, ref, delta)
    prior = _device(c.prior)
    pp = C.c_void_p(prior.data_ptr())
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h
        run = lib.mvs_sweep_run_band_bestk            # (ctx, view_first, view_count, prior, cost, radius, keep, flags)

        def good(what):
            ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what)
            _same_maps(got[:3], maps, what)

        assert run(None, 0, 0, pp, cost, r, keep, BOTH) == EINVAL
        # nothing staged: no planes, no main view, no views
        assert run(h, 0, 0, pp, cost, r, keep, BOTH) == ESTATE
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        assert run(h, 0, 0, pp, cost, r, keep, BOTH) == ESTATE
        ctx.sweep_set_main(c.main_cam, c.main_img)
        assert run(h, 0, 0, pp, cost, r, keep, BOTH) == ESTATE and b"views" in lib.mvs_last_error(h)
        assert not lib.mvs_sweep_depth_device(h) and not lib.mvs_sweep_band_prior_device(h), "a refused call allocates nothing"
        ctx.sweep_set_views(c.side_cams, c.sides)
        good("after MVS_ESTATE")
        # the maps and the volume of another run, which no refused call may touch
        def other_run():
            ctx.sweep_run_band_bestk(prior.data_ptr(), ABSDIFF, 1, 3, 0, 3, BOTH)
        other_run()
        other = ctx.sweep_fetch(want_volume=True)
        _same_cells(other[3], bb.crafted_volume(ABSDIFF, 1, 3, (0, 1, 2)), "absolute difference, radius 1, keep 3, views [0, 3)")
        V = c.V
        for args in ((0, V, None, cost, r, keep, BOTH),                                                                       # no prior
                     (0, V, pp, 2, r, keep, BOTH), (0, V, pp, -1, r, keep, BOTH),                                             # unknown cost
                     (0, V, pp, ZNCC, 0, keep, BOTH), (0, V, pp, ZNCC, 5, keep, BOTH), (0, V, pp, ZNCC, -1, keep, BOTH),      # radius outside the cost's range
                     (0, V, pp, ABSDIFF, 5, keep, BOTH), (0, V, pp, ABSDIFF, -1, keep, BOTH),
                     (0, V, pp, cost, r, 9, BOTH), (0, V, pp, cost, r, -1, BOTH),                                             # keep outside 0..8
                     (-1, 2, pp, cost, r, keep, BOTH), (0, V + 1, pp, cost, r, keep, BOTH), (4, 2, pp, cost, r, keep, BOTH), (0, -1, pp, cost, r, keep, BOTH),
                     (0, V, pp, cost, r, keep, 0), (0, V, pp, cost, r, keep, BOTH | mvs_amd.MVS_SWEEP_FORCE_GENERIC),
                     (0, V, pp, cost, r, keep, BOTH | mvs_amd.MVS_SWEEP_NO_RECT), (0, V, pp, cost, r, keep, VOLUME | 0x100),
                     (0, V, pp, cost, r, keep, 0x80000000 | FUSED)):
            assert run(h, *args) == EINVAL, args
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], other[3], "after EINVAL %s" % (args[3:],))
            _same_maps(got[:3], other[:3], "after EINVAL %s" % (args[3:],))
            good("after EINVAL %s" % (args[3:],))
            other_run()
        # a plane table that is not inside (-1, 1)
        ctx.sweep_set_planes(c.D, -0.9, 1.4)       # the last offset is above 1
        assert oracle.plane_table(c.D, -0.9, 1.4)[-1] > 1.0
        assert run(h, 0, V, pp, cost, r, keep, BOTH) == ESTATE and b"(-1, 1)" in lib.mvs_last_error(h)
        ctx.sweep_set_planes(c.D, -c.HB, c.HB)
        good("after a table outside (-1, 1)")
        # the exact sampler
        ctx.set_sampler("exact")
        assert run(h, 0, V, pp, cost, r, keep, BOTH) == ESTATE and b"FIXED" in lib.mvs_last_error(h)
        ctx.set_sampler("fixed")
        good("after the exact sampler")
        # a caller's volume that is one cell short: refused for a volume run, not needed by a selection alone
        short = torch.empty(c.D * c.H * c.W - 1, dtype=torch.int32, device="cuda")
        short.fill_(7)
        torch.cuda.synchronize()
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert run(h, 0, V, pp, cost, r, keep, BOTH) == EINVAL and b"caller volume" in lib.mvs_last_error(h)
        assert run(h, 0, V, pp, cost, r, keep, VOLUME) == EINVAL
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, V, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], maps, "fused alone beside a short volume")
        assert (short.cpu() == 7).all(), "a refused call wrote into the caller's volume"
        ctx.sweep_use_volume(0, 0)
        good("after the short volume")


FILTER = dict(radius=3, tau=40, max_steps=4.0)


@pytest.mark.parametrize("cost,filter", [(dict(cost="zncc", radius=3), FILTER), (dict(cost="zncc", radius=2, keep=2), None),
                                         (dict(cost="absdiff", radius=1, keep=3), FILTER)])
def test_coarse_to_fine_with_a_cost(oracle, cost, filter):
    W, H, DC, DB = 96, 64, 16, 16
    views, _ = bb.exposure_views(W, H)
    kind = ZNCC if cost["cost"] == "zncc" else ABSDIFF
    ref, prior, vol, maps, resolved = bb.two_levels(oracle, views, DC, DB, kind, cost["radius"], cost.get("keep", KEEP_ALL), filter)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1)
        _same_floats(mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter, cost=cost), ref, "coarse_to_fine(cost=%s, filter=%s)" % (cost, filter))
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], vol, "the band's volume")
        _same_maps(got[:3], maps, "the band's maps")
        _same_floats(_device_map(ctx.sweep_band_pointers()[1], H, W), prior, "the band's prior")
        _same_floats(_device_map(ctx.sweep_band_pointers()[0], H, W), resolved, "the resolved map")
        assert ctx.sweep_band_report() == bm.report(prior, maps[0], maps[2], DB)
        assert mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter, cost=cost, fetch=False) is None
        last = ctx.depth_filtered_pointer() if filter else ctx.sweep_band_pointers()[0]
        _same_floats(_device_map(last, H, W), ref, "fetch=False: the result stays on the device")
        with pytest.raises(ValueError, match="unknown keys"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=dict(cost="zncc", r=2))
        with pytest.raises(ValueError, match="neither"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=dict(cost="ncc"))


def test_coarse_to_fine_without_a_cost_issues_todays_calls():
    W, H, DC, DB = 96, 64, 16, 16
    views, _ = bb.exposure_views(W, H)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1)
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=None)
        vol = ctx.sweep_fetch(want_volume=True)[3]
        hb = float(f32(1.5 * 2.0 / DC))
        ctx.sweep_set_planes(DC, -1.0, 1.0)
        ctx.sweep_run(0, None, BOTH)
        ctx.sweep_refine_depth()
        ctx.sweep_set_planes(DB, -hb, hb)
        ctx.sweep_run_band(ctx.sweep_result_pointers()[0], 0, None, BOTH)
        ctx.sweep_refine_depth()
        _same_floats(got, ctx.sweep_band_resolve(), "cost=None")
        _same_cells(vol, ctx.sweep_fetch(want_volume=True)[3], "cost=None: the band's volume")


@pytest.mark.parametrize("filter", (None, FILTER))
def test_pyramid_coarse_to_fine_with_a_cost(oracle, filter):
    W, H, DC, DB, r, tau = 96, 64, 16, 16, 2, 30
    views, _ = bb.exposure_views(W, H)
    main_cam, main_img, side_cams, sides = views
    lv = pc.levels(main_img, sides, 2)
    below = bb.global_level(oracle, (main_cam, lv[1][0], side_cams, lv[1][1]), DC, -1.0, 1.0, ZNCC, r, KEEP_ALL)[1]
    prior = pm.prior(below, tau, lv[1][0], lv[0][0])
    if filter:
        prior = bb.filtered(prior, main_img, filter, 2.0 / DC)
    hb = float(f32(1.5 * 2.0 / DC))
    resolved, vol, maps = bbm.level(oracle, ZNCC, *views, prior, oracle.plane_table(DB, -hb, hb), r, KEEP_ALL)
    ref = bb.filtered(resolved, main_img, filter, 2.0 * hb / DB) if filter else resolved
    fine, half = mvs_amd.Context(W, H, 0, sampler="fixed"), mvs_amd.Context(W // 2, H // 2, 0, sampler="fixed")
    with fine, half:
        fine.sweep_set(*views, 1)
        got = mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, tau=tau, filter=filter, cost=dict(cost="zncc", radius=r))
        _same_floats(got, ref, "pyramid_coarse_to_fine(cost=..., filter=%s)" % (filter,))
        level = fine.sweep_fetch(want_volume=True)
        _same_cells(level[3], vol, "the finest level's volume")
        _same_maps(level[:3], maps, "the finest level's maps")
        _same_floats(half.sweep_fetch()[0], below, "the coarsest level ran mvs_sweep_run_bestk")
