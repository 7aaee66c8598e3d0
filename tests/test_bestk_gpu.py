"""mvs_sweep_run_bestk on the device (csrc/bestk.hip), bit-identical to the mirror (tests/bestk_mirror.py)
throughout: the crafted case through every combination of outputs, both costs, the radii and the keeps; cross-checks against the summing
sweeps that do not rest on the new mirror; frames at the kernel's own edges; view ranges; the readers behind the volume; the state it
leaves for later calls; every error of the list; and the occluder scene whose figures tests/test_bestk_cpu.py reports."""
import numpy as np
import pytest
import torch

import bestk_cases as bk
import bestk_mirror as bm
import clean_mirror as cm
import mvs_amd
import sgm_mirror as sgm
import window_mirror as wm
from test_zncc_gpu import PLANE_CHUNK, TILE, _device, _noise_views, _same_cells, _same_maps

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
VOLUME, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOLUME | FUSED
ABSDIFF, ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL


def test_the_bindings_constants_are_the_mirrors():
    assert (ABSDIFF, ZNCC, KEEP_ALL) == (bm.COST_ABSDIFF, bm.COST_ZNCC, bm.KEEP_ALL)


def _crafted_context():
    c = bk.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set(*c.views(), c.D, c.Z_LO, c.Z_HI)
    return c, ctx


@pytest.mark.parametrize("cost,r", bk.COST_RADII)
def test_crafted_case(oracle, cost, r):
    c, ctx = _crafted_context()
    z = c.planes(oracle)
    with ctx:
        for keep in bk.KEEPS:
            what = "%s r = %d keep = %d: " % (bk.NAMES[cost], r, keep)
            ref = bk.crafted_volume(cost, r, keep)
            maps = bk.maps(oracle, ref, z)
            ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what + "volume | fused")
            _same_maps(got[:3], maps, what + "volume | fused")
            # the volume alone, then the two-step selection and the refinement
            ctx.sweep_run_bestk(cost, r, keep, 0, 1, BOTH)        # (other cells and maps in between)
            ctx.sweep_run_bestk(cost, r, keep, 0, c.V, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, what + "volume alone")
            ctx.sweep_argmin()
            _same_maps(ctx.sweep_fetch()[:3], maps, what + "volume, then mvs_sweep_argmin")
            ctx.sweep_refine_depth()
            _same_maps(ctx.sweep_fetch()[:3], bk.maps(oracle, ref, z, refine=True), what + "refined")
    # the selection alone, on a context that never had a volume
    for keep in bk.KEEPS:
        c, ctx = _crafted_context()
        with ctx:
            ctx.sweep_run_bestk(cost, r, keep, 0, c.V, FUSED)
            _same_maps(ctx.sweep_fetch()[:3], bk.maps(oracle, bk.crafted_volume(cost, r, keep), z), "%s r = %d keep = %d: fused alone" % (bk.NAMES[cost], r, keep))


def test_cross_checks_against_the_summing_sweeps():
    c, ctx = _crafted_context()
    with ctx:
        for r in (1, 2, 3, 4):
            ctx.sweep_run_zncc(r, 0, c.V, VOLUME)
            summed = ctx.sweep_fetch(want_volume=True)[3]
            ctx.sweep_run_bestk(ZNCC, r, KEEP_ALL, 0, c.V, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], summed, "MVS_KEEP_ALL with ZNCC at r = %d against mvs_sweep_run_zncc" % r)
        for first, count in bk.RANGES:
            ctx.sweep_run(first, count, VOLUME | mvs_amd.MVS_SWEEP_NO_RECT)
            summed = ctx.sweep_fetch(want_volume=True)[3]
            ctx.sweep_run_bestk(ABSDIFF, 0, KEEP_ALL, first, count, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], summed, "MVS_KEEP_ALL with the absolute difference at r = 0 against mvs_sweep_run, views [%d, %d)" % (first, first + count))
        for cost, r in bk.COST_RADII:
            for v in (0, 2, 4):
                ctx.sweep_run_bestk(cost, r, KEEP_ALL, v, 1, VOLUME)
                every = ctx.sweep_fetch(want_volume=True)[3]
                ctx.sweep_run_bestk(cost, r, 1, v, 1, VOLUME)
                _same_cells(ctx.sweep_fetch(want_volume=True)[3], every, "keep 1 against MVS_KEEP_ALL over view %d alone" % v)


@pytest.mark.parametrize("cost", (ABSDIFF, ZNCC))
@pytest.mark.parametrize("W,H,D,r", [(9, 5, 3, 4),                                   # smaller than the window in both directions
                                     (2 * TILE[0], 2 * TILE[1], PLANE_CHUNK + 1, 2),  # whole tiles; a chunk and one plane
                                     (2 * TILE[0], TILE[1], 1, 1),                    # one plane
                                     (TILE[0] + 1, TILE[1] + 1, PLANE_CHUNK, 3),      # one pixel into the next tile; whole chunks
                                     (TILE[0] - 1, 2 * TILE[1] - 1, PLANE_CHUNK + 1, 4)])
def test_shapes_at_the_kernels_edges(oracle, cost, W, H, D, r):
    views = _noise_views(W, H, 3, 0x2ACC + W)
    z = oracle.plane_table(D, -0.5, 0.7)
    ref = bm.volume(oracle, cost, *views, D, -0.5, 0.7, r, 2)
    assert (ref >> 24).max() == 2 and (ref == 0).any()
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, D, -0.5, 0.7)
        ctx.sweep_run_bestk(cost, r, 2, 0, 3, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "%d x %d x %d, r = %d" % (W, H, D, r))
        _same_maps(got[:3], bk.maps(oracle, ref, z), "%d x %d x %d, r = %d" % (W, H, D, r))


@pytest.mark.parametrize("cost,r", bk.COST_RADII)
def test_view_ranges(oracle, cost, r):
    c, ctx = _crafted_context()
    z = c.planes(oracle)
    with ctx:
        for first, count in bk.RANGES:
            for keep in (2, 3):
                what = "%s r = %d keep = %d, views [%d, %d)" % (bk.NAMES[cost], r, keep, first, first + count)
                ref = bk.crafted_volume(cost, r, keep, range(first, first + count))
                ctx.sweep_run_bestk(cost, r, keep, first, count, BOTH)
                got = ctx.sweep_fetch(want_volume=True)
                _same_cells(got[3], ref, what)
                _same_maps(got[:3], bk.maps(oracle, ref, z), what)
        ctx.sweep_run_bestk(cost, r, 2, 2, 0, BOTH)         # no view: nothing is counted anywhere
        got = ctx.sweep_fetch(want_volume=True)
        assert not got[3].any() and (got[2] == -1).all() and (got[0] == 1.0).all() and np.isinf(got[1]).all()


def test_downstream_readers(oracle):
    c, ctx = _crafted_context()
    cost, r, keep = ZNCC, 2, 2
    vol = bk.crafted_volume(cost, r, keep)
    z = c.planes(oracle)
    seen = sgm.seen_cells(vol, 24)
    with ctx:
        ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
        ctx.sweep_aggregate(4, 16, 128, 4080, refine=True)
        S = sgm.aggregate(sgm.cost16(vol, 24, 4080), 4, 16, 128)
        np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)
        _, acost, index = sgm.select(S, seen, z, 4)
        _same_maps(ctx.sweep_fetch()[:3], (sgm.refine(S, seen, z, index), acost, index), "aggregated")
        ctx.sweep_window(1, 255, None, select=True)
        Wv = wm.window(vol, 24, 1)
        _same_cells(ctx.sweep_window_fetch(), Wv, "windowed")
        _same_maps(ctx.sweep_fetch()[:3], bk.maps(oracle, Wv, z), "window select")
        ctx.sweep_argmin()
        before = bk.maps(oracle, vol, z)
        _same_maps(ctx.sweep_fetch()[:3], before, "mvs_sweep_argmin restores the maps")
        ctx.sweep_clean(0, 10, 4, 1)
        cleaned = cm.clean(*before, vol=vol, cs=24, uniqueness=10, speckle_min_size=4, speckle_max_diff=1)
        _same_maps(ctx.sweep_fetch()[:3], cleaned[:3], "cleaned")
        assert ctx.sweep_clean_report() == list(cleaned[3])
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, "the readers left the volume alone")


def test_state_for_later_calls(oracle):
    c, ctx = _crafted_context()
    cost, r, keep = ABSDIFF, 1, 2
    prior = _device(np.zeros((c.H, c.W), np.float32))
    with ctx:
        lib, h = ctx.lib, ctx.h
        ctx.sweep_run_band(prior.data_ptr(), 0, 3, BOTH)
        ctx.sweep_band_resolve()
        ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
        assert lib.mvs_sweep_band_resolve(h) == ESTATE, "a best-K run ends the band run's state"
        ctx.sweep_refine_depth()
        ctx.sweep_run_bestk(cost, r, keep, 0, c.V, VOLUME)
        assert lib.mvs_sweep_refine_depth(h) == ESTATE and lib.mvs_sweep_clean(h, 0, 0, 4, 1, 0) == ESTATE, "no selection on this volume yet"
        ctx.sweep_argmin()
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], bk.maps(oracle, bk.crafted_volume(cost, r, keep), c.planes(oracle), refine=True), "argmin, then the refinement")


def test_errors(oracle):
    c = bk.crafted()
    cost, r, keep = ZNCC, 2, 2
    ref = bk.crafted_volume(cost, r, keep)
    maps = bk.maps(oracle, ref, c.planes(oracle))
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h
        run = lib.mvs_sweep_run_bestk            # (ctx, view_first, view_count, cost, radius, keep, flags)

        def good(what):
            ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what)
            _same_maps(got[:3], maps, what)

        assert run(None, 0, 0, cost, r, keep, BOTH) == EINVAL
        # nothing staged: no planes, no main view, no views
        assert run(h, 0, 0, cost, r, keep, BOTH) == ESTATE
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        assert run(h, 0, 0, cost, r, keep, BOTH) == ESTATE
        ctx.sweep_set_main(c.main_cam, c.main_img)
        assert run(h, 0, 0, cost, r, keep, BOTH) == ESTATE and b"views" in lib.mvs_last_error(h)
        assert not lib.mvs_sweep_depth_device(h), "a refused call allocates nothing"
        ctx.sweep_set_views(c.side_cams, c.sides)
        good("after MVS_ESTATE")
        # the maps and the volume of another run, which no refused call may touch
        ctx.sweep_run_bestk(ABSDIFF, 1, 3, 0, 3, BOTH)
        other = ctx.sweep_fetch(want_volume=True)
        _same_cells(other[3], bk.crafted_volume(ABSDIFF, 1, 3, (0, 1, 2)), "absolute difference, radius 1, keep 3, views [0, 3)")
        V = c.V
        for args in ((0, V, 2, r, keep, BOTH), (0, V, -1, r, keep, BOTH),                                            # unknown cost
                     (0, V, ZNCC, 0, keep, BOTH), (0, V, ZNCC, 5, keep, BOTH), (0, V, ZNCC, -1, keep, BOTH),          # radius outside the cost's range
                     (0, V, ABSDIFF, 5, keep, BOTH), (0, V, ABSDIFF, -1, keep, BOTH),
                     (0, V, cost, r, 9, BOTH), (0, V, cost, r, -1, BOTH),                                            # keep outside 0..8
                     (-1, 2, cost, r, keep, BOTH), (0, V + 1, cost, r, keep, BOTH), (4, 3, cost, r, keep, BOTH), (0, -1, cost, r, keep, BOTH),
                     (0, V, cost, r, keep, 0), (0, V, cost, r, keep, BOTH | mvs_amd.MVS_SWEEP_FORCE_GENERIC),
                     (0, V, cost, r, keep, BOTH | mvs_amd.MVS_SWEEP_NO_RECT), (0, V, cost, r, keep, VOLUME | 0x100),
                     (0, V, cost, r, keep, 0x80000000 | FUSED)):
            assert run(h, *args) == EINVAL, args
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], other[3], "after EINVAL %s" % (args,))
            _same_maps(got[:3], other[:3], "after EINVAL %s" % (args,))
            good("after EINVAL %s" % (args,))
            ctx.sweep_run_bestk(ABSDIFF, 1, 3, 0, 3, BOTH)
        # the exact sampler
        ctx.set_sampler("exact")
        assert run(h, 0, V, cost, r, keep, BOTH) == ESTATE and b"FIXED" in lib.mvs_last_error(h)
        ctx.set_sampler("fixed")
        good("after the exact sampler")
        # a caller's volume that is one cell short: refused for a volume run, not needed by a selection alone
        short = torch.empty(c.D * c.H * c.W - 1, dtype=torch.int32, device="cuda")
        short.fill_(7)
        torch.cuda.synchronize()
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert run(h, 0, V, cost, r, keep, BOTH) == EINVAL and b"caller volume" in lib.mvs_last_error(h)
        assert run(h, 0, V, cost, r, keep, VOLUME) == EINVAL
        ctx.sweep_run_bestk(cost, r, keep, 0, V, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], maps, "fused alone beside a short volume")
        assert (short.cpu() == 7).all(), "a refused call wrote into the caller's volume"
        ctx.sweep_use_volume(0, 0)
        good("after the short volume")


def test_occluder_scene(oracle):
    o = bk.occluder()
    D, r, keep = 48, 2, 2
    ref = bk.occluder_volume(ZNCC, r, D, keep)
    z = oracle.plane_table(D, o.z_lo, o.z_hi)
    with mvs_amd.Context(o.W, o.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*o.views(), D, o.z_lo, o.z_hi)
        ctx.sweep_run_bestk(ZNCC, r, keep, 0, o.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
    _same_cells(got[3], ref, "occluder scene")
    _same_maps(got[:3], bk.maps(oracle, ref, z), "occluder scene")
    bad = np.abs(got[0] - o.truth) > 1.5 * (o.z_hi - o.z_lo) / D
    assert (float(bad.mean()), float(bad[o.edge].mean())) == bk.bad_shares(oracle, ref, D)
