"""mvs_propagate_init / mvs_propagate_run on the device (csrc/propagate.hip), bit-identical to the mirror (tests/propagate_mirror.py,
DESIGN.md section 25) in z, gx, gy, the cells, the cost map and the report throughout: the crafted case through both costs, the radii,
the keeps, slopes, one and two iterations with and without random candidates; frames at the kernel's own edges with holes and dead
depths on the tile seams and where the far neighbours cross them; run(1) twice against run(2); view ranges; every way of staging the
frames; the sources of a start map; the maps into the depth store and the filter; the state the stage must leave alone; every error of
the list; and the coarse-to-fine helpers with propagate= against the same composition of mirrors."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_bestk_cases as bb
import depth_filter_mirror as dm
import mvs_amd
import propagate_cases as pc
import propagate_mirror as pm
import pyramid_cases as pyc
import pyramid_mirror as pym
from test_zncc_gpu import TILE, _device, _noise_views

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
ABSDIFF, ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL
f32 = np.float32
NAMES = ("z", "gx", "gy", "cells", "cost map")


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype.itemsize == 4 and ref.dtype.itemsize == 4, what
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, "%s: %d of %d values differ; first at %s: %r, expected %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def _device_map(ptr, H, W):
    torch.cuda.synchronize()
    return torch.as_tensor(mvs_amd._DeviceArray(ptr, (H, W), "<f4"), device="cuda").cpu().numpy()


def _same_state(ctx, shot, what):
    """z, gx, gy, cells through the fetch, the z and cost maps through their device addresses, and the report"""
    got = ctx.propagate_fetch()
    for g, r, name in zip(got, shot[:4], NAMES):
        _same_bits(g, r, "%s: %s" % (what, name))
    _same_bits(_device_map(ctx.propagate_depth_pointer(), ctx.H, ctx.W), shot[0], what + ": the z map on the device")
    _same_bits(_device_map(ctx.propagate_cost_pointer(), ctx.H, ctx.W), shot[4], what + ": the cost map")
    assert tuple(ctx.propagate_report()) == tuple(shot[5]), what


def test_the_bindings_constants_are_the_mirrors():
    assert (ABSDIFF, ZNCC, KEEP_ALL) == (pm.COST_ABSDIFF, pm.COST_ZNCC, pm.KEEP_ALL) and mvs_amd.MVS_PROPAGATE_SLOPES == 1


def _crafted_context():
    c = pc.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set_main(c.main_cam, c.main_img)          # no plane table: the stage does not need one
    ctx.sweep_set_views(c.side_cams, c.sides)
    return c, ctx, _device(c.prior)


@pytest.mark.parametrize("cost,r", pc.COST_RADII)
def test_crafted_case(cost, r):
    c, ctx, start = _crafted_context()
    with ctx:
        assert ctx.propagate_depth_pointer() == 0 and ctx.propagate_cost_pointer() == 0
        for keep, slopes, nrandom in pc.variants(r):
            what = "%s r = %d keep = %d slopes = %d nrandom = %d" % (pc.NAMES[cost], r, keep, slopes, nrandom)
            shots = pc.crafted_states(cost, r, keep, slopes, nrandom)[1]
            ctx.propagate_init(start.data_ptr(), cost, r, keep, slopes=slopes, max_step=pc.MAX_STEP if slopes else float("inf"))
            _same_state(ctx, shots[0], what + ", init")
            ctx.propagate_run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, shots[1], what + ", one iteration")
            ctx.propagate_run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, shots[2], what + ", two iterations")
            # run(2) at once, from a new init on the same context
            ctx.propagate_init(start.data_ptr(), cost, r, keep, slopes=slopes, max_step=pc.MAX_STEP if slopes else float("inf"))
            ctx.propagate_run(2, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, shots[2], what + ", run(2)")


@pytest.mark.parametrize("cost", (ABSDIFF, ZNCC))
@pytest.mark.parametrize("W,H,r", [(9, 5, 4),                               # a frame smaller than the halo and the far offset's reach
                                   (2 * TILE[0], 2 * TILE[1], 2),           # whole tiles, both seams
                                   (2 * TILE[0], TILE[1], 1),
                                   (TILE[0] + 1, TILE[1] + 1, 3),           # one pixel into the next tile; odd width: both parities per row
                                   (TILE[0] - 1, 2 * TILE[1] - 1, 4)])
def test_shapes_at_the_kernels_edges(oracle, cost, W, H, r):
    views = _noise_views(W, H, 3, 0x2ACC + W)
    start = pc.seam_start(W, H, 0xBE57 + W)
    state = pm.State(pm.Scene(oracle, *views), start, cost, r, 2, slopes=True, max_step=0.05)
    what = "%d x %d, %s r = %d" % (W, H, pc.NAMES[cost], r)
    assert (~pm.inside(state.z)).sum() >= 2 and (np.abs(state.z) == f32(0.995)).any(), what
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main(views[0], views[1])
        ctx.sweep_set_views(views[2], views[3])
        ctx.propagate_init(_device(start).data_ptr(), cost, r, 2, slopes=True, max_step=0.05)
        _same_state(ctx, pc.snapshot(state), what + ", init")
        for it in range(2):
            state.run(1, 0.04, 0.01, 2, 11)
            ctx.propagate_run(1, 0.04, 0.01, 2, 11)
            _same_state(ctx, pc.snapshot(state), what + ", iteration %d" % it)
        assert state.report()[2] > 0 or W < 10, what + ": a far neighbour won somewhere"
        for _, h, rows, cols, _ in state.wins:          # both column parities are active in every half, whatever the width
            assert ((rows + cols + h) % 2 == 0).all() and {int(x) % 2 for x in cols} == {0, 1}


@pytest.mark.parametrize("cost,r", [(ABSDIFF, 1), (ZNCC, 2)])
def test_view_ranges(cost, r):
    c, ctx, start = _crafted_context()
    with ctx:
        for first, count in ((1, 3), (0, 2), (2, 1), (4, 1)):
            what = "%s r = %d, views [%d, %d)" % (pc.NAMES[cost], r, first, first + count)
            shots = pc.crafted_states(cost, r, 2, False, 2, first, count)[1]
            ctx.propagate_init(start.data_ptr(), cost, r, 2, first, count)
            _same_state(ctx, shots[0], what + ", init")
            ctx.propagate_run(2, pc.DZ, pc.DG, 2, pc.SEED)
            _same_state(ctx, shots[2], what + ", run(2)")
        ctx.propagate_init(start.data_ptr(), cost, r, 2, 2, 0)              # no view: nothing is counted anywhere
        ctx.propagate_run(1, pc.DZ, pc.DG, 2, pc.SEED)
        z, gx, gy, cells = ctx.propagate_fetch()
        ref = pm.seed_maps(c.prior)
        _same_bits(z, ref[0], "no view: z")
        assert not cells.any() and not gx.any() and not gy.any() and ctx.propagate_report() == [c.W * c.H, 0, 0, 0, 0]
        assert np.isinf(_device_map(ctx.propagate_cost_pointer(), c.H, c.W)).all()


def test_staged_state():
    c = pc.crafted()
    cost, r, keep = ZNCC, 2, 2
    shots = pc.crafted_states(cost, r, keep, True, 2)[1]
    start = _device(c.prior)
    # the _device setters
    main_t, side_t = _device(c.main_img), [_device(s) for s in c.sides]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main_device(c.main_cam, main_t.data_ptr())
        ctx.sweep_set_views_device(c.side_cams, [t.data_ptr() for t in side_t])
        ctx.propagate_init(start.data_ptr(), cost, r, keep, slopes=True, max_step=pc.MAX_STEP)
        ctx.propagate_run(2, pc.DZ, pc.DG, 2, pc.SEED)
        _same_state(ctx, shots[2], "device setters")
    # the slots left staged by mvs_sweep_handles
    slots = [4, 0, 3, 1]
    part = pc.crafted_states(cost, r, keep, False, 2, 0, 3)[1]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.frame_store(6)
        ctx.frame_upload(slots[0], c.main_img)
        for v in range(3):
            ctx.frame_upload(slots[1 + v], c.sides[v])
        ctx.sweep_handles(slots[0], c.main_cam, slots[1:], c.side_cams[:3], 8)      # leaves the slots staged
        ctx.propagate_init(start.data_ptr(), cost, r, keep, 0, 3)
        _same_state(ctx, part[0], "frame store, init")
        ctx.propagate_run(2, pc.DZ, pc.DG, 2, pc.SEED)
        _same_state(ctx, part[2], "frame store, run(2)")


def test_the_sources_of_a_start_map_and_the_readers_of_the_result(oracle):
    """the context's own depth map after a refined sweep, the band's resolved map, the filtered map and the stage's own z map as the
    start; the z and cost maps into the depth store and the filter; and the sweep, band and filter results as they were before"""
    W, H, DC, DB, r = 96, 64, 8, 4, 2
    views, _ = bb.exposure_views(W, H)
    scene = pm.Scene(oracle, *views)
    step = 2.0 / DC
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1)
        coarse = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=dict(cost="zncc", radius=r), filter=dict(radius=2, tau=40, max_steps=4.0))
        # now: the band's maps (offsets) at sweep_result_pointers, the resolved map, the filtered map
        sweep_before = ctx.sweep_fetch(want_volume=True)
        band_before = _device_map(ctx.sweep_band_pointers()[0], H, W), _device_map(ctx.sweep_band_pointers()[1], H, W), ctx.sweep_band_report()
        filtered_before = _device_map(ctx.depth_filtered_pointer(), H, W)
        _same_bits(filtered_before, coarse, "the helper's result is the filtered map")
        for name, ptr, ref in (("the band's resolved map", ctx.sweep_band_pointers()[0], band_before[0]), ("the filtered map", ctx.depth_filtered_pointer(), filtered_before),
                               ("the band's offsets at mvs_sweep_depth_device", ctx.sweep_result_pointers()[0], sweep_before[0])):
            state = pm.State(scene, ref, ZNCC, r, KEEP_ALL, slopes=True, max_step=step).run(1, 0.5 * step, 0.125 * step, 2, 3)
            ctx.propagate_init(ptr, ZNCC, r, KEEP_ALL, slopes=True, max_step=step)
            ctx.propagate_run(1, 0.5 * step, 0.125 * step, 2, 3)
            _same_state(ctx, pc.snapshot(state), "start = " + name)
        # the stage's own z map as the next start, slopes from it, in place
        again = pm.State(scene, state.z, ABSDIFF, 1, 2, slopes=True, max_step=step).run(1, 0.25 * step, 0.0, 1, 4)
        ctx.propagate_init(ctx.propagate_depth_pointer(), ABSDIFF, 1, 2, slopes=True, max_step=step)
        ctx.propagate_run(1, 0.25 * step, 0.0, 1, 4)
        _same_state(ctx, pc.snapshot(again), "start = the stage's own z map")
        # nothing else moved
        after = ctx.sweep_fetch(want_volume=True)
        for g, b, name in zip(after, sweep_before, ("depth", "cost", "index", "volume")):
            _same_bits(g, b, "the sweep's %s after the propagation" % name)
        _same_bits(_device_map(ctx.sweep_band_pointers()[0], H, W), band_before[0], "the band's resolved map after the propagation")
        _same_bits(_device_map(ctx.sweep_band_pointers()[1], H, W), band_before[1], "the band's prior after the propagation")
        assert ctx.sweep_band_report() == band_before[2]
        _same_bits(_device_map(ctx.depth_filtered_pointer(), H, W), filtered_before, "the filtered map after the propagation")
        _same_bits(ctx.sweep_band_resolve(), band_before[0], "the band still resolves")
        # the z / cost maps into the depth store and the filter, unchanged
        ctx.depth_store(2)
        ctx.depth_upload_device(1, views[0], ctx.propagate_depth_pointer(), ctx.propagate_cost_pointer())
        _same_bits(_device_map(ctx.depth_slot_pointer(1), H, W), again.z, "the z map in a depth slot")
        got = ctx.depth_filter(ctx.propagate_depth_pointer(), radius=2, tau=40, max_step=float(f32(4.0 * step)))
        _same_bits(got, dm.filter(again.z, 2, 40, f32(4.0 * step), views[1]), "the filter on the z map")
        _same_state(ctx, pc.snapshot(again), "the readers left the stage's maps alone")


def test_errors():
    c = pc.crafted()
    cost, r, keep = ZNCC, 2, 2
    shots = pc.crafted_states(cost, r, keep, False, 2)[1]
    start = _device(c.prior)
    sp = C.c_void_p(start.data_ptr())
    inf, nan = float("inf"), float("nan")
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h
        init, run = lib.mvs_propagate_init, lib.mvs_propagate_run   # (ctx, depth, first, count, cost, radius, keep, max_step, flags) / (ctx, iterations, dz, dg, nrandom, seed)
        fp, up, lp = (C.c_float * (c.W * c.H))(), (C.c_uint32 * (c.W * c.H))(), (C.c_longlong * 5)()

        def good(what):
            ctx.propagate_init(start.data_ptr(), cost, r, keep)
            _same_state(ctx, shots[0], what + ": init")
            ctx.propagate_run(1, pc.DZ, pc.DG, 2, pc.SEED)
            _same_state(ctx, shots[1], what + ": run")

        assert init(None, sp, 0, 0, cost, r, keep, inf, 0) == EINVAL and run(None, 1, 0.0, 0.0, 0, 0) == EINVAL
        assert lib.mvs_propagate_fetch(None, fp, fp, fp, up) == EINVAL and lib.mvs_propagate_report(None, lp) == EINVAL
        # nothing staged; then no views
        assert init(h, sp, 0, 0, cost, r, keep, inf, 0) == ESTATE
        ctx.sweep_set_main(c.main_cam, c.main_img)
        assert init(h, sp, 0, 0, cost, r, keep, inf, 0) == ESTATE and b"views" in lib.mvs_last_error(h)
        ctx.sweep_set_views(c.side_cams, c.sides)
        # before init
        assert run(h, 1, 0.1, 0.1, 2, 0) == ESTATE and lib.mvs_propagate_fetch(h, fp, fp, fp, up) == ESTATE and lib.mvs_propagate_report(h, lp) == ESTATE
        assert not lib.mvs_propagate_depth_device(h) and not lib.mvs_propagate_cost_device(h), "a refused call allocates nothing"
        good("after MVS_ESTATE")
        V = c.V
        for args in ((None, 0, V, cost, r, keep, inf, 0),                                                                     # no start map
                     (sp, 0, V, 2, r, keep, inf, 0), (sp, 0, V, -1, r, keep, inf, 0),                                         # unknown cost
                     (sp, 0, V, ZNCC, 0, keep, inf, 0), (sp, 0, V, ZNCC, 5, keep, inf, 0), (sp, 0, V, ABSDIFF, 5, keep, inf, 0), (sp, 0, V, ABSDIFF, -1, keep, inf, 0),
                     (sp, 0, V, cost, r, 9, inf, 0), (sp, 0, V, cost, r, -1, inf, 0),                                         # keep outside 0..8
                     (sp, -1, 2, cost, r, keep, inf, 0), (sp, 0, V + 1, cost, r, keep, inf, 0), (sp, 4, 2, cost, r, keep, inf, 0), (sp, 0, -1, cost, r, keep, inf, 0),
                     (sp, 0, V, cost, r, keep, inf, 2), (sp, 0, V, cost, r, keep, inf, 0x80000001),                           # unknown flags
                     (sp, 0, V, cost, r, keep, -0.5, 1), (sp, 0, V, cost, r, keep, nan, 1)):
            assert init(h, *args) == EINVAL, args
            _same_state(ctx, shots[1], "after EINVAL %s" % (args[1:],))
            good("after EINVAL %s" % (args[1:],))
        for args in ((0, 0.1, 0.1, 2, 0), (-1, 0.1, 0.1, 2, 0), (1, 0.1, 0.1, 5, 0), (1, 0.1, 0.1, -1, 0), (1, -0.1, 0.1, 2, 0), (1, 0.1, -0.1, 2, 0),
                     (1, inf, 0.1, 2, 0), (1, 0.1, inf, 2, 0), (1, nan, 0.1, 2, 0), (1, 0.1, nan, 2, 0)):
            assert run(h, *args) == EINVAL, args
            _same_state(ctx, shots[1], "after EINVAL of run %s" % (args,))
            good("after EINVAL of run %s" % (args,))
        assert lib.mvs_propagate_report(h, None) == EINVAL
        assert lib.mvs_propagate_fetch(h, None, None, None, None) == 0 and lib.mvs_propagate_fetch(h, None, fp, None, up) == 0
        _same_bits(np.frombuffer(up, np.uint32).reshape(c.H, c.W), shots[1][3], "fetch of the cells alone")
        # the exact sampler
        ctx.set_sampler("exact")
        assert init(h, sp, 0, V, cost, r, keep, inf, 0) == ESTATE and b"FIXED" in lib.mvs_last_error(h)
        assert run(h, 1, 0.1, 0.1, 2, 0) == ESTATE
        ctx.set_sampler("fixed")
        good("after the exact sampler")


PROPAGATE = dict(iterations=2, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=9, slopes=True)
FILTER = dict(radius=3, tau=40, max_steps=4.0)


@pytest.mark.parametrize("cost,filter", [(dict(cost="zncc", radius=2), FILTER), (dict(cost="absdiff", radius=1, keep=3), None)])
def test_coarse_to_fine_with_propagate(oracle, cost, filter):
    W, H, DC, DB = 96, 64, 16, 16
    views, _ = bb.exposure_views(W, H)
    kind = ZNCC if cost["cost"] == "zncc" else ABSDIFF
    final = bb.two_levels(oracle, views, DC, DB, kind, cost["radius"], cost.get("keep", KEEP_ALL), filter)[0]
    hb = float(f32(1.5 * 2.0 / DC))
    state = pc.propagated(oracle, views, final, kind, cost["radius"], cost.get("keep", KEEP_ALL), PROPAGATE, 2.0 * hb / DB)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1)
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter, cost=cost, propagate=PROPAGATE)
        _same_bits(got, state.z, "coarse_to_fine(propagate=...)")
        _same_state(ctx, pc.snapshot(state), "coarse_to_fine(propagate=...)")
        assert mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter, cost=cost, propagate=PROPAGATE, fetch=False) is None
        _same_bits(_device_map(ctx.propagate_depth_pointer(), H, W), state.z, "fetch=False: the result stays on the device")
        # propagate=None issues today's calls
        _same_bits(mvs_amd.coarse_to_fine(ctx, DC, DB, filter=filter, cost=cost, propagate=None), final, "propagate=None")
        _same_state(ctx, pc.snapshot(state), "propagate=None leaves the stage alone")
        with pytest.raises(ValueError, match="unknown keys"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(iteration=2))
        with pytest.raises(ValueError, match="needs cost"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, propagate=PROPAGATE)


def test_pyramid_coarse_to_fine_with_propagate(oracle):
    W, H, DC, DB, r, tau = 96, 64, 16, 16, 2, 30
    import band_bestk_mirror as bbm
    views, _ = bb.exposure_views(W, H)
    main_cam, main_img, side_cams, sides = views
    lv = pyc.levels(main_img, sides, 2)
    below = bb.global_level(oracle, (main_cam, lv[1][0], side_cams, lv[1][1]), DC, -1.0, 1.0, ZNCC, r, KEEP_ALL)[1]
    prior = pym.prior(below, tau, lv[1][0], lv[0][0])
    hb = float(f32(1.5 * 2.0 / DC))
    resolved = bbm.level(oracle, ZNCC, *views, prior, oracle.plane_table(DB, -hb, hb), r, KEEP_ALL)[0]
    state = pc.propagated(oracle, views, resolved, ZNCC, r, KEEP_ALL, PROPAGATE, 2.0 * hb / DB)
    fine, half = mvs_amd.Context(W, H, 0, sampler="fixed"), mvs_amd.Context(W // 2, H // 2, 0, sampler="fixed")
    with fine, half:
        fine.sweep_set(*views, 1)
        got = mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, tau=tau, cost=dict(cost="zncc", radius=r), propagate=PROPAGATE)
        _same_bits(got, state.z, "pyramid_coarse_to_fine(propagate=...)")
        _same_state(fine, pc.snapshot(state), "pyramid_coarse_to_fine(propagate=...)")
        assert half.propagate_depth_pointer() == 0, "the coarse level never calls the stage and allocates nothing for it"
        _same_bits(mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, tau=tau, cost=dict(cost="zncc", radius=r), propagate=None), resolved, "propagate=None")
