"""The geometric term of the propagation (mvs_propagate_set_consistency, csrc/propagate.hip) on the device, bit-identical to the mirror
(tests/consistency_mirror.py) in z, gx, gy, the cells, the cost map, the report and the support map after init and
after run: the crafted 70 x 19 case (every clause of rule 5 on both sides of the tile seams) through both costs, the radii and the list
sizes, with and without the guide gate; the identities (no neighbours, weight 0, a setter between init and run, run(1) twice against
run(2)); neighbour maps that a sweep left on the device; every error of the list; what a context that never calls the setter allocates;
and the wrappers against the same composition of mirrors.  The mirror takes the matrices mvs_depth_slot_matrices returns; the main
camera's are those of a spare slot stored with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_bestk_cases as bb
import consistency_cases as cc
import consistency_mirror as cm
import gated_cases as gc
import mvs_amd
import propagate_cases as pc
import propagate_mirror as pm
from mvs_amd import synth
from test_propagate_gpu import _device_map, _same_bits, _same_state
from test_zncc_gpu import _device

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
ABSDIFF, ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL
f32 = np.float32
SPARE = cc.NSLOT                     # the slot that holds the main camera, for its matrices


def _support(ctx):
    torch.cuda.synchronize()
    on_device = torch.as_tensor(mvs_amd._DeviceArray(ctx.propagate_support_pointer(), (ctx.H, ctx.W), "|u1"), device="cuda").cpu().numpy()
    got = ctx.propagate_support()
    assert got.dtype == np.uint8 and np.array_equal(got, on_device)
    return got


def _same(ctx, shot, what):
    _same_state(ctx, shot, what)
    got = _support(ctx)
    bad = np.argwhere(got != shot[6])
    assert len(bad) == 0, "%s: support: %d pixels differ; first at %s: %d, expected %d" % (what, len(bad), bad[0], got[tuple(bad[0])], shot[6][tuple(bad[0])])


def _context():
    """the crafted case staged, its six slots stored (slot 5 with a cost map, the others without), the main camera in the spare slot"""
    c = cc.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set_main(c.main_cam, c.main_img)
    ctx.sweep_set_views(c.side_cams, c.sides)
    ctx.depth_store(cc.NSLOT + 1)
    for s in range(cc.NSLOT):
        ctx.depth_upload(s, c.cams[s], c.maps[s], np.zeros((c.H, c.W), f32) if s == 5 else None)
    ctx.depth_upload(SPARE, c.main_cam, c.start)
    return c, ctx, _device(c.start)


def _mats(ctx):
    """what the mirror needs of the library: slot -> (P, P^-1, centre), and the main camera's (M, M^-1)"""
    return {s: ctx.depth_slot_matrices(s) for s in range(cc.NSLOT)}, ctx.depth_slot_matrices(SPARE)


def _shots(ctx, cost, r, keep, gate=None, **kw):
    mats, main = _mats(ctx)
    return cc.shots(cost, r, keep, gate, mats, main, key="library", **kw)


def test_the_librarys_matrices_are_the_mirrors_up_to_the_last_bit():
    c, ctx, _ = _context()
    with ctx:
        mats, main = _mats(ctx)
        for s in range(cc.NSLOT):
            P, Pi, _ = cm.fm.slot_matrices(c.cams[s])
            assert np.array_equal(mats[s][0], P.astype(f32)) and np.allclose(mats[s][1], Pi, rtol=1e-6, atol=1e-9)
        assert np.array_equal(main[0], np.asarray(c.main_cam, f32).reshape(4, 4))


@pytest.mark.parametrize("gate", (None, "crafted"))
@pytest.mark.parametrize("cost,r", cc.COST_RADII)
def test_crafted_case(cost, r, gate):
    c, ctx, start = _context()
    guide = _device(gc.crafted_guide())
    with ctx:
        assert ctx.propagate_support_pointer() == 0
        if gate:
            ctx.propagate_set_gate(gc.TAU, guide.data_ptr())
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        for keep in cc.KEEPS + ((8,) if (cost, r) == (ZNCC, 1) else ()):
            what = "%s r = %d keep = %d gate = %s" % (cc.NAMES[cost], r, keep, gate)
            shots = _shots(ctx, cost, r, keep, gate)
            ctx.propagate_init(start.data_ptr(), cost, r, keep)
            _same(ctx, shots[0], what + ", init")
            ctx.propagate_run(2, cc.DZ, cc.DG, 2, cc.SEED)
            _same(ctx, shots[2], what + ", run(2)")
            assert shots[2][6].max() >= 6 and (shots[2][6] < 3).any() and (shots[2][3] != _shots(ctx, cost, r, keep, gate, slots=())[2][3]).any(), what


def test_identities():
    c, ctx, start = _context()
    cost, r, keep = ZNCC, 2, 2
    with ctx:
        on, zero, off = _shots(ctx, cost, r, keep), _shots(ctx, cost, r, keep, weight=0.0), _shots(ctx, cost, r, keep, slots=())
        # a context that never called the setter
        never = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
        with never:
            never.sweep_set_main(c.main_cam, c.main_img)
            never.sweep_set_views(c.side_cams, c.sides)
            never.propagate_init(start.data_ptr(), cost, r, keep)
            never.propagate_run(2, cc.DZ, cc.DG, 2, cc.SEED)
            untouched = never.propagate_fetch() + (_device_map(never.propagate_cost_pointer(), c.H, c.W), tuple(never.propagate_report()), _support(never))
        # nslots = 0 after a run with the term: the bytes of the context that never set it
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        ctx.propagate_run(1, cc.DZ, cc.DG, 2, cc.SEED)
        _same(ctx, on[1], "the term, one iteration")
        ctx.propagate_set_consistency(())
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        ctx.propagate_run(2, cc.DZ, cc.DG, 2, cc.SEED)
        _same(ctx, untouched, "nslots = 0 against a context that never called the setter")
        _same(ctx, off[2], "nslots = 0 against the mirror")
        # weight 0: the support map only
        ctx.propagate_set_consistency(cc.SLOTS, 0.0, cc.MAX_PX)
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        _same(ctx, zero[0], "weight 0, init")
        ctx.propagate_run(2, cc.DZ, cc.DG, 2, cc.SEED)
        _same(ctx, zero[2], "weight 0, run(2)")
        _same_state(ctx, off[2], "weight 0 against nslots = 0")
        assert _support(ctx).any()
        # a setter between init and run changes nothing until the next init; run(1) then run(1) is run(2)
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        _same(ctx, on[0], "the term, init")
        ctx.propagate_set_consistency(())
        ctx.propagate_run(1, cc.DZ, cc.DG, 2, cc.SEED)
        _same(ctx, on[1], "set_consistency(()) between init and run")
        ctx.propagate_set_consistency((0, 1), 9.0, 2.5)
        ctx.propagate_run(1, cc.DZ, cc.DG, 2, cc.SEED)
        _same(ctx, on[2], "another term recorded, the runs still use the init's; run(1) twice")
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        ctx.propagate_run(2, cc.DZ, cc.DG, 2, cc.SEED)
        _same(ctx, on[2], "run(2) at once")


def test_neighbour_maps_left_on_the_device_by_a_sweep(oracle):
    """96 x 64, the synthetic four-view scene: each side view swept as a main view, its refined map stored device to device"""
    W, H, D, r, keep = 96, 64, 16, 1, 2
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, 4)
    cams, imgs = [main_cam] + list(side_cams), [main_img] + list(sides)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.depth_store(6)
        maps = []
        for v in range(1, 5):
            others = [i for i in range(5) if i != v]
            ctx.sweep_set(cams[v], imgs[v], np.stack([cams[i] for i in others]), [imgs[i] for i in others], D)
            ctx.sweep_run_bestk(ZNCC, r, keep, 0, None, BOTH)
            ctx.sweep_refine_depth()
            ctx.depth_upload_device(v - 1, cams[v], *ctx.sweep_result_pointers()[:2])
            maps.append(ctx.sweep_fetch()[0])
            _same_bits(_device_map(ctx.depth_slot_pointer(v - 1), H, W), maps[-1], "slot %d" % (v - 1))
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run_bestk(ZNCC, r, keep, 0, None, BOTH)
        ctx.sweep_refine_depth()
        start = ctx.sweep_fetch()[0]
        ctx.depth_upload_device(5, main_cam, ctx.sweep_result_pointers()[0])
        mats = {s: ctx.depth_slot_matrices(s) for s in (0, 1, 2, 3, 5)}      # (slot 4 stays empty)
        term = cm.Term(mats[5], [(mats[s][0], mats[s][1], maps[s]) for s in (0, 1, 2, 3)], 6.0, 2.0)
        state = cm.State(pm.Scene(oracle, main_cam, main_img, side_cams, sides), start, ZNCC, r, keep, slopes=True, term=term)
        ctx.propagate_set_consistency((0, 1, 2, 3), 6.0, 2.0)
        ctx.propagate_init(ctx.sweep_result_pointers()[0], ZNCC, r, keep, slopes=True)
        _same(ctx, cc.snapshot(state), "init")
        state.run(1, 0.02, 0.005, 2, 5)
        ctx.propagate_run(1, 0.02, 0.005, 2, 5)
        _same(ctx, cc.snapshot(state), "one iteration")
        assert (state.support() == 4).any() and (state.support() < 4).any()


def test_errors():
    c, ctx, start = _context()
    cost, r, keep = ZNCC, 1, 2
    inf, nan = float("inf"), float("nan")
    with ctx:
        lib, h = ctx.lib, ctx.h
        setter, init, run = lib.mvs_propagate_set_consistency, lib.mvs_propagate_init, lib.mvs_propagate_run
        sp = C.c_void_p(start.data_ptr())
        slots = (C.c_int * 8)(*cc.SLOTS)
        on = _shots(ctx, cost, r, keep)

        def good(what):
            ctx.propagate_init(start.data_ptr(), cost, r, keep)
            _same(ctx, on[0], what + ": init")
            ctx.propagate_run(1, cc.DZ, cc.DG, 2, cc.SEED)
            _same(ctx, on[1], what + ": run")

        assert lib.mvs_propagate_support_fetch(None, None) == EINVAL and not lib.mvs_propagate_support_device(None)
        assert lib.mvs_propagate_support_fetch(h, (C.c_uint8 * (c.W * c.H))()) == ESTATE and not lib.mvs_propagate_support_device(h)
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        good("the crafted term")
        assert lib.mvs_propagate_support_fetch(h, None) == EINVAL
        # the setter: nothing is recorded by a refused call, so the next init still takes the crafted term
        inside, too_much = 1307.0, 1310.0               # with max_px 3: floorf(3 * w * 255) = 999 855 and 1 002 150 around rule 7's 1 000 000
        assert setter(None, 0, None, 0.0, 1.0) == EINVAL
        for args in ((-1, slots, 1.0, 1.0), (9, slots, 1.0, 1.0), (3, None, 1.0, 1.0), (8, (C.c_int * 8)(0, 1, -1, 3, 4, 5, 0, 2), 1.0, 1.0),
                     (8, slots, -0.5, 1.0), (8, slots, inf, 1.0), (8, slots, nan, 1.0), (8, slots, 1.0, 0.0), (8, slots, 1.0, -1.0), (8, slots, 1.0, inf),
                     (8, slots, 1.0, nan), (8, slots, too_much, 3.0)):
            assert setter(h, *args) == EINVAL, args
            _same(ctx, on[1], "after EINVAL of the setter %s" % (args[::3],))
            good("after EINVAL of the setter %s" % (args[::3],))
        assert setter(h, 8, slots, inside, 3.0) == 0, "just inside rule 7's bound"
        assert setter(h, 0, None, nan, nan) == 0, "nslots = 0: the other arguments are not read"
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        # init: a slot outside the store, an unfilled slot, no store at all, a singular main camera, too many views under MVS_KEEP_ALL
        ctx.propagate_set_consistency((0, cc.NSLOT + 1), cc.WEIGHT, cc.MAX_PX)
        assert init(h, sp, 0, cc.V, cost, r, keep, inf, 0) == ESTATE and b"outside" in lib.mvs_last_error(h)
        _same(ctx, on[1], "after a slot outside the store")
        fresh = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
        with fresh:
            fresh.sweep_set_main(c.main_cam, c.main_img)
            fresh.sweep_set_views(c.side_cams, c.sides)
            fresh.propagate_set_consistency((0,), cc.WEIGHT, cc.MAX_PX)
            assert fresh.lib.mvs_propagate_init(fresh.h, sp, 0, cc.V, cost, r, keep, inf, 0) == ESTATE and b"no depth store" in fresh.lib.mvs_last_error(fresh.h)
            fresh.depth_store(2)
            fresh.depth_upload(1, c.cams[0], c.maps[0])
            assert fresh.lib.mvs_propagate_init(fresh.h, sp, 0, cc.V, cost, r, keep, inf, 0) == ESTATE and b"holds no depth map" in fresh.lib.mvs_last_error(fresh.h)
            assert fresh.propagate_depth_pointer() == 0 and fresh.propagate_support_pointer() == 0, "a refused init allocates nothing"
            singular = np.array(c.main_cam, f32).reshape(4, 4).copy()
            singular[3] = 0.0
            fresh.sweep_set_main(singular, c.main_img)
            fresh.sweep_set_views(c.side_cams, c.sides)
            fresh.propagate_set_consistency((1,), cc.WEIGHT, cc.MAX_PX)
            assert fresh.lib.mvs_propagate_init(fresh.h, sp, 0, cc.V, cost, r, keep, inf, 0) == EINVAL and b"singular" in fresh.lib.mvs_last_error(fresh.h)
            assert fresh.propagate_depth_pointer() == 0
            fresh.sweep_set_main(c.main_cam, c.main_img)
            fresh.sweep_set_views(c.side_cams, c.sides)
            fresh.propagate_init(start.data_ptr(), cost, r, keep)      # usable
            assert fresh.propagate_depth_pointer() != 0 and fresh.propagate_support().max() <= 1
        ctx.propagate_set_consistency(cc.SLOTS, inside, 3.0)
        wide = np.concatenate([c.side_cams] * 6)
        ctx.sweep_set_views(wide, c.sides * 6)
        assert init(h, sp, 0, 18, cost, r, KEEP_ALL, inf, 0) == EINVAL and b"24-bit" in lib.mvs_last_error(h)
        assert init(h, sp, 0, 18, cost, r, 8, inf, 0) == 0, "keep <= 8 always fits"
        ctx.sweep_set_views(c.side_cams, c.sides)
        ctx.propagate_set_consistency(cc.SLOTS, cc.WEIGHT, cc.MAX_PX)
        good("after the refusals of init")
        # run: a listed slot no longer filled, the store re-sized
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        before = ctx.propagate_fetch() + (_device_map(ctx.propagate_cost_pointer(), c.H, c.W), tuple(ctx.propagate_report()), _support(ctx))
        ctx.depth_store(cc.NSLOT + 1)                                   # the same capacity: every slot is empty again
        assert run(h, 1, cc.DZ, cc.DG, 2, cc.SEED) == ESTATE and b"holds no depth map" in lib.mvs_last_error(h)
        ctx.depth_store(cc.NSLOT + 3)
        assert run(h, 1, cc.DZ, cc.DG, 2, cc.SEED) == ESTATE and b"re-sized" in lib.mvs_last_error(h)
        _same(ctx, before, "after the refusals of run")
        assert init(h, sp, 0, cc.V, cost, r, keep, inf, 0) == ESTATE
        for s in range(cc.NSLOT):
            ctx.depth_upload(s, c.cams[s], c.maps[s])
        good("the store filled again")


def test_a_context_that_never_sets_the_term_allocates_nothing_new():
    c = cc.crafted()
    start = _device(c.start)
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main(c.main_cam, c.main_img)
        ctx.sweep_set_views(c.side_cams, c.sides)
        assert ctx.propagate_support_pointer() == 0 and ctx.depth_slot_pointer(0) == 0
        ctx.propagate_init(start.data_ptr(), ZNCC, 1, 2)
        P = c.W * c.H
        # the support map is part of the stage's one allocation: behind the five maps and the guide bytes
        assert ctx.propagate_support_pointer() == ctx.propagate_depth_pointer() + 5 * 4 * P + P == ctx.propagate_cost_pointer() + 4 * P + P
        assert not _support(ctx).any() and ctx.depth_slot_pointer(0) == 0, "no depth store was made"
        ctx.propagate_run(1, cc.DZ, cc.DG, 2, cc.SEED)
        assert not _support(ctx).any()


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------
PROPAGATE = dict(iterations=1, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=9, slopes=True)
TERM = dict(weight=5.0, max_px=2.0)


def _run(state, propagate, step):
    return state.run(int(propagate["iterations"]), float(f32(float(propagate["dz_steps"]) * step)), float(f32(float(propagate["dg_steps"]) * step)),
                     int(propagate["nrandom"]), int(propagate["seed"]))


def test_coarse_to_fine_with_the_term(oracle):
    W, H, DC, DB, r, keep = 48, 32, 8, 8, 1, 2
    views, truth = bb.exposure_views(W, H, 2)
    main_cam, main_img, side_cams, sides = views
    cost = dict(cost="zncc", radius=r, keep=keep)
    final = bb.two_levels(oracle, views, DC, DB, ZNCC, r, keep, None)[0]
    hb = float(f32(1.5 * 2.0 / DC))
    sc = synth.Scene(synth.SEED_SCENE, W / 1920.0)
    centers = [[0.15 * np.cos(np.pi * v), 0.15 * np.sin(np.pi * v), 0.0] for v in range(2)]
    maps = [sc.render(ctr, W, H, want_depth=True)[1] for ctr in centers]
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1)
        ctx.depth_store(3)
        for v in range(2):
            ctx.depth_upload(v, side_cams[v], maps[v])
        ctx.depth_upload(2, main_cam, truth)
        mats = [ctx.depth_slot_matrices(s) for s in range(3)]
        term = cm.Term(mats[2], [(mats[s][0], mats[s][1], maps[s]) for s in (0, 1)], **TERM)
        state = _run(cm.State(pm.Scene(oracle, *views), final, ZNCC, r, keep, slopes=True, term=term), PROPAGATE, 2.0 * hb / DB)
        plain = _run(pm.State(pm.Scene(oracle, *views), final, ZNCC, r, keep, slopes=True), PROPAGATE, 2.0 * hb / DB)
        assert (state.cells != plain.cells).any()
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(PROPAGATE, consistency=dict(TERM, slots=(0, 1))))
        _same_bits(got, state.z, "coarse_to_fine(propagate=dict(..., consistency=...))")
        _same(ctx, cc.snapshot(state), "coarse_to_fine(propagate=dict(..., consistency=...))")
        # the term is off afterwards: without the key, today's calls and today's result
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=PROPAGATE)
        _same_bits(got, plain.z, "coarse_to_fine(propagate=...) after one with the term")
        _same_state(ctx, pc.snapshot(plain), "coarse_to_fine(propagate=...) after one with the term")
        assert not _support(ctx).any()
        with pytest.raises(ValueError, match="unknown keys"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(PROPAGATE, consistency=dict(TERM, slots=(0,), cap=3)))
        with pytest.raises(mvs_amd.MvsError, match="max_px"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(PROPAGATE, consistency=dict(slots=(0,), weight=1.0, max_px=0.0)))
        _same_bits(mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=PROPAGATE), plain.z, "after a refused term the term is off")


def test_propagate_two_stage(oracle):
    W, H, D, r, keep, n = 48, 32, 8, 1, 2, 3
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, 2)
    cams, imgs = [main_cam] + list(side_cams), [main_img] + list(sides)
    cost = dict(cost="zncc", radius=r, keep=keep)
    frame_slots = [4, 1, 3]                                            # where the three frames sit in the frame store
    side_slots = [[frame_slots[j] for j in range(n) if j != i] for i in range(n)]
    side_cams_of = [np.stack([cams[j] for j in range(n) if j != i]) for i in range(n)]
    step = 2.0 / D
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.frame_store(5)
        for i in range(n):
            ctx.frame_upload(frame_slots[i], imgs[i])
        ctx.depth_store(2 * n)
        got = mvs_amd.propagate_two_stage(ctx, frame_slots, np.stack(cams), side_slots, np.stack(side_cams_of), D, cost=cost, propagate=PROPAGATE, consistency=TERM)
        mats = [ctx.depth_slot_matrices(i) for i in range(2 * n)]
        scenes = [pm.Scene(oracle, cams[i], imgs[i], side_cams_of[i], [imgs[j] for j in range(n) if j != i]) for i in range(n)]
        first = []
        for i in range(n):
            views = (cams[i], imgs[i], side_cams_of[i], [imgs[j] for j in range(n) if j != i])
            start = bb.global_level(oracle, views, D, -1.0, 1.0, ZNCC, r, keep)[1]
            first.append(_run(pm.State(scenes[i], start, ZNCC, r, keep, slopes=True), PROPAGATE, step))
            _same_bits(_device_map(ctx.depth_slot_pointer(i), H, W), first[i].z, "stage 1, frame %d" % i)
        for i in range(n):
            assert np.array_equal(mats[i][0], mats[n + i][0]) and np.array_equal(mats[i][1], mats[n + i][1])
            term = cm.Term(mats[i], [(mats[j][0], mats[j][1], first[j].z) for j in range(n) if j != i], **TERM)
            second = _run(cm.State(scenes[i], first[i].z, ZNCC, r, keep, slopes=True, term=term), PROPAGATE, step)
            _same_bits(got[i], second.z, "stage 2, frame %d" % i)
            _same_bits(_device_map(ctx.depth_slot_pointer(n + i), H, W), second.z, "stage 2, frame %d, in its slot" % i)
            assert (second.cells != _run(pm.State(scenes[i], first[i].z, ZNCC, r, keep, slopes=True), PROPAGATE, step).cells).any()
        _same(ctx, cc.snapshot(second), "the stage holds the last frame's second stage")
        # the term is off again
        ctx.propagate_init(ctx.depth_slot_pointer(0), ZNCC, r, keep)
        assert not _support(ctx).any()
        with pytest.raises(ValueError, match="unknown keys"):
            mvs_amd.propagate_two_stage(ctx, frame_slots, np.stack(cams), side_slots, np.stack(side_cams_of), D, cost=cost, propagate=PROPAGATE, consistency=dict(TERM, slots=(0,)))
        with pytest.raises(ValueError, match="needs cost"):
            mvs_amd.propagate_two_stage(ctx, frame_slots, np.stack(cams), side_slots, np.stack(side_cams_of), D, propagate=PROPAGATE, consistency=TERM)
