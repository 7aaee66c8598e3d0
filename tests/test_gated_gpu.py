"""mvs_sweep_run_bestk_gated (csrc/bestk_gated.hip) and the gate of the propagation (mvs_propagate_set_gate, csrc/propagate.hip) on the
device, bit-identical to the mirror (tests/gated_mirror.py) throughout: the crafted guide on section 22's crafted
case through every combination of outputs, both costs, the radii, the keeps and the taus; the identities against mvs_sweep_run_bestk on
the same context; frames at the kernel's own edges with a guide border on the tile seams and in the last column and row; view ranges;
every way of staging the frames; the readers behind the volume; the state it leaves; every error of both lists; the gated propagation
through init, one, two and two-at-once iterations; the helpers' tau key; and the contrast scene."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_bestk_cases as bb
import bestk_cases as bk
import clean_mirror as cm
import gated_cases as gc
import gated_mirror as gm
import mvs_amd
import propagate_cases as pc
import propagate_mirror as pm
import pyramid_cases as pyc
import pyramid_mirror as pym
import window_mirror as wm
from test_propagate_gpu import _same_bits, _same_state
from test_zncc_gpu import TILE, _device, _noise_views, _same_cells, _same_maps

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
VOLUME, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOLUME | FUSED
ABSDIFF, ZNCC, KEEP_ALL, TAU = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL, gc.TAU
f32 = np.float32


def _crafted_context():
    c = gc.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set(*c.views(), c.D, c.Z_LO, c.Z_HI)
    return c, ctx


@pytest.mark.parametrize("cost,r", gc.COST_RADII)
def test_crafted_case(oracle, cost, r):
    c, ctx = _crafted_context()
    z = c.planes(oracle)
    crafted = _device(gc.crafted_guide())
    guides = {"main": 0, "crafted": crafted.data_ptr()}
    with ctx:
        for name, ptr in guides.items():
            for tau in gc.TAUS:
                for keep in gc.KEEPS:
                    what = "%s r = %d keep = %d tau = %d guide = %s: " % (gc.NAMES[cost], r, keep, tau, name)
                    ref = gc.crafted_volume(cost, r, keep, tau, name)
                    maps = gc.maps(oracle, ref, z)
                    ctx.sweep_run_bestk_gated(cost, r, keep, tau, ptr, 0, c.V, BOTH)
                    got = ctx.sweep_fetch(want_volume=True)
                    _same_cells(got[3], ref, what + "volume | fused")
                    _same_maps(got[:3], maps, what + "volume | fused")
                    # the volume alone, then the two-step selection and the refinement
                    ctx.sweep_run_bestk_gated(cost, r, keep, tau, ptr, 0, 1, BOTH)        # (other cells and maps in between)
                    ctx.sweep_run_bestk_gated(cost, r, keep, tau, ptr, 0, c.V, VOLUME)
                    _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, what + "volume alone")
                    ctx.sweep_argmin()
                    _same_maps(ctx.sweep_fetch()[:3], maps, what + "volume, then mvs_sweep_argmin")
                    ctx.sweep_refine_depth()
                    _same_maps(ctx.sweep_fetch()[:3], gc.maps(oracle, ref, z, refine=True), what + "refined")
    # the selection alone, on a context that never had a volume
    for keep in gc.KEEPS:
        c, ctx = _crafted_context()
        with ctx:
            ctx.sweep_run_bestk_gated(cost, r, keep, TAU, guides["crafted"], 0, c.V, FUSED)
            _same_maps(ctx.sweep_fetch()[:3], gc.maps(oracle, gc.crafted_volume(cost, r, keep, TAU), z), "%s r = %d keep = %d: fused alone" % (gc.NAMES[cost], r, keep))


def test_identities_against_the_ungated_entry():
    c, ctx = _crafted_context()
    crafted, constant = _device(gc.crafted_guide()), _device(gc.constant_guide())
    with ctx:
        for cost in (ABSDIFF, ZNCC):
            for r in (1, 2, 3, 4):
                for keep in (KEEP_ALL, 2, 8):
                    ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
                    ungated = ctx.sweep_fetch(want_volume=True)
                    for what, tau, ptr in (("tau 255, the main image", 255, 0), ("tau 255, the crafted guide", 255, crafted.data_ptr()),
                                           ("tau 0, a constant guide", 0, constant.data_ptr()), ("the crafted tau, a constant guide", TAU, constant.data_ptr())):
                        ctx.sweep_run_bestk_gated(cost, r, keep, tau, ptr, 0, 1, BOTH)    # (other cells and maps in between)
                        ctx.sweep_run_bestk_gated(cost, r, keep, tau, ptr, 0, c.V, BOTH)
                        got = ctx.sweep_fetch(want_volume=True)
                        _same_cells(got[3], ungated[3], "%s r = %d keep = %d, %s" % (gc.NAMES[cost], r, keep, what))
                        _same_maps(got[:3], ungated[:3], "%s r = %d keep = %d, %s" % (gc.NAMES[cost], r, keep, what))
        ctx.sweep_run_zncc(2, 0, c.V, VOLUME)
        summed = ctx.sweep_fetch(want_volume=True)[3]
        ctx.sweep_run_bestk_gated(ZNCC, 2, KEEP_ALL, 255, 0, 0, c.V, VOLUME)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], summed, "MVS_KEEP_ALL with ZNCC at tau 255 against mvs_sweep_run_zncc")


def _edge_guide(W, H):
    """blocks with a border on every tile seam of the frame, in the last column and row, and inside the first tile"""
    rows = sorted({0, H // 3} | set(range(TILE[1], H, TILE[1])) | {H - 1})
    cols = sorted({0, W // 3} | set(range(TILE[0], W, TILE[0])) | {W - 1})
    g = gc.block_guide(W, H, rows, cols, ((H // 2, W // 2),))
    assert (g[:, W - 2] != g[:, W - 1]).all() and (g[H - 2] != g[H - 1]).all()
    assert W <= TILE[0] or (g[:, TILE[0] - 1] != g[:, TILE[0]]).all()
    assert H <= TILE[1] or (g[TILE[1] - 1] != g[TILE[1]]).all()
    return g


SHAPES = [(9, 5, 3, 4),                                   # smaller than the window in both directions
          (2 * TILE[0], 2 * TILE[1], 3, 2),               # whole tiles; a chunk and one plane
          (2 * TILE[0], TILE[1], 1, 1),                   # one plane
          (TILE[0] + 1, TILE[1] + 1, 2, 3),               # one pixel into the next tile; whole chunks
          (TILE[0] - 1, 2 * TILE[1] - 1, 3, 4)]


@pytest.mark.parametrize("cost", (ABSDIFF, ZNCC))
@pytest.mark.parametrize("W,H,D,r", SHAPES)
def test_shapes_at_the_kernels_edges(oracle, cost, W, H, D, r):
    views = _noise_views(W, H, 3, 0x6A7E + W)
    guide = _edge_guide(W, H)
    z = oracle.plane_table(D, -0.5, 0.7)
    ref = gm.volume(oracle, cost, *views, D, -0.5, 0.7, r, 2, TAU, guide)
    assert (ref >> 24).max() == 2 and (ref == 0).any()
    assert (ref != gm.bm.volume(oracle, cost, *views, D, -0.5, 0.7, r, 2)).any()
    g = _device(guide)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, D, -0.5, 0.7)
        ctx.sweep_run_bestk_gated(cost, r, 2, TAU, g.data_ptr(), 0, 3, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "%d x %d x %d, r = %d" % (W, H, D, r))
        _same_maps(got[:3], gc.maps(oracle, ref, z), "%d x %d x %d, r = %d" % (W, H, D, r))
        # the main image (noise) as the guide: most members are out
        ref = gm.volume(oracle, cost, *views, D, -0.5, 0.7, r, KEEP_ALL, 60)
        ctx.sweep_run_bestk_gated(cost, r, KEEP_ALL, 60, None, 0, 3, VOLUME)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, "%d x %d x %d, r = %d, the noise as the guide" % (W, H, D, r))


@pytest.mark.parametrize("cost,r", ((ABSDIFF, 2), (ZNCC, 1), (ZNCC, 4)))
def test_view_ranges(oracle, cost, r):
    c, ctx = _crafted_context()
    z = c.planes(oracle)
    g = _device(gc.crafted_guide())
    with ctx:
        for first, count in gc.RANGES:
            for keep in (2, 8):
                what = "%s r = %d keep = %d, views [%d, %d)" % (gc.NAMES[cost], r, keep, first, first + count)
                ref = gc.crafted_volume(cost, r, keep, TAU, "crafted", range(first, first + count))
                ctx.sweep_run_bestk_gated(cost, r, keep, TAU, g.data_ptr(), first, count, BOTH)
                got = ctx.sweep_fetch(want_volume=True)
                _same_cells(got[3], ref, what)
                _same_maps(got[:3], gc.maps(oracle, ref, z), what)
        ctx.sweep_run_bestk_gated(cost, r, 2, TAU, g.data_ptr(), 2, 0, BOTH)         # no view: nothing is counted anywhere
        got = ctx.sweep_fetch(want_volume=True)
        assert not got[3].any() and (got[2] == -1).all() and (got[0] == 1.0).all() and np.isinf(got[1]).all()


def test_staged_state(oracle):
    c = gc.crafted()
    cost, r, keep = ZNCC, 2, 2
    g = _device(gc.crafted_guide())
    main_t, side_t = _device(c.main_img), [_device(s) for s in c.sides]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:                   # the _device setters
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        ctx.sweep_set_main_device(c.main_cam, main_t.data_ptr())
        ctx.sweep_set_views_device(c.side_cams, [t.data_ptr() for t in side_t])
        for name, ptr in (("main", None), ("crafted", g.data_ptr())):
            ctx.sweep_run_bestk_gated(cost, r, keep, TAU, ptr, 0, c.V, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], gc.crafted_volume(cost, r, keep, TAU, name), "device setters, guide = " + name)
    slots = [4, 0, 3, 1]                                                        # the slots left staged by mvs_sweep_handles
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.frame_store(6)
        ctx.frame_upload(slots[0], c.main_img)
        for v in range(3):
            ctx.frame_upload(slots[1 + v], c.sides[v])
        ctx.sweep_handles(slots[0], c.main_cam, slots[1:], c.side_cams[:3], 8)
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        for name, ptr in (("main", None), ("crafted", g.data_ptr())):           # (the main image is a slot of the store here)
            ctx.sweep_run_bestk_gated(cost, r, keep, TAU, ptr, 0, 3, VOLUME)
            _same_cells(ctx.sweep_fetch(want_volume=True)[3], gc.crafted_volume(cost, r, keep, TAU, name, (0, 1, 2)), "frame store, guide = " + name)


def test_downstream_readers_and_state(oracle):
    c, ctx = _crafted_context()
    cost, r, keep = ZNCC, 2, 2
    vol = gc.crafted_volume(cost, r, keep, TAU)
    z = c.planes(oracle)
    g = _device(gc.crafted_guide())
    prior = _device(np.zeros((c.H, c.W), np.float32))
    with ctx:
        lib, h = ctx.lib, ctx.h
        ctx.sweep_run_band(prior.data_ptr(), 0, 3, BOTH)
        ctx.sweep_band_resolve()
        ctx.sweep_run_bestk_gated(cost, r, keep, TAU, g.data_ptr(), 0, c.V, BOTH)
        assert lib.mvs_sweep_band_resolve(h) == ESTATE, "a gated run ends the band run's state"
        ctx.sweep_window(1, 255, None, select=True)
        Wv = wm.window(vol, 24, 1)
        _same_cells(ctx.sweep_window_fetch(), Wv, "windowed")
        _same_maps(ctx.sweep_fetch()[:3], gc.maps(oracle, Wv, z), "window select")
        ctx.sweep_argmin()
        before = gc.maps(oracle, vol, z)
        _same_maps(ctx.sweep_fetch()[:3], before, "mvs_sweep_argmin restores the maps")
        ctx.sweep_clean(0, 10, 4, 1)
        cleaned = cm.clean(*before, vol=vol, cs=24, uniqueness=10, speckle_min_size=4, speckle_max_diff=1)
        _same_maps(ctx.sweep_fetch()[:3], cleaned[:3], "cleaned")
        assert ctx.sweep_clean_report() == list(cleaned[3])
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, "the readers left the volume alone")
        ctx.sweep_run_bestk_gated(cost, r, keep, TAU, g.data_ptr(), 0, c.V, VOLUME)
        assert lib.mvs_sweep_refine_depth(h) == ESTATE and lib.mvs_sweep_clean(h, 0, 0, 4, 1, 0) == ESTATE, "no selection on this volume yet"
        ctx.sweep_argmin()
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], gc.maps(oracle, vol, z, refine=True), "argmin, then the refinement")


def test_errors(oracle):
    c = gc.crafted()
    cost, r, keep = ZNCC, 2, 2
    ref = gc.crafted_volume(cost, r, keep, TAU)
    maps = gc.maps(oracle, ref, c.planes(oracle))
    g = _device(gc.crafted_guide())
    gp = C.c_void_p(g.data_ptr())
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h
        run = lib.mvs_sweep_run_bestk_gated            # (ctx, view_first, view_count, cost, radius, keep, tau, guide, flags)

        def good(what):
            ctx.sweep_run_bestk_gated(cost, r, keep, TAU, g.data_ptr(), 0, c.V, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what)
            _same_maps(got[:3], maps, what)

        assert run(None, 0, 0, cost, r, keep, TAU, gp, BOTH) == EINVAL
        # nothing staged: no planes, no main view, no views
        assert run(h, 0, 0, cost, r, keep, TAU, gp, BOTH) == ESTATE
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        assert run(h, 0, 0, cost, r, keep, TAU, gp, BOTH) == ESTATE
        ctx.sweep_set_main(c.main_cam, c.main_img)
        assert run(h, 0, 0, cost, r, keep, TAU, None, BOTH) == ESTATE and b"views" in lib.mvs_last_error(h)
        assert not lib.mvs_sweep_depth_device(h), "a refused call allocates nothing"
        ctx.sweep_set_views(c.side_cams, c.sides)
        good("after MVS_ESTATE")
        # the maps and the volume of another run, which no refused call may touch
        ctx.sweep_run_bestk(ABSDIFF, 1, 3, 0, 3, BOTH)
        other = ctx.sweep_fetch(want_volume=True)
        V = c.V
        for args in ((0, V, 2, r, keep, TAU, gp, BOTH), (0, V, -1, r, keep, TAU, gp, BOTH),                                  # unknown cost
                     (0, V, ZNCC, 0, keep, TAU, gp, BOTH), (0, V, ZNCC, 5, keep, TAU, gp, BOTH), (0, V, ZNCC, -1, keep, TAU, gp, BOTH),
                     (0, V, ABSDIFF, 0, keep, TAU, gp, BOTH), (0, V, ABSDIFF, 5, keep, TAU, gp, BOTH), (0, V, ABSDIFF, -1, keep, TAU, None, BOTH),   # radius outside 1..4
                     (0, V, cost, r, 9, TAU, gp, BOTH), (0, V, cost, r, -1, TAU, gp, BOTH),                                  # keep outside 0..8
                     (0, V, cost, r, keep, -1, gp, BOTH), (0, V, cost, r, keep, 256, gp, BOTH), (0, V, cost, r, keep, 256, None, BOTH),             # tau outside 0..255
                     (-1, 2, cost, r, keep, TAU, gp, BOTH), (0, V + 1, cost, r, keep, TAU, gp, BOTH), (4, 3, cost, r, keep, TAU, gp, BOTH), (0, -1, cost, r, keep, TAU, gp, BOTH),
                     (0, V, cost, r, keep, TAU, gp, 0), (0, V, cost, r, keep, TAU, gp, BOTH | mvs_amd.MVS_SWEEP_FORCE_GENERIC),
                     (0, V, cost, r, keep, TAU, gp, BOTH | mvs_amd.MVS_SWEEP_NO_RECT), (0, V, cost, r, keep, TAU, gp, VOLUME | 0x100),
                     (0, V, cost, r, keep, TAU, gp, 0x80000000 | FUSED)):
            assert run(h, *args) == EINVAL, args
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], other[3], "after EINVAL %s" % (args,))
            _same_maps(got[:3], other[:3], "after EINVAL %s" % (args,))
            good("after EINVAL %s" % (args,))
            ctx.sweep_run_bestk(ABSDIFF, 1, 3, 0, 3, BOTH)
        # the exact sampler
        ctx.set_sampler("exact")
        assert run(h, 0, V, cost, r, keep, TAU, gp, BOTH) == ESTATE and b"FIXED" in lib.mvs_last_error(h)
        ctx.set_sampler("fixed")
        good("after the exact sampler")
        # a caller's volume that is one cell short: refused for a volume run, not needed by a selection alone
        short = torch.empty(c.D * c.H * c.W - 1, dtype=torch.int32, device="cuda")
        short.fill_(7)
        torch.cuda.synchronize()
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert run(h, 0, V, cost, r, keep, TAU, gp, BOTH) == EINVAL and b"caller volume" in lib.mvs_last_error(h)
        assert run(h, 0, V, cost, r, keep, TAU, gp, VOLUME) == EINVAL
        ctx.sweep_run_bestk_gated(cost, r, keep, TAU, g.data_ptr(), 0, V, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], maps, "fused alone beside a short volume")
        assert (short.cpu() == 7).all(), "a refused call wrote into the caller's volume"
        ctx.sweep_use_volume(0, 0)
        good("after the short volume")
        # the propagation's gate: refused values record nothing
        assert lib.mvs_propagate_set_gate(None, 30, None) == EINVAL
        start = _device(pc.crafted().prior)
        ctx.propagate_set_gate(TAU, g.data_ptr())
        for tau in (-1, 256):
            assert lib.mvs_propagate_set_gate(h, tau, None) == EINVAL and b"tau" in lib.mvs_last_error(h)
        ctx.propagate_init(start.data_ptr(), ZNCC, 2, 2)
        _same_state(ctx, _gated_shots(ZNCC, 2, 2, False, 0, "crafted")[0], "after EINVAL of mvs_propagate_set_gate: the gate recorded before it")


# ---- the propagation ---------------------------------------------------------------------------------------------------------------
PROP_VARIANTS = ((KEEP_ALL, False, 2), (2, True, 0), (2, False, 2), (KEEP_ALL, True, 0))     # (keep, slopes, nrandom)
_SHOTS = {}


def _gated_shots(cost, r, keep, slopes, nrandom, guide, tau=TAU):
    """the mirror on the crafted case under the gate -> snapshots after init, after run(1) and after another run(1)"""
    import orc
    key = (cost, r, keep, slopes, nrandom, guide, tau)
    if key not in _SHOTS:
        c = pc.crafted()
        state = pm.State(gm.Scene(orc.load(), *c.views(), tau=tau, guide=gc.guide_of(guide)), c.prior, cost, r, keep, slopes=slopes, max_step=pc.MAX_STEP if slopes else np.inf)
        shots = [pc.snapshot(state)]
        for _ in range(2):
            state.run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
            shots.append(pc.snapshot(state))
        _SHOTS[key] = shots
    return _SHOTS[key]


def _prop_context():
    c = pc.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set_main(c.main_cam, c.main_img)
    ctx.sweep_set_views(c.side_cams, c.sides)
    return c, ctx, _device(c.prior)


@pytest.mark.parametrize("cost,r", ((ABSDIFF, 1), (ABSDIFF, 4), (ZNCC, 1), (ZNCC, 4)))
def test_gated_propagation_on_the_crafted_case(cost, r):
    c, ctx, start = _prop_context()
    g = _device(gc.crafted_guide())
    with ctx:
        ctx.propagate_set_gate(TAU, g.data_ptr())
        for keep, slopes, nrandom in PROP_VARIANTS:
            what = "%s r = %d keep = %d slopes = %d nrandom = %d" % (gc.NAMES[cost], r, keep, slopes, nrandom)
            shots = _gated_shots(cost, r, keep, slopes, nrandom, "crafted")
            max_step = pc.MAX_STEP if slopes else float("inf")
            ctx.propagate_init(start.data_ptr(), cost, r, keep, slopes=slopes, max_step=max_step)
            _same_state(ctx, shots[0], what + ", init")
            ctx.propagate_run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, shots[1], what + ", one iteration")
            ctx.propagate_run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, shots[2], what + ", two iterations")
            ctx.propagate_init(start.data_ptr(), cost, r, keep, slopes=slopes, max_step=max_step)
            ctx.propagate_run(2, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, shots[2], what + ", run(2)")
        assert any((_gated_shots(cost, r, k, s, n, "crafted")[2][3] != pc.crafted_states(cost, r, k, s, n)[1][2][3]).any() for k, s, n in PROP_VARIANTS[:1])


def test_the_propagations_gate_is_taken_by_init():
    c, ctx, start = _prop_context()
    cost, r, keep, slopes, nrandom = ZNCC, 2, 2, True, 2
    g, main_copy = _device(gc.crafted_guide()), _device(c.main_img)
    init = dict(slopes=slopes, max_step=pc.MAX_STEP)
    ungated = pc.crafted_states(cost, r, keep, slopes, nrandom)[1]
    by_main, by_guide = _gated_shots(cost, r, keep, slopes, nrandom, "main", 12), _gated_shots(cost, r, keep, slopes, nrandom, "crafted")
    assert (by_main[2][3] != ungated[2][3]).any() and (by_guide[2][3] != ungated[2][3]).any()
    with ctx:
        # the default gate is none
        ctx.propagate_init(start.data_ptr(), cost, r, keep, **init)
        ctx.propagate_run(2, pc.DZ, pc.DG, nrandom, pc.SEED)
        _same_state(ctx, ungated[2], "the default gate")
        # guide NULL against a device copy of the main image
        for what, ptr in (("guide NULL", None), ("a copy of the main image as the guide", main_copy.data_ptr())):
            ctx.propagate_set_gate(12, ptr)
            ctx.propagate_init(start.data_ptr(), cost, r, keep, **init)
            ctx.propagate_run(2, pc.DZ, pc.DG, nrandom, pc.SEED)
            _same_state(ctx, by_main[2], what)
        # a set_gate between init and run changes nothing until the next init; the caller's buffer may change after init
        ctx.propagate_set_gate(TAU, g.data_ptr())
        ctx.propagate_init(start.data_ptr(), cost, r, keep, **init)
        _same_state(ctx, by_guide[0], "the crafted guide, init")          # (synchronises: the copy of the guide is done)
        ctx.propagate_set_gate(3, None)
        g.fill_(0)
        torch.cuda.synchronize()
        ctx.propagate_run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
        _same_state(ctx, by_guide[1], "set_gate and an overwritten guide between init and run")
        ctx.propagate_set_gate(255, None)
        ctx.propagate_run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
        _same_state(ctx, by_guide[2], "gate 255 recorded, the runs still use the init's")
        # gate 255 after a gated run: today's bytes
        ctx.propagate_init(start.data_ptr(), cost, r, keep, **init)
        ctx.propagate_run(2, pc.DZ, pc.DG, nrandom, pc.SEED)
        _same_state(ctx, ungated[2], "gate 255 after a gated run")


@pytest.mark.parametrize("cost", (ABSDIFF, ZNCC))
@pytest.mark.parametrize("W,H,r", [(9, 5, 4), (TILE[0] + 1, TILE[1] + 1, 2)])
def test_gated_propagation_at_the_kernels_edges(oracle, cost, W, H, r):
    views = _noise_views(W, H, 3, 0x6A7E + W)
    guide = _edge_guide(W, H)
    start = pc.seam_start(W, H, 0xBE57 + W)
    state = pm.State(gm.Scene(oracle, *views, tau=TAU, guide=guide), start, cost, r, 2, slopes=True, max_step=0.05)
    what = "%d x %d, %s r = %d" % (W, H, gc.NAMES[cost], r)
    g = _device(guide)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main(views[0], views[1])
        ctx.sweep_set_views(views[2], views[3])
        ctx.propagate_set_gate(TAU, g.data_ptr())
        ctx.propagate_init(_device(start).data_ptr(), cost, r, 2, slopes=True, max_step=0.05)
        _same_state(ctx, pc.snapshot(state), what + ", init")
        for it in range(2):
            state.run(1, 0.04, 0.01, 2, 11)
            ctx.propagate_run(1, 0.04, 0.01, 2, 11)
            _same_state(ctx, pc.snapshot(state), what + ", iteration %d" % it)


PROPAGATE = dict(iterations=2, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=9, slopes=True)


def _gated_propagated(oracle, views, start, cost, r, keep, propagate, step, tau):
    state = pm.State(gm.Scene(oracle, *views, tau=tau), start, cost, r, keep, slopes=bool(propagate.get("slopes", False)))
    return state.run(int(propagate["iterations"]), float(f32(float(propagate["dz_steps"]) * step)), float(f32(float(propagate["dg_steps"]) * step)),
                     int(propagate["nrandom"]), int(propagate["seed"]))


def test_coarse_to_fine_with_a_gated_propagation(oracle):
    W, H, DC, DB = 96, 64, 16, 16
    views, _ = bb.exposure_views(W, H)
    cost = dict(cost="absdiff", radius=1, keep=3)
    final = bb.two_levels(oracle, views, DC, DB, ABSDIFF, 1, 3, None)[0]
    hb = float(f32(1.5 * 2.0 / DC))
    gated = _gated_propagated(oracle, views, final, ABSDIFF, 1, 3, PROPAGATE, 2.0 * hb / DB, 6)          # (the scene is smooth: 6 takes a quarter of the members out)
    ungated = pc.propagated(oracle, views, final, ABSDIFF, 1, 3, PROPAGATE, 2.0 * hb / DB)
    assert (gated.cells != ungated.cells).any()
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, 1)
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(PROPAGATE, tau=6))
        _same_bits(got, gated.z, "coarse_to_fine(propagate=dict(..., tau=6))")
        _same_state(ctx, pc.snapshot(gated), "coarse_to_fine(propagate=dict(..., tau=6))")
        # without the key: today's calls and today's result; the helper put 255 back
        got = mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=PROPAGATE)
        _same_bits(got, ungated.z, "coarse_to_fine(propagate=...) after a gated one")
        _same_state(ctx, pc.snapshot(ungated), "coarse_to_fine(propagate=...) after a gated one")
        with pytest.raises(ValueError, match="tau"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=dict(cost, tau=30), propagate=PROPAGATE)
        with pytest.raises(mvs_amd.MvsError, match="tau"):
            mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=dict(PROPAGATE, tau=256))
        _same_bits(mvs_amd.coarse_to_fine(ctx, DC, DB, cost=cost, propagate=PROPAGATE), ungated.z, "after a refused tau the gate is 255")


def test_pyramid_coarse_to_fine_with_a_gated_propagation(oracle):
    W, H, DC, DB, r, tau = 96, 64, 16, 16, 2, 30
    import band_bestk_mirror as bbm
    views, _ = bb.exposure_views(W, H)
    main_cam, main_img, side_cams, sides = views
    lv = pyc.levels(main_img, sides, 2)
    below = bb.global_level(oracle, (main_cam, lv[1][0], side_cams, lv[1][1]), DC, -1.0, 1.0, ZNCC, r, KEEP_ALL)[1]
    prior = pym.prior(below, tau, lv[1][0], lv[0][0])
    hb = float(f32(1.5 * 2.0 / DC))
    resolved = bbm.level(oracle, ZNCC, *views, prior, oracle.plane_table(DB, -hb, hb), r, KEEP_ALL)[0]
    gated = _gated_propagated(oracle, views, resolved, ZNCC, r, KEEP_ALL, PROPAGATE, 2.0 * hb / DB, 6)
    assert (gated.cells != pc.propagated(oracle, views, resolved, ZNCC, r, KEEP_ALL, PROPAGATE, 2.0 * hb / DB).cells).any()
    fine, half = mvs_amd.Context(W, H, 0, sampler="fixed"), mvs_amd.Context(W // 2, H // 2, 0, sampler="fixed")
    with fine, half:
        fine.sweep_set(*views, 1)
        got = mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, tau=tau, cost=dict(cost="zncc", radius=r), propagate=dict(PROPAGATE, tau=6))
        _same_bits(got, gated.z, "pyramid_coarse_to_fine(propagate=dict(..., tau=6))")
        _same_state(fine, pc.snapshot(gated), "pyramid_coarse_to_fine(propagate=dict(..., tau=6))")
        assert half.propagate_depth_pointer() == 0
        with pytest.raises(ValueError, match="tau"):
            mvs_amd.pyramid_coarse_to_fine([fine, half], DC, DB, tau=tau, cost=dict(cost="zncc", radius=r, tau=6), propagate=PROPAGATE)


@pytest.mark.parametrize("cost", (ABSDIFF, ZNCC))
def test_contrast_scene(oracle, cost):
    s = gc.scene("contrast")
    D, r, keep, tau = 16, 2, 2, 30
    ref = gc.scene_volume("contrast", cost, r, D, keep, tau)
    z = oracle.plane_table(D, s.z_lo, s.z_hi)
    with mvs_amd.Context(s.W, s.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*s.views(), D, s.z_lo, s.z_hi)
        ctx.sweep_run_bestk_gated(cost, r, keep, tau, None, 0, s.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
    _same_cells(got[3], ref, "contrast scene")
    _same_maps(got[:3], gc.maps(oracle, ref, z), "contrast scene")
    assert gc.bad_shares(oracle, "contrast", got[0], D) == gc.wta_shares(oracle, "contrast", ref, D)
