"""mvs_sweep_run_zncc on the device (csrc/zncc.hip), bit-identical to the mirror (tests/zncc_mirror.py) throughout:
the crafted case through every combination of outputs at every radius, frames at the kernel's own edges, view subsets, every way of
staging the frames, the readers behind the volume, the state it leaves for later calls, every error of the list and the exposure scene
whose accuracy tests/test_zncc_cpu.py reports."""
import numpy as np
import pytest
import torch

import band_cases as bc
import clean_mirror as cm
import mvs_amd
import sgm_mirror as sgm
import window_mirror as wm
import zncc_cases as zc
import zncc_mirror as zm
from mvs_amd import synth

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
VOLUME, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOLUME | FUSED
PLANE_CHUNK = 2       # csrc/zncc.hip: ZN_PC
TILE = (32, 16)       # csrc/zncc.hip: ZN_TW, ZN_TH


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


def _crafted_context():
    c = zc.crafted()
    ctx = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
    ctx.sweep_set(*c.views(), c.D, c.Z_LO, c.Z_HI)
    return c, ctx


@pytest.mark.parametrize("r", zc.RADII)
def test_crafted_case(oracle, r):
    c, ctx = _crafted_context()
    z = c.planes(oracle)
    ref = zc.crafted_volume(r)
    maps = zc.maps(oracle, ref, z)
    with ctx:
        ctx.sweep_run_zncc(r, 0, c.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "volume | fused")
        _same_maps(got[:3], maps, "volume | fused")
        # the volume alone, then the two-step selection and the refinement
        ctx.sweep_run_zncc(r, 0, 1, BOTH)        # (other cells and maps in between)
        ctx.sweep_run_zncc(r, 0, c.V, VOLUME)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], ref, "volume alone")
        ctx.sweep_argmin()
        _same_maps(ctx.sweep_fetch()[:3], maps, "volume, then mvs_sweep_argmin")
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], zc.maps(oracle, ref, z, refine=True), "refined")
    # the selection alone, on a context that never had a volume
    c, ctx = _crafted_context()
    with ctx:
        ctx.sweep_run_zncc(r, 0, c.V, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], maps, "fused alone")


def _noise_views(W, H, V, seed):
    """noise frames (variance in every window) seen by cameras that are turned, displaced along the axis, and shifted far"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cams = [synth.camera_at([0.12, 0.02, 0.0], W, H, rot=bc.rot_y(4.0)), synth.camera_at([0.03, -0.02, -0.35], W, H),
            synth.camera_at([0.6, 0.1, 0.0], W, H, rot=bc.rot_x(-2.0))][:V]
    return (synth.camera_at([0, 0, 0], W, H), rng.integers(0, 256, (H, W), dtype=np.uint8), np.stack(cams),
            [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(V)])


@pytest.mark.parametrize("W,H,D,r", [(9, 5, 3, 4),                                   # smaller than the window in both directions
                                     (2 * TILE[0], 2 * TILE[1], PLANE_CHUNK + 1, 2),  # whole tiles; a chunk and one plane
                                     (2 * TILE[0], TILE[1], 1, 1),                    # one plane
                                     (TILE[0] + 1, TILE[1] + 1, PLANE_CHUNK, 3),      # one pixel into the next tile; whole chunks
                                     (TILE[0] - 1, 2 * TILE[1] - 1, PLANE_CHUNK + 1, 4)])
def test_shapes_at_the_kernels_edges(oracle, W, H, D, r):
    views = _noise_views(W, H, 3, 0x2ACC + W)
    z = oracle.plane_table(D, -0.5, 0.7)
    ref = zm.volume(oracle, *views, z, r)
    assert (ref >> 24).max() == 3 and (ref == 0).any()
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*views, D, -0.5, 0.7)
        ctx.sweep_run_zncc(r, 0, 3, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "%d x %d x %d, r = %d" % (W, H, D, r))
        _same_maps(got[:3], zc.maps(oracle, ref, z), "%d x %d x %d, r = %d" % (W, H, D, r))


def test_view_subsets(oracle):
    c, ctx = _crafted_context()
    r = 2
    with ctx:
        vols = []
        for first, count in ((0, 2), (2, 3), (0, 5), (3, 1)):
            ctx.sweep_run_zncc(r, first, count, VOLUME)
            vols.append(ctx.sweep_fetch(want_volume=True)[3])
        _same_cells(vols[0] + vols[1], vols[2], "views [0, 2) + [2, 5)")
        _same_cells(vols[1], zc.crafted_volume(r, (2, 3, 4)), "views [2, 5)")
        _same_cells(vols[3], zc.crafted_volume(r, (3,)), "view 3 alone")
        ctx.sweep_run_zncc(r, 1, 2, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], zc.maps(oracle, zc.crafted_volume(r, (1, 2)), c.planes(oracle)), "fused, views [1, 3)")
        ctx.sweep_run_zncc(r, 2, 0, BOTH)         # no view: nothing is counted anywhere
        got = ctx.sweep_fetch(want_volume=True)
        assert not got[3].any() and (got[2] == -1).all() and (got[0] == 1.0).all() and np.isinf(got[1]).all()


def test_staged_state(oracle):
    c = zc.crafted()
    r = 2
    ref = zc.crafted_volume(r)
    maps = zc.maps(oracle, ref, c.planes(oracle))
    # the _device setters
    main_t, side_t = _device(c.main_img), [_device(s) for s in c.sides]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set_main_device(c.main_cam, main_t.data_ptr())
        ctx.sweep_set_views_device(c.side_cams, [t.data_ptr() for t in side_t])
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        ctx.sweep_run_zncc(r, 0, c.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "device setters")
        _same_maps(got[:3], maps, "device setters")
    # the slots left staged by mvs_sweep_handles
    slots = [4, 0, 3, 1]
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        ctx.frame_store(6)
        ctx.frame_upload(slots[0], c.main_img)
        for v in range(3):
            ctx.frame_upload(slots[1 + v], c.sides[v])
        ctx.sweep_handles(slots[0], c.main_cam, slots[1:], c.side_cams[:3], 8)      # leaves the slots staged
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        ctx.sweep_run_zncc(r, 0, 3, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], zc.crafted_volume(r, (0, 1, 2)), "frame store")
        _same_maps(got[:3], zc.maps(oracle, zc.crafted_volume(r, (0, 1, 2)), c.planes(oracle)), "frame store")
        ctx.sweep_run_zncc(r, 1, 2, VOLUME)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], zc.crafted_volume(r, (1, 2)), "frame store, views [1, 3)")
    # the caller's volume
    c, ctx = _crafted_context()
    with ctx:
        vol_t = torch.empty(c.D * c.H * c.W + 5, dtype=torch.int32, device="cuda")
        vol_t.fill_(-1)
        torch.cuda.synchronize()
        ctx.sweep_use_volume(vol_t.data_ptr(), vol_t.numel() * 4)
        ctx.sweep_run_zncc(r, 0, c.V, BOTH)
        got = ctx.sweep_fetch()
        mine = vol_t.cpu().numpy().view(np.uint32)
        _same_cells(mine[:-5].reshape(ref.shape), ref, "caller's volume")
        assert (mine[-5:] == 0xffffffff).all()
        _same_maps(got[:3], maps, "caller's volume")
        ctx.sweep_use_volume(0, 0)


def test_downstream_readers(oracle):
    c, ctx = _crafted_context()
    r = 2
    vol = zc.crafted_volume(r)
    z = c.planes(oracle)
    seen = sgm.seen_cells(vol, 24)
    with ctx:
        ctx.sweep_run_zncc(r, 0, c.V, BOTH)
        ctx.sweep_aggregate(4, 16, 128, 4080, refine=True)
        S = sgm.aggregate(sgm.cost16(vol, 24, 4080), 4, 16, 128)
        np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)
        _, cost, index = sgm.select(S, seen, z, 4)
        _same_maps(ctx.sweep_fetch()[:3], (sgm.refine(S, seen, z, index), cost, index), "aggregated")
        ctx.sweep_window(1, 255, None, select=True)
        Wv = wm.window(vol, 24, 1)
        _same_cells(ctx.sweep_window_fetch(), Wv, "windowed")
        _same_maps(ctx.sweep_fetch()[:3], zc.maps(oracle, Wv, z), "window select")
        ctx.sweep_argmin()
        before = zc.maps(oracle, vol, z)
        _same_maps(ctx.sweep_fetch()[:3], before, "mvs_sweep_argmin restores the maps")
        ctx.sweep_clean(0, 10, 4, 1)
        cleaned = cm.clean(*before, vol=vol, cs=24, uniqueness=10, speckle_min_size=4, speckle_max_diff=1)
        _same_maps(ctx.sweep_fetch()[:3], cleaned[:3], "cleaned")
        assert ctx.sweep_clean_report() == list(cleaned[3]) and cleaned[3][2] > 0
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, "the readers left the volume alone")


def test_state_for_later_calls(oracle):
    c, ctx = _crafted_context()
    r = 1
    prior = _device(np.zeros((c.H, c.W), np.float32))
    with ctx:
        lib, h = ctx.lib, ctx.h
        ctx.sweep_run_band(prior.data_ptr(), 0, 3, BOTH)
        ctx.sweep_band_resolve()
        ctx.sweep_run_zncc(r, 0, c.V, BOTH)
        assert lib.mvs_sweep_band_resolve(h) == ESTATE, "a ZNCC run ends the band run's state"
        ctx.sweep_refine_depth()
        ctx.sweep_run_zncc(r, 0, c.V, VOLUME)
        assert lib.mvs_sweep_refine_depth(h) == ESTATE and lib.mvs_sweep_clean(h, 0, 0, 4, 1, 0) == ESTATE, "no selection on this volume yet"
        ctx.sweep_argmin()
        ctx.sweep_refine_depth()
        _same_maps(ctx.sweep_fetch()[:3], zc.maps(oracle, zc.crafted_volume(r), c.planes(oracle), refine=True), "argmin, then the refinement")


def test_errors(oracle):
    c = zc.crafted()
    r = 2
    ref = zc.crafted_volume(r)
    maps = zc.maps(oracle, ref, c.planes(oracle))
    with mvs_amd.Context(c.W, c.H, 0, sampler="fixed") as ctx:
        lib, h = ctx.lib, ctx.h

        def good(what):
            ctx.sweep_run_zncc(r, 0, c.V, BOTH)
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], ref, what)
            _same_maps(got[:3], maps, what)

        assert lib.mvs_sweep_run_zncc(None, 0, 0, r, BOTH) == EINVAL
        # nothing staged: no planes, no main view, no views
        assert lib.mvs_sweep_run_zncc(h, 0, 0, r, BOTH) == ESTATE
        ctx.sweep_set_planes(c.D, c.Z_LO, c.Z_HI)
        assert lib.mvs_sweep_run_zncc(h, 0, 0, r, BOTH) == ESTATE
        ctx.sweep_set_main(c.main_cam, c.main_img)
        assert lib.mvs_sweep_run_zncc(h, 0, 0, r, BOTH) == ESTATE and b"views" in lib.mvs_last_error(h)
        assert not lib.mvs_sweep_depth_device(h), "a refused call allocates nothing"
        ctx.sweep_set_views(c.side_cams, c.sides)
        good("after MVS_ESTATE")
        # the maps and the volume of another run, which no refused call may touch
        ctx.sweep_run_zncc(1, 0, 3, BOTH)
        other = ctx.sweep_fetch(want_volume=True)
        _same_cells(other[3], zc.crafted_volume(1, (0, 1, 2)), "radius 1, views [0, 3)")
        for args in ((0, c.V, 0, BOTH), (0, c.V, 5, BOTH), (0, c.V, -1, BOTH), (-1, 2, r, BOTH), (0, c.V + 1, r, BOTH), (3, 3, r, BOTH), (0, -1, r, BOTH),
                     (0, c.V, r, 0), (0, c.V, r, BOTH | mvs_amd.MVS_SWEEP_FORCE_GENERIC), (0, c.V, r, BOTH | mvs_amd.MVS_SWEEP_NO_RECT),
                     (0, c.V, r, VOLUME | 0x100), (0, c.V, r, 0x80000000 | FUSED)):
            assert lib.mvs_sweep_run_zncc(h, *args) == EINVAL, args
            got = ctx.sweep_fetch(want_volume=True)
            _same_cells(got[3], other[3], "after EINVAL %s" % (args,))
            _same_maps(got[:3], other[:3], "after EINVAL %s" % (args,))
            good("after EINVAL %s" % (args,))
            ctx.sweep_run_zncc(1, 0, 3, BOTH)
        # the exact sampler
        ctx.set_sampler("exact")
        assert lib.mvs_sweep_run_zncc(h, 0, c.V, r, BOTH) == ESTATE and b"FIXED" in lib.mvs_last_error(h)
        ctx.set_sampler("fixed")
        good("after the exact sampler")
        # a caller's volume that is one cell short: refused for a volume run, not needed by a selection alone
        short = torch.empty(c.D * c.H * c.W - 1, dtype=torch.int32, device="cuda")
        short.fill_(7)
        torch.cuda.synchronize()
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert lib.mvs_sweep_run_zncc(h, 0, c.V, r, BOTH) == EINVAL and b"caller volume" in lib.mvs_last_error(h)
        assert lib.mvs_sweep_run_zncc(h, 0, c.V, r, VOLUME) == EINVAL
        ctx.sweep_run_zncc(r, 0, c.V, FUSED)
        _same_maps(ctx.sweep_fetch()[:3], maps, "fused alone beside a short volume")
        assert (short.cpu() == 7).all(), "a refused call wrote into the caller's volume"
        ctx.sweep_use_volume(0, 0)
        good("after the short volume")


def test_exposure_scene(oracle):
    e = zc.exposure(True)
    ref = zc.exposure_volume(True, e.R)
    z = oracle.plane_table(e.D, -1.0, 1.0)
    with mvs_amd.Context(e.W, e.H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(*e.views(), e.D)
        ctx.sweep_run_zncc(e.R, 0, e.V, BOTH)
        got = ctx.sweep_fetch(want_volume=True)
        _same_cells(got[3], ref, "exposure scene")
        _same_maps(got[:3], zc.maps(oracle, ref, z), "exposure scene")
        ctx.sweep_refine_depth()
        refined = ctx.sweep_fetch()[0]
    np.testing.assert_array_equal(refined, oracle.refine_depth(ref, z, got[2], sampler="fixed"))
    bad = float((np.abs(got[0] - e.truth) > 1.5 * 2.0 / e.D).mean())
    assert bad == zc.quality(oracle, ref, e.truth, e.D)[0] and bad <= 0.05
