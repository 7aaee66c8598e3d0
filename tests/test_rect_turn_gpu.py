"""The turn of a region in the rectified-view kernel (csrc/sweep_rect.hip): the copies that run whole-wavefront under the buffer's
range check, the record stream in the order a workgroup walks it, the decode that comes out of the planner.  sweep_fx_rect against
the general kernel sweep_fx_tiled (MVS_SWEEP_NO_RECT) and the oracle, every cell of volume, depth, best cost and index, on shapes
chosen for what those touch (the planner's MVS_RECT_VERBOSE lines show that a case is what it is there for):

  * boxes that take 1, 2 and 3 copy instructions per wavefront;
  * boxes whose last copy instruction fetches with few and with 63 of its 64 lanes.  How many lanes fetch is (rows x RS / 4) mod 64
    with RS one of 64, 84, 96, 128 and at most 32 rows: 63 lanes is 3 rows at RS 84; ONE lane is not reachable (21 x rows = 1 mod 64
    needs 61 rows; the other strides give multiples of 8) -- the fewest any plan can have is 8 (3 rows at RS 96), and that is the case
    here;
  * 1, 2 and an odd number of regions per workgroup; one view; a plane count that is not a multiple of 16; a width and a height that
    are not multiples of 64 and 8;
  * every forced plane-split count (each workgroup's share of the record stream ends in a region with no successor);
  * view subsets (the records are packed again for the launch's own order);
  * a camera ring with failed certificates and one with views partly out of frame.
"""
import re

import numpy as np
import pytest

import mvs_amd
from mvs_amd import synth

pytestmark = pytest.mark.gpu

VOL, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOL | FUSED
NO_RECT = mvs_amd.MVS_SWEEP_NO_RECT

COPIES = re.compile(r"sweep_rect_plan: copies: row stride (\d+), (\d+) instructions per region \((\d+) per wavefront\); boxes need (\d+) to (\d+), "
                    r"last instruction (\d+) to (\d+) lanes \(set 0x([0-9a-f]+)\)")
STAT = re.compile(r"sweep_rect_plan: clean regions ([0-9.]+) % of (\d+); planes: nothing in frame ([0-9.]+) %, failed certificate ([0-9.]+) %, "
                  r"border left ([0-9.]+) % right ([0-9.]+) % top ([0-9.]+) % bottom ([0-9.]+) %")


def _plan(text):
    c, s = COPIES.findall(text), STAT.findall(text)
    assert c and s, "the planner printed no statistics:\n" + text[-2000:]
    out = dict(zip(("rs", "instrs", "per_wave", "need_lo", "need_hi", "live_lo", "live_hi"), map(int, c[-1][:7])))
    out["live_set"] = int(c[-1][7], 16)
    out.update(zip(("clean", "regions", "none", "flagged", "left", "right", "top", "bottom"), map(float, s[-1])))
    return out


def _same(a, b, what):
    for x, y, name in zip(a, b, ("depth", "cost", "index", "volume")):
        if x is None or y is None:
            continue
        bad = np.count_nonzero(x != y)
        assert bad == 0, "%s, %s: %d of %d differ" % (what, name, bad, x.size)


def _all_variants(ctx, V, extra=0):
    """volume + fused, fused only and volume only of the rectified kernel against the general kernel"""
    ctx.sweep_run(0, V, BOTH | NO_RECT)
    gen = ctx.sweep_fetch(want_volume=True)
    ctx.sweep_run(0, V, BOTH | extra)
    assert ctx.plan_shape() == 4, "the ring geometry should take the rectified kernel"
    both = ctx.sweep_fetch(want_volume=True)
    _same(both, gen, "volume + fused")
    ctx.sweep_run(0, V, FUSED | extra)
    _same(ctx.sweep_fetch(want_volume=False)[:3], gen[:3], "fused only")
    ctx.sweep_run(0, V, VOL | extra)
    np.testing.assert_array_equal(ctx.sweep_fetch(want_volume=True)[3], gen[3])
    return both


CASES = {
    # name: (W, H, D, V, radius), what the plan must show (the planner counts regions per wavefront: four to a workgroup's one)
    "one_region_one_view": ((64, 8, 16, 1, 0.05), lambda p: p["per_wave"] == 1 and p["regions"] == 4),
    "two_regions": ((64, 8, 16, 2, 0.05), lambda p: p["per_wave"] == 1 and p["regions"] == 8),
    "three_regions": ((64, 8, 16, 3, 0.05), lambda p: p["regions"] == 12),
    "two_copies_per_wavefront": ((512, 128, 96, 4, 0.15), lambda p: p["per_wave"] == 2 and p["need_lo"] < p["need_hi"]),
    # ragged W, H and D; views partly out of frame; 8 lanes in a last instruction (the fewest a plan can have)
    "three_copies_ragged_out_of_frame": ((200, 90, 20, 3, 0.3), lambda p: p["per_wave"] == 3 and p["live_lo"] == 8 and p["none"] > 0.0 and p["right"] > 0.0),
    "last_copy_63_lanes": ((130, 41, 24, 4, 0.05), lambda p: p["rs"] == 84 and (p["live_set"] >> 62) & 1 and p["live_hi"] == 63),
    "last_copy_63_lanes_one_chunk": ((192, 33, 16, 3, 0.03), lambda p: (p["live_set"] >> 62) & 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_turn_equals_general_and_oracle(oracle, monkeypatch, capfd, name):
    monkeypatch.setenv("MVS_RECT_VERBOSE", "1")
    (W, H, D, V, radius), shows = CASES[name]
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=radius, freq_scale=0.5)
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        rect = _all_variants(ctx, V)
    plan = _plan(capfd.readouterr().err)
    print(name, plan)
    assert shows(plan), "the case is not what it is there for: %s" % plan
    ref = oracle.sweep(main_cam, main_img, side_cams, sides, D, want_volume=True, nthreads=8, sampler="fixed")
    np.testing.assert_array_equal(rect[3], ref[3])
    np.testing.assert_array_equal(rect[2], ref[2])
    np.testing.assert_array_equal(rect[0], ref[0])
    np.testing.assert_array_equal(rect[1], ref[1])


@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 5, 6])
def test_turn_forced_plane_splits(oracle, nsplit):
    """96 planes = 6 chunks over 1 ... 6 workgroups per tile: shares of 6, 3, 2, 2 (the last workgroup idle), 2 (ragged) and 1 chunks"""
    W, H, D, V = 200, 90, 96, 3
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=0.2, freq_scale=0.5)
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        rect = _all_variants(ctx, V, extra=nsplit << 16)
    ref = oracle.sweep(main_cam, main_img, side_cams, sides, D, want_volume=True, nthreads=8, sampler="fixed")
    for got, want in zip(rect, ref):
        np.testing.assert_array_equal(got, want)


def test_turn_view_subsets_plane_groups_and_row_bands():
    """launches that walk the regions in another order than the plan's: view subsets x plane groups (volume), then the whole again, then
    row bands with a forced split"""
    W, H, D, V = 320, 120, 96, 5
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=0.1, freq_scale=0.5)
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH | NO_RECT)
        full = ctx.sweep_fetch(want_volume=True)
        assert ctx.plan_shape() == 4
        acc = np.zeros_like(full[3])
        for v0, vn in ((0, 1), (1, 3), (4, 1)):
            for p0, pn in ((0, 32), (32, 64)):
                ctx.sweep_run_planes(v0, vn, p0, pn, VOL)
                acc[p0:p0 + pn] += ctx.sweep_fetch(want_volume=True)[3][p0:p0 + pn]
        np.testing.assert_array_equal(acc, full[3])
        ctx.sweep_run(0, V, BOTH)
        _same(ctx.sweep_fetch(want_volume=True), full, "the whole after the subsets")
        g = ctx.row_granularity()
        for r0 in range(0, H, 3 * g):
            ctx.sweep_run_rows(r0, min(3 * g, H - r0), 0, V, BOTH | (2 << 16))
        _same(ctx.sweep_fetch(want_volume=True), full, "row bands, two workgroups per tile")


def test_turn_ring_with_failed_certificates(monkeypatch, capfd):
    """c3's ring (16 views on 128 planes: a few planes per thousand fail their certificate): a 64-row band of the rectified kernel
    against the general one, every variant"""
    monkeypatch.setenv("MVS_RECT_VERBOSE", "1")
    W, H, D, V = 1920, 1080, 128, 16
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=0.15)
    lo, n = 504, 64
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run_rows(lo, n, 0, V, BOTH | NO_RECT)
        gen = [a[..., lo:lo + n, :].copy() for a in ctx.sweep_fetch(want_volume=True)]
        ctx.sweep_run_rows(lo, n, 0, V, BOTH)
        assert ctx.plan_shape() == 4
        rect = [a[..., lo:lo + n, :].copy() for a in ctx.sweep_fetch(want_volume=True)]
        plan = _plan(capfd.readouterr().err)
        _same(rect, gen, "volume + fused")
        ctx.sweep_run_rows(lo, n, 0, V, FUSED)
        _same([a[lo:lo + n] for a in ctx.sweep_fetch(want_volume=False)[:3]], gen[:3], "fused only")
        ctx.sweep_run(0, V, BOTH)  # the whole frame: the band's cells again
        _same([a[lo:lo + n] for a in ctx.sweep_fetch(want_volume=False)[:3]], gen[:3], "whole frame")
    assert plan["flagged"] > 0.0 and plan["per_wave"] == 2, "c3's ring has failed certificates and two copies per wavefront: %s" % plan
