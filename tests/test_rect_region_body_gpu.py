"""The two region bodies of the rectified-view kernel (csrc/sweep_rect.hip): the straight-line CLEAN body (every plane of the
wavefront certified and wholly in frame) and the per-plane body (border planes, planes with nothing in frame, failed certificates).
Each case is compared cell for cell with the general tiled kernel (MVS_SWEEP_NO_RECT) and, where small enough, with the oracle; the
planner's statistics (MVS_RECT_VERBOSE: clean regions; planes with nothing in frame, with a failed certificate, at each border) show that
a case exercises what it is there for."""
import re

import numpy as np
import pytest

import mvs_amd
from mvs_amd import synth

pytestmark = pytest.mark.gpu

BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN


def _same(a, b):
    for x, y, name in zip(a, b, ("depth", "cost", "index", "volume")):
        if x is None and y is None:
            continue
        bad = np.count_nonzero(x != y)
        assert bad == 0, "%s: %d of %d differ" % (name, bad, x.size)


STAT = re.compile(r"sweep_rect_plan: clean regions ([0-9.]+) % of \d+; planes: nothing in frame ([0-9.]+) %, failed certificate ([0-9.]+) %, "
                  r"border left ([0-9.]+) % right ([0-9.]+) % top ([0-9.]+) % bottom ([0-9.]+) %")


def _plan_stats(text):
    """what the planner printed last (percent): clean regions, and per plane nothing in frame, failed certificate, border by side"""
    got = STAT.findall(text)
    assert got, "the planner printed no region statistics:\n" + text[-2000:]
    return dict(zip(("clean", "none", "flagged", "left", "right", "top", "bottom"), map(float, got[-1])))


def _rect_vs_general(W, H, D, V, radius, freq_scale=None, extra=0):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=radius, freq_scale=freq_scale)
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH | extra)
        assert ctx.plan_shape() == 4, "the ring geometry should take the rectified kernel"
        rect = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_run(0, V, BOTH | mvs_amd.MVS_SWEEP_NO_RECT)
        gen = ctx.sweep_fetch(want_volume=True)
    _same(rect, gen)
    return (main_cam, main_img, side_cams, sides), rect


@pytest.mark.parametrize("W,H,D,V,radius,kinds", [
    (256, 64, 32, 4, 0.02, ("left", "right", "top", "bottom")),  # small baseline: mostly clean, border tiles on all four sides
    (320, 240, 32, 4, 0.3, ("none", "left", "right", "top", "bottom")),  # wide baseline: border tiles, planes wholly out of frame
    (130, 45, 24, 4, 0.1, ("left", "right")),  # ragged last tiles: W not a multiple of 64, H not a multiple of 8, ragged last chunk
    (333, 77, 37, 5, 0.3, ("none",)),          # odd sizes, views partly out of frame at the near planes
])
def test_region_bodies_equal_general_and_oracle(oracle, monkeypatch, capfd, W, H, D, V, radius, kinds):
    monkeypatch.setenv("MVS_RECT_VERBOSE", "1")
    views, rect = _rect_vs_general(W, H, D, V, radius, freq_scale=0.5)
    st = _plan_stats(capfd.readouterr().err)
    assert 0.0 < st["clean"] < 100.0, "both region bodies should run: %s" % st
    for kind in kinds:
        assert st[kind] > 0.0, "the case should contain %s planes: %s" % (kind, st)
    ref = oracle.sweep(*views, D, want_volume=True, nthreads=8, sampler="fixed")
    np.testing.assert_array_equal(rect[3], ref[3])
    np.testing.assert_array_equal(rect[2], ref[2])


def test_region_bodies_c3_ring_rows(monkeypatch, capfd):
    """c3's own geometry (its ring has failed certificates): a 64-row band through the middle against the general kernel, and the
    planner's clean share of the whole frame"""
    monkeypatch.setenv("MVS_RECT_VERBOSE", "1")
    W, H, D, V = 1920, 1080, 128, 16
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=0.15)
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH)
        assert ctx.plan_shape() == 4
        rect_full = ctx.sweep_fetch(want_volume=False)
        st = _plan_stats(capfd.readouterr().err)
        ctx.sweep_run_rows(504, 64, 0, V, BOTH | mvs_amd.MVS_SWEEP_NO_RECT)
        gen = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_run_rows(504, 64, 0, V, BOTH)
        rect = ctx.sweep_fetch(want_volume=True)
    assert 50.0 < st["clean"] < 100.0 and st["flagged"] > 0.0, "c3's ring has clean regions and failed certificates: %s" % st
    _same(rect[3][:, 504:568], gen[3][:, 504:568])
    for a, b in zip(rect[:3], gen[:3]):
        np.testing.assert_array_equal(a[504:568], b[504:568])
    for a, b in zip(rect_full[:3], rect[:3]):
        np.testing.assert_array_equal(a[504:568], b[504:568])


def test_region_bodies_view_subsets_and_plane_splits():
    """subsets of the views (regions of one view at a time) summed into the whole volume, and forced plane splits"""
    W, H, D, V = 448, 200, 64, 6
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=0.2, freq_scale=0.5)
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH | mvs_amd.MVS_SWEEP_NO_RECT)
        full = ctx.sweep_fetch(want_volume=True)
        acc = np.zeros_like(full[3])
        for v0 in range(V):
            ctx.sweep_run(v0, 1, mvs_amd.MVS_SWEEP_VOLUME)
            assert ctx.plan_shape() == 4
            acc += ctx.sweep_fetch(want_volume=True)[3]
        np.testing.assert_array_equal(acc, full[3])
        for nsplit in (1, 2, 4):
            ctx.sweep_run(0, V, BOTH | (nsplit << 16))
            got = ctx.sweep_fetch(want_volume=True)
            _same(got, full)
