"""Inputs of the windowed band sweep's tests (tests/test_band_bestk_cpu.py, tests/test_band_bestk_gpu.py): the crafted case, the exposure
scene at two sizes, the occluder scene, and the two-level composition of mirrors that the coarse-to-fine helpers must equal.  Everything is
computed once, shared and read-only."""
import functools

import numpy as np

import band_bestk_mirror as bbm
import band_cases as bc
import band_mirror as bm
import bestk_cases as bk
import bestk_mirror as km
import depth_filter_mirror as dm
import zncc_cases as zc
from mvs_amd import synth

ABSDIFF, ZNCC, KEEP_ALL = bbm.COST_ABSDIFF, bbm.COST_ZNCC, bbm.KEEP_ALL
COST_RADII = [(ABSDIFF, 0), (ABSDIFF, 1), (ABSDIFF, 4), (ZNCC, 1), (ZNCC, 2), (ZNCC, 4)]
KEEPS = (KEEP_ALL, 1, 2, 3, 8)
RANGES = ((0, 5), (1, 3), (0, 2), (2, 3))      # (view_first, view_count); [0, 2) and [2, 5) are disjoint and cover every view
NAMES = bk.NAMES
f32 = np.float32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Crafted:
    """zncc_cases.Crafted's 70 x 19 frames and five views (a constant block in the main image, a saturated band in side 0, side 1
    inverted, the main camera with the main frame and with its inverse) with band_cases.Crafted's prior (a ramp, a step, a block of 1.0,
    NaNs, columns at +-0.995 whose planes are mostly dead, a block of i.i.d. values) and 7 offsets over [-0.3, 0.3]"""
    W, H, D, V, HB = zc.Crafted.W, zc.Crafted.H, 7, zc.Crafted.V, 0.3

    def __init__(self):
        c = zc.crafted()
        assert (c.W, c.H) == (bc.Crafted.W, bc.Crafted.H)
        self.main_cam, self.main_img, self.side_cams, self.sides = c.views()
        self.prior = bc.crafted().prior

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides

    def offsets(self, oracle):
        return bc.offsets(oracle, self.D, self.HB)


@functools.lru_cache(maxsize=None)
def crafted():
    return Crafted()


@functools.lru_cache(maxsize=None)
def crafted_view(cost, r, v):
    """the mirror on view v of the crafted case -> (counted, c), [D, H, W] each"""
    import orc
    c, oracle = crafted(), orc.load()
    out = bbm.view_costs(oracle, cost, c.main_cam, c.main_img, c.side_cams[v], c.sides[v], c.prior, c.offsets(oracle), r)
    _frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def _crafted_volume(cost, r, keep, views):
    vol = km.merge([crafted_view(cost, r, v) for v in views], keep, (Crafted.D, Crafted.H, Crafted.W))
    _frozen(vol)
    return vol


def crafted_volume(cost, r, keep, views=None):
    """the mirror's volume of the crafted case (over the side views `views`, default all)"""
    return _crafted_volume(cost, r, keep, tuple(range(Crafted.V)) if views is None else tuple(views))


maps = zc.maps


@functools.lru_cache(maxsize=None)
def exposure_views(W, H, V=4):
    """zncc_cases.Exposure at any size: synth.make_views(W, H, V) with side frame v at clip(rint(g_v I + o_v)) -> (views, analytic depth)"""
    main_cam, main_img, side_cams, sides, truth = synth.make_views(W, H, V)
    sides = [np.ascontiguousarray(np.clip(np.rint(g * s.astype(np.float64) + o), 0, 255).astype(np.uint8)) for s, (g, o) in zip(sides, zc.GAINS)]
    _frozen(main_img, truth, *sides)
    return (main_cam, main_img, side_cams, sides), truth


def filtered(depth, guide, filter, step):
    """the `filter` keyword of the coarse-to-fine helpers on the mirror"""
    return dm.filter(depth, filter["radius"], filter.get("tau", 255), f32(filter.get("max_steps", float("inf")) * step), guide)


def global_level(oracle, views, D, z_lo, z_hi, cost, r, keep):
    """mvs_sweep_run_bestk over D planes, selected and refined -> (winner-take-all depth, refined depth, volume)"""
    z = oracle.plane_table(D, z_lo, z_hi)
    vol = km.volume(oracle, cost, *views, D, z_lo, z_hi, r, keep)
    depth, _, index = oracle.argmin(vol, z, sampler="fixed")
    return depth, oracle.refine_depth(vol, z, index, sampler="fixed"), vol


def two_levels(oracle, views, DC, DB, cost, r, keep, filter=None, z_lo=-1.0, z_hi=1.0, band_steps=1.5):
    """mvs_amd.coarse_to_fine(ctx, DC, DB, band_steps, z_lo, z_hi, filter=filter, cost=dict(...)) as a composition of mirrors ->
    (the returned map, the band's prior, the band's volume, the band's (offset, cost, index), the resolved map before its filter)"""
    main_img = views[1]
    prior = global_level(oracle, views, DC, z_lo, z_hi, cost, r, keep)[1]
    if filter is not None:
        prior = filtered(prior, main_img, filter, (float(z_hi) - float(z_lo)) / DC)
    hb = float(f32(band_steps * (float(z_hi) - float(z_lo)) / DC))
    resolved, vol, level_maps = bbm.level(oracle, cost, *views, prior, oracle.plane_table(DB, -hb, hb), r, keep)
    out = resolved if filter is None else filtered(resolved, main_img, filter, 2.0 * hb / DB)
    return out, prior, vol, level_maps, resolved


def quality(depth, truth, step):
    """(share of pixels more than 1.5 `step` from the analytic depth, the median error)"""
    err = np.abs(np.asarray(depth, np.float64) - truth)
    return float((err > 1.5 * step).mean()), float(np.median(err))
