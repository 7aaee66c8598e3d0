"""Inputs of the ZNCC sweep's tests (tests/test_zncc_cpu.py, tests/test_zncc_gpu.py): the crafted case, the exposure scene and the
mirror's results on them.  Everything is computed once, shared and read-only."""
import functools

import numpy as np

import band_cases as bc
import zncc_mirror as zm
from mvs_amd import synth

RADII = (1, 2, 4)
GAINS = ((0.8, 12.0), (1.1, -8.0), (0.9, 5.0), (1.0, 15.0))   # (gain, offset) of the exposure scene's four side frames


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Crafted:
    """70 x 19: tile rests in both directions; 7 planes over (-0.6, 0.9); five views.  Views 0-2 are band_cases.general_views(70, 19, 3)
    with a constant block in the main image (va = 0), a saturated band in side 0 (vb = 0) and side 1 inverted (negative correlation);
    view 3 is the main camera with the main frame itself (ncc clamps at 1, c = 0), view 4 the main camera with the inverted main frame
    (c = 65024)"""
    W, H, D, V, Z_LO, Z_HI = 70, 19, 7, 5, -0.6, 0.9

    def __init__(self):
        main_cam, main_img, cams, sides, _ = bc.general_views(self.W, self.H, 3)
        main_img = main_img.copy()
        main_img[2:9, 5:14] = 77
        sides = [s.copy() for s in sides]
        sides[0][:, 30:50] = 255
        sides[1] = 255 - sides[1]
        self.main_cam, self.main_img = main_cam, main_img
        self.side_cams = np.stack(list(cams) + [main_cam, main_cam])
        self.sides = sides + [main_img.copy(), 255 - main_img]
        _frozen(self.main_img, self.side_cams, *self.sides)

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides

    def planes(self, oracle):
        return oracle.plane_table(self.D, self.Z_LO, self.Z_HI)


@functools.lru_cache(maxsize=None)
def crafted():
    return Crafted()


@functools.lru_cache(maxsize=None)
def crafted_view(r, v):
    """the mirror on view v of the crafted case at radius r -> (ok, counted, c), [D, H, W] each"""
    import orc
    c, oracle = crafted(), orc.load()
    out = zm.view_volume(oracle, c.main_cam, c.main_img, c.side_cams[v], c.sides[v], c.planes(oracle), r)
    _frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def _crafted_volume(r, views):
    vol = np.zeros((Crafted.D, Crafted.H, Crafted.W), np.uint32)
    for v in views:
        vol += zm.cells(*crafted_view(r, v)[1:])
    _frozen(vol)
    return vol


def crafted_volume(r, views=None):
    """the mirror's volume of the crafted case at radius r (over the side views `views`, default all)"""
    return _crafted_volume(r, tuple(range(Crafted.V)) if views is None else tuple(views))


def maps(oracle, vol, z, refine=False):
    """(depth, cost, index) of mvs_sweep_argmin on vol, the depth refined if asked"""
    depth, cost, index = oracle.argmin(vol, z, sampler="fixed")
    if refine:
        depth = oracle.refine_depth(vol, z, index, sampler="fixed")
    return depth, cost, index


class Exposure:
    """synth.make_views(96, 64, 4), 48 planes over [-1, 1]; `gains`: side frame v becomes clip(rint(g_v I + o_v))"""
    W, H, D, V, R = 96, 64, 48, 4, 3

    def __init__(self, gains):
        self.main_cam, self.main_img, self.side_cams, sides, self.truth = synth.make_views(self.W, self.H, self.V)
        if gains:
            sides = [np.clip(np.rint(g * s.astype(np.float64) + o), 0, 255).astype(np.uint8) for s, (g, o) in zip(sides, GAINS)]
        self.sides = [np.ascontiguousarray(s) for s in sides]
        _frozen(self.main_img, self.truth, *self.sides)

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides


@functools.lru_cache(maxsize=None)
def exposure(gains):
    return Exposure(gains)


@functools.lru_cache(maxsize=None)
def exposure_volume(gains, r):
    import orc
    e, oracle = exposure(gains), orc.load()
    vol = zm.volume(oracle, *e.views(), oracle.plane_table(e.D, -1.0, 1.0), r)
    _frozen(vol)
    return vol


def quality(oracle, vol, truth, D):
    """winner-take-all on vol -> (share of pixels more than 1.5 plane steps from the analytic depth, median error after refine_depth)"""
    z = oracle.plane_table(D, -1.0, 1.0)
    depth, _, index = oracle.argmin(vol, z, sampler="fixed")
    refined = oracle.refine_depth(vol, z, index, sampler="fixed")
    return float((np.abs(depth - truth) > 1.5 * 2.0 / D).mean()), float(np.median(np.abs(refined - truth)))
