"""Inputs of the occlusion-robust sweep's tests (tests/test_bestk_cpu.py, tests/test_bestk_gpu.py): the crafted case, the occluder scene
and the mirror's results on them.  Everything is computed once, shared and read-only."""
import functools

import numpy as np

import bestk_mirror as bm
import zncc_cases as zc
import zncc_mirror as zm
from mvs_amd import synth

ABSDIFF, ZNCC, KEEP_ALL = bm.COST_ABSDIFF, bm.COST_ZNCC, bm.KEEP_ALL
COST_RADII = [(ABSDIFF, 0), (ABSDIFF, 1), (ABSDIFF, 2), (ABSDIFF, 4), (ZNCC, 1), (ZNCC, 2), (ZNCC, 4)]
KEEPS = (1, 2, 3, 8, KEEP_ALL)
RANGES = ((0, 6), (1, 3), (0, 3))     # (view_first, view_count) of the crafted case: all, [1, 4) with the identity view, [0, 3) without
NAMES = {ABSDIFF: "absdiff", ZNCC: "zncc"}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Crafted:
    """zncc_cases.Crafted (70 x 19, 7 planes, views 0-4) plus view 5, a duplicate of view 0: the same camera and the same frame, so that
    equal per-view costs occur at every cell where view 0 counts.  View 3 is the main camera with the main frame itself (cost 0 wherever
    it counts), view 4 the main camera with the inverted main frame (ZNCC: 65024, the top of the scale)"""
    V = zc.Crafted.V + 1

    def __init__(self):
        c = zc.crafted()
        self.W, self.H, self.D, self.Z_LO, self.Z_HI = c.W, c.H, c.D, c.Z_LO, c.Z_HI
        self.main_cam, self.main_img = c.main_cam, c.main_img
        self.side_cams = np.concatenate([c.side_cams, c.side_cams[:1]])
        self.sides = list(c.sides) + [c.sides[0].copy()]
        _frozen(self.side_cams, self.sides[-1])

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides

    def planes(self, oracle):
        return oracle.plane_table(self.D, self.Z_LO, self.Z_HI)


@functools.lru_cache(maxsize=None)
def crafted():
    return Crafted()


@functools.lru_cache(maxsize=None)
def crafted_view(cost, r, v):
    """the mirror on view v of the crafted case -> (counted, c), [D, H, W] each"""
    import orc
    if v == Crafted.V - 1:
        return crafted_view(cost, r, 0)
    if cost == ZNCC:
        return zc.crafted_view(r, v)[1:]
    c, oracle = crafted(), orc.load()
    out = bm.view_costs(oracle, cost, c.main_cam, c.main_img, c.side_cams[v], c.sides[v], c.D, c.Z_LO, c.Z_HI, r)
    _frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def _crafted_volume(cost, r, keep, views):
    vol = bm.merge([crafted_view(cost, r, v) for v in views], keep, (zc.Crafted.D, zc.Crafted.H, zc.Crafted.W))
    _frozen(vol)
    return vol


def crafted_volume(cost, r, keep, views=None):
    """the mirror's volume of the crafted case (over the side views `views`, default all)"""
    return _crafted_volume(cost, r, keep, tuple(range(Crafted.V)) if views is None else tuple(views))


maps = zc.maps


class Occluder:
    """Two fronto-parallel textured planes seen by synth.ring_cameras(V, W, H, 0.3), V = 4 in the tests and 8 beside it in the table: a back plane at z = -3.3 with the synthetic scene's
    albedo at freq_scale 0.25, and in front of it the rectangle |X - 0.1| < 0.45, |Y + 0.05| < 0.35 at z = -2.4 with the same albedo
    displaced by (5, -3).  Next to the rectangle's outline the back plane is hidden in the views on the far side.  Planes over
    [min truth - 0.02, max truth + 0.02]"""
    W, H, RING = 160, 100, 0.3
    Z_BACK, Z_FRONT = -3.3, -2.4
    EDGE = 12                        # "edge": the background pixels within this many pixels (Chebyshev) of the rectangle in the main view

    def __init__(self, V):
        self.V = V
        self.scene = synth.Scene(synth.SEED_SCENE, 0.25)
        self.main_cam, self.side_cams = synth.ring_cameras(self.V, self.W, self.H, self.RING)
        self.main_img, self.truth, self.front = self.render([0.0, 0.0, 0.0])
        self.sides = []
        for v in range(self.V):
            a = 2.0 * np.pi * v / self.V
            self.sides.append(self.render([self.RING * np.cos(a), self.RING * np.sin(a), 0.0])[0])
        self.z_lo, self.z_hi = float(self.truth.min()) - 0.02, float(self.truth.max()) + 0.02
        self.edge = (zm.box(self.front.astype(np.int64), self.EDGE) > 0) & ~self.front
        _frozen(self.main_img, self.truth, self.front, self.edge, self.side_cams, *self.sides)

    def render(self, center):
        """-> (u8 image, NDC depth of that camera, mask of the rectangle)"""
        cx, cy, cz = center
        W, H = self.W, self.H
        col = (np.arange(W, dtype=np.float64) * 2 + 1) / W - 1.0
        row = 1.0 - (np.arange(H, dtype=np.float64) * 2 + 1) / H
        dx = (col * synth.FOVX / 2.0)[None, :].repeat(H, 0)
        dy = (row * synth.FOVX / (2.0 * W / H))[:, None].repeat(W, 1)
        tf, tb = cz - self.Z_FRONT, cz - self.Z_BACK
        Xf, Yf = cx + tf * dx, cy + tf * dy
        front = (np.abs(Xf - 0.1) < 0.45) & (np.abs(Yf + 0.05) < 0.35)
        Xb, Yb = cx + tb * dx, cy + tb * dy
        alb = np.where(front, self.scene.albedo(Xf + 5.0, Yf - 3.0), self.scene.albedo(Xb, Yb))
        t = np.where(front, tf, tb)
        far, near = synth.FAR, synth.NEAR
        zn = (far + near) / (far - near) + (2.0 * far * near / (near - far)) / t
        return np.clip(np.rint(alb), 0, 255).astype(np.uint8), zn.astype(np.float32), front

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides


@functools.lru_cache(maxsize=None)
def occluder(V=4):
    return Occluder(V)


@functools.lru_cache(maxsize=None)
def occluder_views(cost, r, D, V=4):
    """the mirror's per-view costs of the V-view occluder scene over D planes -> a tuple of (counted, c)"""
    import orc
    o, oracle = occluder(V), orc.load()
    out = tuple(bm.view_costs(oracle, cost, o.main_cam, o.main_img, o.side_cams[v], o.sides[v], D, o.z_lo, o.z_hi, r) for v in range(o.V))
    for p in out:
        _frozen(*p)
    return out


@functools.lru_cache(maxsize=None)
def occluder_volume(cost, r, D, keep, V=4):
    o = occluder(V)
    vol = bm.merge(occluder_views(cost, r, D, V), keep, (D, o.H, o.W))
    _frozen(vol)
    return vol


def bad_shares(oracle, vol, D, V=4):
    """winner-take-all on the V-view occluder scene's volume -> (share of pixels more than 1.5 plane steps from the analytic depth over
    the whole image, the same share over the edge pixels)"""
    o = occluder(V)
    depth = oracle.argmin(vol, oracle.plane_table(D, o.z_lo, o.z_hi), sampler="fixed")[0]
    bad = np.abs(depth - o.truth) > 1.5 * (o.z_hi - o.z_lo) / D
    return float(bad.mean()), float(bad[o.edge].mean())
