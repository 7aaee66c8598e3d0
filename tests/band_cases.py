"""Inputs of the band sweep's tests (tests/test_band_cpu.py, tests/test_band_gpu.py): the crafted case and the general-camera views.
Everything is computed once, shared and read-only."""
import functools

import numpy as np

import band_mirror as bm
from mvs_amd import synth


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)


def rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], np.float64)


def offsets(oracle, D, hb):
    return oracle.plane_table(D, -hb, hb)


class Crafted:
    """70 x 19: three tiles across with a 6-column rest, three down with a 3-row rest; 19 planes: one chunk and a tail of 3; 3 views: one
    turned about y, one displaced along the optical axis, one shifted so far that part of the frame leaves it; noise frames; a prior with
    a ramp, a step, a block of 1.0, NaNs, columns at +-0.995 (dead planes) and a block of i.i.d. values"""
    W, H, D, V, HB = 70, 19, 19, 3, 0.3

    def __init__(self):
        W, H = self.W, self.H
        rng = np.random.Generator(np.random.PCG64(0xBA2D))
        self.main_cam = synth.camera_at([0, 0, 0], W, H)
        self.side_cams = np.stack([synth.camera_at([0.12, 0.02, 0.0], W, H, rot=rot_y(4.0)),
                                   synth.camera_at([0.03, -0.02, -0.35], W, H),
                                   synth.camera_at([1.1, 0.1, 0.0], W, H, rot=rot_x(-2.0))])
        self.main_img = rng.integers(0, 256, (H, W), dtype=np.uint8)
        self.sides = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(self.V)]
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        prior = (-0.45 + 0.9 * x / W + 0.01 * y).astype(np.float32)         # smooth ramp
        prior[9:, 30:] += np.float32(0.25)                                  # depth step
        prior[2:6, 5:12] = 1.0                                              # background
        prior[8:16, 40:67] = rng.uniform(-0.9, 0.9, (8, 27)).astype(np.float32)   # i.i.d.: no locality between neighbours
        prior[:, 20] = 0.995                                                # most planes above 1
        prior[:, 21] = -0.995                                               # most planes below -1
        for r, c in ((0, 0), (10, 33), (18, 69), (7, 64)):
            prior[r, c] = np.nan
        self.prior = prior
        for a in (self.main_img, self.prior, *self.sides):
            a.setflags(write=False)

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides


@functools.lru_cache(maxsize=None)
def crafted():
    return Crafted()


@functools.lru_cache(maxsize=None)
def _crafted_volume(views):
    import orc
    c, oracle = crafted(), orc.load()
    vol = bm.band_volume(oracle, *c.views(), c.prior, offsets(oracle, c.D, c.HB), views=None if views is None else list(views))
    vol.setflags(write=False)
    return vol


def crafted_volume(views=None):
    """the mirror's volume of the crafted case (over the side views `views`, default all)"""
    return _crafted_volume(None if views is None else tuple(views))


@functools.lru_cache(maxsize=None)
def general_views(W, H, V):
    """the synthetic scene seen by V cameras on a ring, each turned a little about x and y: no view is rectified"""
    sc = synth.Scene(synth.SEED_SCENE, W / 1920.0)
    main_cam = synth.camera_at([0, 0, 0], W, H)
    main_img, depth = sc.render([0, 0, 0], W, H, want_depth=True)
    cams, sides = [], []
    for v in range(V):
        a = 2.0 * np.pi * v / V
        center = [0.2 * np.cos(a), 0.2 * np.sin(a), 0.0]
        cams.append(synth.camera_at(center, W, H, rot=rot_y(1.0 + v) @ rot_x(0.5 * v - 1.0)))
        sides.append(sc.render(center, W, H))     # (the frames are those of the unturned cameras: texture, not geometry, is what the tests need)
    return main_cam, main_img, np.stack(cams), sides, depth
