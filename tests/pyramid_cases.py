"""Inputs and reference compositions of the pyramid's tests (tests/test_pyramid_cpu.py, tests/test_pyramid_gpu.py): the crafted coarse
maps and guides of rule U, and the coarse-to-fine sequence composed of the oracle, the pyramid mirror and the band mirror.  Everything is
computed once, shared and read-only."""
import functools

import numpy as np

import band_mirror as bm
import pyramid_mirror as pm

FIXED = "fixed"


def levels(main_img, sides, nlevels):
    """[(main image, side images)] per level, level 0 the given frames, each further level the rule-D copy of the one before"""
    out = [(np.asarray(main_img, np.uint8), [np.asarray(s, np.uint8) for s in sides])]
    for _ in range(nlevels - 1):
        m, s = out[-1]
        out.append((pm.downsample(m), [pm.downsample(f) for f in s]))
    return out


def refined_sweep(oracle, main_cam, main_img, side_cams, sides, D):
    _, _, index, vol = oracle.sweep(main_cam, main_img, side_cams, sides, D, want_volume=True, nthreads=4, sampler=FIXED)
    return oracle.refine_depth(vol, oracle.plane_table(D, -1.0, 1.0), index, sampler=FIXED)


def band_level(oracle, main_cam, main_img, side_cams, sides, prior, D, hb):
    """one band level on `prior` -> (absolute depth, volume, (offset, cost, index))"""
    delta = oracle.plane_table(D, -hb, hb)
    vol = bm.band_volume(oracle, main_cam, main_img, side_cams, sides, prior, delta)
    _, cost, index = oracle.argmin(vol, delta, sampler=FIXED)
    offset = oracle.refine_depth(vol, delta, index, sampler=FIXED)
    return bm.resolve(prior, offset, index), vol, (offset, cost, index)


def coarse_to_fine(oracle, main_cam, main_img, side_cams, sides, nlevels, DC, DB, band_steps=1.5, tau=255):
    """what mvs_amd.pyramid_coarse_to_fine computes on nlevels contexts -> (finest depth, its prior, its volume, its (offset, cost, index))"""
    lv = levels(main_img, sides, nlevels)
    depth = refined_sweep(oracle, main_cam, lv[-1][0], side_cams, lv[-1][1], DC)
    step = 2.0 / DC
    prior = vol = maps = None
    for k in range(nlevels - 2, -1, -1):
        prior = pm.prior(depth, tau, lv[k + 1][0], lv[k][0])
        hb = float(np.float32(band_steps * step))
        depth, vol, maps = band_level(oracle, main_cam, lv[k][0], side_cams, lv[k][1], prior, DB, hb)
        step = 2.0 * hb / DB
    return depth, prior, vol, maps


class CraftedPrior:
    """35 x 21 coarse map (fine 70 x 42: two blocks across with a 6-column rest, eleven down with a 2-row rest): a ramp with a depth step
    along column 17, pixels at 1.0, -1.0 and NaN inside and on every border, a hole at each corner and along parts of the borders; guides
    with an edge along the same column (coarse column 17 = fine columns 34, 35), noise of a few grey levels on both"""
    Wc, Hc = 35, 21

    def __init__(self):
        Wc, Hc = self.Wc, self.Hc
        rng = np.random.Generator(np.random.PCG64(0x9124))
        x, y = np.meshgrid(np.arange(Wc), np.arange(Hc))
        z = (-0.6 + 0.01 * x + 0.013 * y).astype(np.float32)
        z[:, 17:] += np.float32(0.7)
        z[8:12, 5:9] = rng.uniform(-0.99, 0.99, (4, 4)).astype(np.float32)
        for r, c, v in ((0, 0, 1.0), (0, Wc - 1, np.nan), (Hc - 1, 0, -1.0), (Hc - 1, Wc - 1, 1.0), (5, 17, 1.0), (6, 16, np.nan), (7, 17, -1.0),
                        (12, 30, 1.0), (12, 31, 1.0), (13, 30, 1.0), (13, 31, 1.0), (3, 3, np.nan), (3, 4, -1.0), (15, 20, 1.5), (15, 22, -3.0)):
            z[r, c] = v
        z[0, 10:14] = 1.0
        z[Hc - 1, 20:23] = np.nan
        z[9:12, 0] = 1.0
        z[14:16, Wc - 1] = -1.0
        z[17:20, 8:12] = 1.0             # a 3 x 4 hole: fine pixels inside it have no valid tap
        self.depth = z
        gc = np.where(x < 17, 60, 180) + rng.integers(-4, 5, (Hc, Wc))
        self.coarse_guide = gc.astype(np.uint8)
        xf, _ = np.meshgrid(np.arange(2 * Wc), np.arange(2 * Hc))
        gf = np.where(xf < 35, 60, 180) + rng.integers(-4, 5, (2 * Hc, 2 * Wc))    # the fine edge one column to the right of the coarse one
        gf[20:24, 10:14] = 120                                                   # resembles no tap within 20: falls back to every valid tap
        self.fine_guide = gf.astype(np.uint8)
        for a in (self.depth, self.coarse_guide, self.fine_guide):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def crafted_prior():
    return CraftedPrior()
