"""Crafted packed cost volumes and guide images for the windowed matching cost, numpy only, with seeded generators
and read-only arrays like tests/sgm_volumes.py.  tests/test_window_cpu.py checks with the mirror alone that every one does what it is
here for; tests/test_window_gpu.py hands them to the kernel.

Every volume is uint32 [D, H, W] for cs = 24 (fixed sampler, cells count << 24 | sum) or 16 (exact sampler, count << 16 | sum); every
guide is uint8 [H, W]."""
import functools

import numpy as np

CS = {"fixed": 24, "exact": 16}
PER_SAMPLE = {24: 255 * 255, 16: 255}     # the largest cost one view adds to a sum
MAX_VIEWS = {24: 255, 16: 257}

# what the GPU file runs: every frame with every plane count, radius and tolerance, both samplers
FRAMES = ((64, 8), (65, 9), (130, 19), (7, 5))    # (W, H): one exact tile; a tile of one column and one of one row; more than one tile each way,
PLANES = (2, 5, 33)                               # no multiple of the tile; smaller than a 9 x 9 window
RADII = (0, 1, 2, 4)
TAUS = (0, 20, 255)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pack(n, s, cs):
    n, s = np.asarray(n, np.int64), np.asarray(s, np.int64)
    assert (s >= 0).all() and (s < (1 << cs)).all() and (n >= 0).all() and (n < (1 << (32 - cs))).all()
    return ((n << cs) | s).astype(np.uint32)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def noise(W, H, D, cs, seed=0):
    """30 % unseen cells, counts that vary per pixel and plane (mostly 1..4, one cell in sixteen anything up to the sampler's largest
    count), sums anywhere from 0 to count * the largest per-sample cost, one cell in eight free (ties).  Half of the unseen cells keep a
    non-zero sum field: it must not show anywhere."""
    rng = _rng(0x5EED0 + 7919 * seed + 31 * W + 17 * H + D + cs)
    n = rng.integers(1, 5, (D, H, W))
    many = rng.random((D, H, W)) < 1.0 / 16
    n[many] = rng.integers(1, MAX_VIEWS[cs] + 1, int(many.sum()))
    s = (rng.integers(0, PER_SAMPLE[cs] + 1, (D, H, W)) * n) // rng.integers(1, 9, (D, H, W))
    s[rng.random((D, H, W)) < 0.125] = 0
    unseen = rng.random((D, H, W)) < 0.30
    n[unseen] = 0
    s[unseen & (rng.random((D, H, W)) < 0.5)] = 0
    return _frozen(_pack(n, s, cs))


@functools.lru_cache(maxsize=None)
def full(W, H, D, cs):
    """every cell the largest the sampler can write: 255 << 24 | 255 * 65025 (S n reaches 40 bits at radius 4) or 257 << 16 | 65535"""
    n = MAX_VIEWS[cs]
    return _frozen(np.full((D, H, W), _pack(n, n * PER_SAMPLE[cs], cs), np.uint32))


@functools.lru_cache(maxsize=None)
def constant(W, H, D, cs):
    """one cell everywhere: every plane ties and the index is 0"""
    return _frozen(np.full((D, H, W), _pack(3, 3 * PER_SAMPLE[cs] // 7, cs), np.uint32))


@functools.lru_cache(maxsize=None)
def guide_levels(W, H, seed=0):
    """8 grey levels 9 apart: tau 0 joins equal pixels only, tau 20 those at most 2 levels apart, and neither is a box"""
    return _frozen((9 * _rng(0x61D + 131 * seed + 7 * W + H).integers(0, 8, (H, W))).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def guide_checkerboard(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return _frozen(np.where((x + y) % 2 == 0, 40, 200).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def guide_constant(W, H):
    return _frozen(np.full((H, W), 77, np.uint8))


# ---- the step case: a depth step along an intensity edge -----------------------------------------------------------------------------
STEP_W, STEP_H, STEP_D, STEP_V = 64, 32, 24, 3
STEP_PLANES = (5, 18)


@functools.lru_cache(maxsize=None)
def step_case():
    """(volume, guide, truth, near): the true plane is 5 in the left half and 18 in the right; the guide is 60 on the left and 180 on the
    right, plus or minus 6 of noise; per-view costs are uniform in [0, 90) grey levels off the true plane and in [0, 60) on it (fixed
    sampler: sums in 1/255 grey levels).  `near`: within 3 columns of the step."""
    rng = np.random.default_rng(7)
    W, H, D, V = STEP_W, STEP_H, STEP_D, STEP_V
    truth = np.where(np.arange(W)[None, :] < W // 2, STEP_PLANES[0], STEP_PLANES[1]) * np.ones((H, 1), np.int64)
    guide = (np.where(truth == STEP_PLANES[0], 60, 180) + rng.integers(-6, 7, (H, W))).astype(np.uint8)
    per = rng.integers(0, 90 * 255, (D, H, W, V))
    on = rng.integers(0, 60 * 255, (H, W, V))
    y, x = np.mgrid[0:H, 0:W]
    per[truth, y, x] = on
    vol = _pack(np.full((D, H, W), V), per.sum(-1), 24)
    near = np.abs(np.arange(W) - (W // 2 - 0.5))[None, :] * np.ones((H, 1)) < 3
    return _frozen(vol), _frozen(guide), _frozen(truth), _frozen(near)
