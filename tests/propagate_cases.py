"""Inputs of the propagation's tests (tests/test_propagate_cpu.py, tests/test_propagate_gpu.py): the crafted case and the mirror's states
on it, the start maps for the kernel's edges, the exposure scene's raw coarse map, and the compositions of mirrors that the
coarse-to-fine helpers with propagate= must equal.  Everything is computed once, shared and read-only."""
import functools

import numpy as np

import band_bestk_cases as bb
import propagate_mirror as pm

ABSDIFF, ZNCC, KEEP_ALL = pm.COST_ABSDIFF, pm.COST_ZNCC, pm.KEEP_ALL
COST_RADII = [(ABSDIFF, 0), (ABSDIFF, 1), (ABSDIFF, 4), (ZNCC, 1), (ZNCC, 2), (ZNCC, 4)]
NAMES = bb.NAMES
f32 = np.float32
DZ, DG, SEED, MAX_STEP = 0.05, 0.01, 0x5EED, 0.1      # the crafted case's random steps, seed, and slope gate
# (keep, slopes, nrandom) of the crafted case, each run for one iteration and then another; radius 4 runs the first four (every keep) only
VARIANTS = ((KEEP_ALL, False, 2), (2, True, 2), (8, True, 0), (1, False, 2), (2, False, 0), (KEEP_ALL, True, 2))


def variants(r):
    return VARIANTS[:4] if r == 4 else VARIANTS


@functools.lru_cache(maxsize=None)
def crafted():
    """section 21's 70 x 19 frames with five views and section 19's prior as the start map (band_bestk_cases.Crafted)"""
    return bb.crafted()


@functools.lru_cache(maxsize=None)
def crafted_scene():
    import orc
    return pm.Scene(orc.load(), *crafted().views())


def snapshot(state):
    out = state.copy_maps() + (state.cost_map(), tuple(state.report()))
    for a in out[:5]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def crafted_states(cost, r, keep, slopes, nrandom, view_first=0, view_count=None):
    """the mirror on the crafted case -> (the state, [snapshot after init, after run(1), after another run(1)]);
    a snapshot is (z, gx, gy, cells, cost map, report)"""
    state = pm.State(crafted_scene(), crafted().prior, cost, r, keep, view_first, view_count, slopes, MAX_STEP if slopes else np.inf)
    shots = [snapshot(state)]
    for _ in range(2):
        state.run(1, DZ, DG, nrandom, SEED)
        shots.append(snapshot(state))
    return state, shots


def seam_start(W, H, seed):
    """a ramp with noise; holes and +-0.995 on the tile seams (columns 31 / 32, rows 15 / 16), at the frame's edge and 5 pixels from it"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    start = (-0.2 + 0.4 * x / W + 0.005 * y + rng.uniform(-0.03, 0.03, (H, W))).astype(f32)
    marks = ((3, 31, np.nan), (4, 32, 1.0), (15, 5, np.nan), (16, 6, -1.0), (15, 31, 0.995), (16, 32, -0.995), (15, 32, np.nan), (16, 31, 0.995),
             (0, 0, np.nan), (0, 5, 0.995), (5, 0, -0.995), (2, 2, 0.995), (10, 31, -0.995), (11, 32, np.nan), (15, 36, 0.995), (16, 27, np.nan),
             (30, 30, 1.0), (4, 8, -0.995), (H - 1, W - 1, np.nan), (H - 1, W - 6, 0.995), (H - 6, W - 1, np.nan), (20, 31, np.inf), (21, 32, 0.995),
             (10, 26, np.nan), (11, 37, -0.995), (0, 31, np.nan), (0, 32, 0.995))
    for row, col, v in marks:
        if 0 <= row < H and 0 <= col < W:
            start[row, col] = v
    return start


@functools.lru_cache(maxsize=None)
def exposure_start(W, H):
    """the exposure scene at W x H -> (views, analytic depth, the RAW refined map of a 16-plane global ZNCC sweep, radius 3)"""
    import orc
    views, truth = bb.exposure_views(W, H)
    start = bb.global_level(orc.load(), views, 16, -1.0, 1.0, ZNCC, 3, KEEP_ALL)[1]
    start.setflags(write=False)
    return views, truth, start


def propagated(oracle, views, start, cost, r, keep, propagate, step):
    """the `propagate` keyword of the coarse-to-fine helpers on the mirror -> the state"""
    state = pm.State(pm.Scene(oracle, *views), start, cost, r, keep, slopes=bool(propagate.get("slopes", False)))
    return state.run(int(propagate.get("iterations", 3)), float(f32(float(propagate.get("dz_steps", 0.5)) * step)),
                     float(f32(float(propagate.get("dg_steps", 0.125)) * step)), int(propagate.get("nrandom", 2)), int(propagate.get("seed", 0)))
