"""Inputs of the geometric term's tests (tests/test_consistency_cpu.py, tests/test_consistency_gpu.py): the crafted case on the gated
suite's 70 x 19 frame, the counts that state its premise, the mirror's states on it, and the occluder scene's neighbour maps.  Everything
is computed once, shared and read-only.

The crafted case.  Three side views (the first three of section 21's crafted frames, whose cameras are turned a little), a start map that
is the main camera's analytic depth with a ripple, two steps and four holes, and six depth-store slots whose cameras are NOT the side
views' -- the term reads slots, not views:
  slot 0  a camera 0.2 to the right with the analytic depth of its view: e is rounding noise wherever the start map is the surface
  slot 1  the same camera; the map shifted in depth by 0.035 per column of a 32-column period, so that e crosses max_px inside a tile
  slot 2  a camera 1.2 to the right: the main view's left third projects outside its frame, the border runs down columns 25-31
  slot 3  a camera turned by 180 degrees: q_w <= 0 everywhere
  slot 4  a camera 0.2 BEHIND the main one with its near plane at 0.05, and a block of depths next to that near plane: the point such a
          depth stands for lies behind the main camera (s_w <= 0)
  slot 5  slot 0's camera and map with blocks of 1.0, NaN, 1.5 and -1.0 / -2.0
SLOTS lists eight of them, slots 0 and 2 twice."""
import functools

import numpy as np

import band_cases as bc
import consistency_mirror as cm
import fuse_mirror as fm
import gated_cases as gc
import gated_mirror as gm
import propagate_cases as pc
import propagate_mirror as pm
from mvs_amd import synth

ABSDIFF, ZNCC, KEEP_ALL = pm.COST_ABSDIFF, pm.COST_ZNCC, pm.KEEP_ALL
NAMES = pc.NAMES
f32 = np.float32
W, H, V = 70, 19, 3
TILE_W, TILE_H = 32, 16
NSLOT = 6
SLOTS = (0, 1, 2, 3, 4, 5, 0, 2)
WEIGHT, MAX_PX = 4.0, 1.0
DZ, DG, SEED = 0.05, 0.01, 0xC0DE
NEAR4 = 0.05
COST_RADII = [(ABSDIFF, 0), (ABSDIFF, 2), (ZNCC, 1), (ZNCC, 4)]
KEEPS = (KEEP_ALL, 2)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Crafted:
    def __init__(self):
        c = pc.crafted()
        assert (c.W, c.H) == (W, H)
        self.W, self.H = W, H
        self.main_cam, self.main_img = c.main_cam, c.main_img
        self.side_cams, self.sides = np.ascontiguousarray(c.side_cams[:V]), list(c.sides[:V])
        sc = synth.Scene(synth.SEED_SCENE, W / 1920.0)
        truth = sc.render([0, 0, 0], W, H, want_depth=True)[1]
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        start = (truth + 0.004 * np.sin(0.9 * x + 0.4 * y)).astype(f32)
        start[:, 20:23] += f32(0.08)                      # two steps inside the first tile
        start[6:9, 40:52] -= f32(0.06)
        for (row, col), v in (((3, 10), np.nan), ((15, 31), 1.0), ((16, 32), np.nan), ((18, 69), 1.0)):
            start[row, col] = v
        self.truth, self.start = truth, start
        right = [0.2, 0.0, 0.0]
        exact = sc.render(right, W, H, want_depth=True)[1]
        shifted = (exact + f32(0.035) * (x % TILE_W).astype(f32)).astype(f32)
        far_right = [1.2, 0.0, 0.0]
        behind = sc.render([0.0, 0.0, 0.2], W, H, want_depth=True, near=NEAR4)[1].copy()
        behind[4:14, 8:28] = f32(-0.999)                  # t = 0.05003 in front of a camera 0.2 behind the main one
        blocks = exact.copy()
        blocks[0:5, 2:12], blocks[5:10, 2:12], blocks[10:15, 2:12], blocks[0:8, 14:20], blocks[8:16, 14:20] = 1.0, np.nan, 1.5, -1.0, -2.0
        self.cams = np.stack([synth.camera_at(right, W, H), synth.camera_at(right, W, H), synth.camera_at(far_right, W, H),
                              synth.camera_at([0, 0, 0], W, H, rot=bc.rot_y(180.0)), synth.camera_at([0.0, 0.0, 0.2], W, H, near=NEAR4),
                              synth.camera_at(right, W, H)]).astype(f32)
        self.maps = [exact, shifted, sc.render(far_right, W, H, want_depth=True)[1], np.zeros((H, W), f32), behind, blocks]
        _frozen(self.truth, self.start, self.cams, self.side_cams, *self.maps)

    def views(self):
        return self.main_cam, self.main_img, self.side_cams, self.sides

    def term(self, mats=None, main=None, slots=SLOTS, weight=WEIGHT, max_px=MAX_PX):
        """the term over `slots`; mats: slot -> (P, P^-1, ...) and main = (M, M^-1) as the library makes them (default: fuse_mirror's, which
        may differ from the library's in the last bit of an inverse -- the CPU tests compare the mirror with itself)"""
        mats = {s: fm.slot_matrices(self.cams[s]) for s in range(NSLOT)} if mats is None else mats
        main = fm.slot_matrices(self.main_cam) if main is None else main
        return cm.Term(main, [(mats[s][0], mats[s][1], self.maps[s]) for s in slots], weight, max_px)


@functools.lru_cache(maxsize=None)
def crafted():
    return Crafted()


@functools.lru_cache(maxsize=None)
def clause_counts(max_px=MAX_PX):
    """per clause of rule 5 the (pixel, listed neighbour) pairs of the start map that end there, over the frame and over the first tile;
    and the same per listed neighbour -> (counts [6], counts of the first tile [6], per neighbour [8, 6])"""
    c = crafted()
    rows, cols = np.nonzero(pm.inside(c.start))
    clause = c.term(max_px=max_px).evaluate(rows, cols, c.start[rows, cols], H, W)[2]
    tile = (rows < TILE_H) & (cols < TILE_W)
    count = lambda x: np.bincount(x.reshape(-1), minlength=6)
    return count(clause), count(clause[tile]), np.stack([count(clause[:, j]) for j in range(len(SLOTS))])


def scene(oracle, gate=None):
    """propagate_mirror.Scene of the crafted case, or gated_mirror.Scene under gate = (tau, guide)"""
    c = crafted()
    return pm.Scene(oracle, *c.views()) if gate is None else gm.Scene(oracle, *c.views(), tau=gate[0], guide=gate[1])


def snapshot(state):
    out = pc.snapshot(state) + (state.support(),)
    out[-1].setflags(write=False)
    return out


_SHOTS = {}


def shots(cost, r, keep, gate=None, mats=None, main=None, slots=SLOTS, weight=WEIGHT, max_px=MAX_PX, nrandom=2, key=None):
    """the mirror on the crafted case -> snapshots (z, gx, gy, cells, cost map, report, support) after init, after run(1) and after
    another run(1); gate: None or "crafted" (tau 20 on gated_cases' crafted guide).  `key` names the matrices (None: fuse_mirror's)"""
    import orc
    k = (cost, r, keep, gate, key, tuple(slots), float(weight), float(max_px), nrandom)
    assert (mats is None) == (key is None)
    if k not in _SHOTS:
        c = crafted()
        g = None if gate is None else (gc.TAU, gc.crafted_guide())
        term = c.term(mats, main, slots, weight, max_px) if len(slots) else None
        state = cm.State(scene(orc.load(), g), c.start, cost, r, keep, term=term)
        out = [snapshot(state)]
        for _ in range(2):
            state.run(1, DZ, DG, nrandom, SEED)
            out.append(snapshot(state))
        _SHOTS[k] = out
    return _SHOTS[k]


# ---- the occluder scene (sections 22, 25, 26) -----------------------------------------------------------------------------------------
def ring_center(s, v):
    a = 2.0 * np.pi * v / s.V
    return [s.RING * np.cos(a), s.RING * np.sin(a), 0.0]


@functools.lru_cache(maxsize=None)
def analytic_neighbours(name):
    """per side view of the scene: (P, P^-1, the analytic depth map of its camera)"""
    s = gc.scene(name)
    out = []
    for v in range(s.V):
        P, Pi, _ = fm.slot_matrices(s.side_cams[v])
        out.append((P.astype(f32), Pi.astype(f32), s.render(ring_center(s, v))[1]))
    return out


@functools.lru_cache(maxsize=None)
def estimated_neighbours(name, tau=255):
    """per side view of the scene: (P, P^-1, its depth map ESTIMATED the way the main view's is -- that view as the main one, the main
    view and the other side views beside it, section 25's start (16 planes, ZNCC r = 2, keep 2, refined), 3 iterations without random
    candidates under the gate tau)"""
    import orc
    s, oracle = gc.scene(name), orc.load()
    cams, imgs = [s.main_cam] + list(s.side_cams), [s.main_img] + list(s.sides)
    out = []
    for v in range(1, s.V + 1):
        others = [i for i in range(s.V + 1) if i != v]
        views = (cams[v], imgs[v], np.stack([cams[i] for i in others]), [imgs[i] for i in others])
        z = oracle.plane_table(16, s.z_lo, s.z_hi)
        vol = gm.bm.volume(oracle, ZNCC, *views, 16, s.z_lo, s.z_hi, 2, 2)
        start = oracle.refine_depth(vol, z, oracle.argmin(vol, z, sampler="fixed")[2], sampler="fixed")
        state = pm.State(gm.Scene(oracle, *views, tau=tau), start, ZNCC, 2, 2).run(3, 0.0, 0.0, 0, 0)
        P, Pi, _ = fm.slot_matrices(cams[v])
        out.append((P.astype(f32), Pi.astype(f32), state.z))
    return out


@functools.lru_cache(maxsize=None)
def consistent(name, neighbours, weight, max_px=3.0, tau=255):
    """section 25's run on a scene (from propagation_start, ZNCC r = 2, keep 2, 3 iterations without random candidates, gate tau) with the
    term on `neighbours` ("analytic" or "estimated") -> (z, support)"""
    import orc
    s = gc.scene(name)
    nb = analytic_neighbours(name) if neighbours == "analytic" else estimated_neighbours(name, tau)
    term = cm.Term(fm.slot_matrices(s.main_cam), nb, weight, max_px)
    state = cm.State(gm.Scene(orc.load(), *s.views(), tau=tau), gc.propagation_start(name), ZNCC, 2, 2, term=term).run(3, 0.0, 0.0, 0, 0)
    out = state.z, state.support()
    _frozen(*out)
    return out
