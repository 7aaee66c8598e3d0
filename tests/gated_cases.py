"""Inputs of the guide-gated windows' tests (tests/test_gated_cpu.py, tests/test_gated_gpu.py): the crafted guide on section 22's crafted
case, the contrast scene, and the mirror's results on them.  Everything is computed once, shared and read-only."""
import functools

import numpy as np

import bestk_cases as bk
import gated_mirror as gm

ABSDIFF, ZNCC, KEEP_ALL = gm.COST_ABSDIFF, gm.COST_ZNCC, gm.KEEP_ALL
NAMES = bk.NAMES
COST_RADII = [(ABSDIFF, 1), (ABSDIFF, 2), (ABSDIFF, 4), (ZNCC, 1), (ZNCC, 2), (ZNCC, 4)]
KEEPS = (KEEP_ALL, 1, 2, 8)
RANGES = bk.RANGES                    # (view_first, view_count) of the crafted case
TAU = 20                              # the crafted tau
TAUS = (0, TAU, 255)
LEVELS = (50, 70, 91, 111, 132, 152)  # the blocks' grey levels: neighbours in this list are TAU and TAU + 1 apart in turn
LONE = 250                            # isolated single pixels: further than TAU from every level
ROW_EDGES = (0, 2, 9, 12, 16, 18)     # blocks begin here: rows 2 and 9 bound the main image's constant block, 16 is the tile seam, 18 the last row
COL_EDGES = (0, 5, 9, 14, 19, 23, 28, 32, 37, 41, 46, 50, 54, 57, 61, 64, 69)   # 5 and 14 bound the constant block, 32 and 64 are the tile seams, 69 is the last column
LONE_AT = ((0, 0), (5, 27), (12, 32), (16, 45), (12, 60), (18, 69))   # more than 4 pixels apart; on both seams and in two corners


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def block_guide(W, H, row_edges, col_edges, lone=()):
    """a piecewise constant guide: block (i, j) holds LEVELS[(j + 3 i) % 6], so that a horizontal neighbour is TAU or TAU + 1 away (or
    102 at the wrap) and a vertical one at least 61; the pixels `lone` hold LONE"""
    bi = np.searchsorted(np.asarray(row_edges), np.arange(H), side="right") - 1
    bj = np.searchsorted(np.asarray(col_edges), np.arange(W), side="right") - 1
    g = np.asarray(LEVELS, np.uint8)[(bj[None, :] + 3 * bi[:, None]) % 6]
    for row, col in lone:
        g[row, col] = LONE
    return np.ascontiguousarray(g)


@functools.lru_cache(maxsize=None)
def crafted():
    return bk.crafted()


@functools.lru_cache(maxsize=None)
def crafted_guide():
    c = crafted()
    g = block_guide(c.W, c.H, ROW_EDGES, COL_EDGES, LONE_AT)
    _frozen(g)
    return g


@functools.lru_cache(maxsize=None)
def constant_guide():
    c = crafted()
    g = np.full((c.H, c.W), 93, np.uint8)
    _frozen(g)
    return g


def guide_of(name):
    """"main" -> None (the staged main image), "crafted", "constant" """
    return {"main": lambda: None, "crafted": crafted_guide, "constant": constant_guide}[name]()


@functools.lru_cache(maxsize=None)
def crafted_raw(cost, v):
    import orc
    if v == bk.Crafted.V - 1:
        return crafted_raw(cost, 0)           # view 5 is view 0 again
    c, oracle = crafted(), orc.load()
    out = gm.raw_view(oracle, cost, c.main_cam, c.main_img, c.side_cams[v], c.sides[v], c.D, c.Z_LO, c.Z_HI)
    _frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def crafted_gate(guide, tau, r):
    g = guide_of(guide)
    out = gm.gates(crafted().main_img if g is None else g, tau, r)
    _frozen(out)
    return out


@functools.lru_cache(maxsize=None)
def crafted_view(cost, r, tau, guide, v):
    """the mirror on view v of the crafted case -> (counted, c), [D, H, W] each; guide: "main", "crafted" or "constant" """
    if v == bk.Crafted.V - 1:
        return crafted_view(cost, r, tau, guide, 0)
    out = gm.view_costs(cost, crafted().main_img, crafted_raw(cost, v), crafted_gate(guide, tau, r), r)
    _frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def _crafted_volume(cost, r, keep, tau, guide, views):
    c = crafted()
    vol = gm.bm.merge([crafted_view(cost, r, tau, guide, v) for v in views], keep, (c.D, c.H, c.W))
    _frozen(vol)
    return vol


def crafted_volume(cost, r, keep, tau, guide="crafted", views=None):
    """the mirror's volume of the crafted case (over the side views `views`, default all)"""
    return _crafted_volume(cost, r, keep, tau, guide, tuple(range(bk.Crafted.V)) if views is None else tuple(views))


maps = bk.maps


class Contrast(bk.Occluder):
    """bestk_cases.Occluder with an intensity edge on the depth step: after the parent's rounding to u8, f = img as float64 and
    img = clip(rint(where(front, 150 + 0.4 f, 10 + 0.4 f))).  The main image's means are 200 on the rectangle and 61 off it"""

    def render(self, center):
        img, zn, front = super().render(center)
        f = img.astype(np.float64)
        img = np.clip(np.rint(np.where(front, 150.0 + 0.4 * f, 10.0 + 0.4 * f)), 0, 255).astype(np.uint8)
        return img, zn, front


@functools.lru_cache(maxsize=None)
def scene(name, V=4):
    """"occluder": bestk_cases.occluder(V) as it is; "contrast": Contrast(V)"""
    return bk.occluder(V) if name == "occluder" else Contrast(V)


@functools.lru_cache(maxsize=None)
def scene_raw(name, cost, D):
    import orc
    s, oracle = scene(name), orc.load()
    out = tuple(gm.raw_view(oracle, cost, s.main_cam, s.main_img, s.side_cams[v], s.sides[v], D, s.z_lo, s.z_hi) for v in range(s.V))
    for p in out:
        _frozen(*p)
    return out


@functools.lru_cache(maxsize=None)
def scene_views(name, cost, r, D, tau):
    """the mirror's gated per-view costs of a scene over D planes, the guide its main image -> a tuple of (counted, c)"""
    s = scene(name)
    gate = gm.gates(s.main_img, tau, r)
    out = tuple(gm.view_costs(cost, s.main_img, raw, gate, r) for raw in scene_raw(name, cost, D))
    for p in out:
        _frozen(*p)
    return out


@functools.lru_cache(maxsize=None)
def scene_volume(name, cost, r, D, keep, tau):
    s = scene(name)
    vol = gm.bm.merge(scene_views(name, cost, r, D, tau), keep, (D, s.H, s.W))
    _frozen(vol)
    return vol


def bad_shares(oracle, name, depth, D):
    """(share of pixels more than 1.5 steps of a D-plane table from the analytic depth over the whole image, over the edge pixels), in %"""
    s = scene(name)
    bad = np.abs(depth - s.truth) > 1.5 * (s.z_hi - s.z_lo) / D
    return 100.0 * float(bad.mean()), 100.0 * float(bad[s.edge].mean())


def wta_shares(oracle, name, vol, D):
    """winner-take-all on a scene's volume -> bad_shares"""
    s = scene(name)
    return bad_shares(oracle, name, oracle.argmin(vol, oracle.plane_table(D, s.z_lo, s.z_hi), sampler="fixed")[0], D)


@functools.lru_cache(maxsize=None)
def propagation_start(name):
    """the UNGATED start of section 25's occluder table on a scene: ZNCC r = 2, keep 2, 16 planes, selected and refined"""
    import orc
    s, oracle = scene(name), orc.load()
    z = oracle.plane_table(16, s.z_lo, s.z_hi)
    vol = gm.bm.volume(oracle, ZNCC, *s.views(), 16, s.z_lo, s.z_hi, 2, 2)
    start = oracle.refine_depth(vol, z, oracle.argmin(vol, z, sampler="fixed")[2], sampler="fixed")
    start.setflags(write=False)
    return start


@functools.lru_cache(maxsize=None)
def propagated(name, tau, random):
    """3 iterations from propagation_start, ZNCC r = 2, keep 2, under the gate tau on the main image; random: dz half a coarse step, dg
    an eighth, nrandom 3 -- else no random candidates -> the z map"""
    import orc
    s = scene(name)
    coarse = (s.z_hi - s.z_lo) / 16
    state = gm.pm.State(gm.Scene(orc.load(), *s.views(), tau=tau), propagation_start(name), ZNCC, 2, 2)
    state.run(3, 0.5 * coarse, 0.125 * coarse, 3, 0) if random else state.run(3, 0.0, 0.0, 0, 0)
    state.z.setflags(write=False)
    return state.z
