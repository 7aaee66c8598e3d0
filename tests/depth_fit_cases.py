"""Crafted depth maps for the depth-map plane fit: every case is a map, a guide and the arguments of one
mvs_depth_fit call, built to sit on an edge of the contract or of the kernel.  tests/test_depth_fit_cpu.py holds the mirror's two
statements against each other on them and shows that each rule decides the bytes of a named case; tests/test_depth_fit_gpu.py runs them
on the device.  The maps the filter's cases share (a noisy slanted surface with a step and holes of every invalid kind, the map of every
kind of value, the gates' map, the tile seams' map) come from tests/depth_filter_cases.py."""
import collections
import functools

import numpy as np

import depth_filter_cases as dc
import depth_fit_mirror as fm

f32 = np.float32
RADII = (1, 2, 3, 4)
TILE = (32, 8)       # csrc/depth_fit.hip: FT_TW, FT_TH
INF = float("inf")
FULL_D = 23619600    # D of a full radius-4 window: 81 * 540 * 540, above 2^24

Case = collections.namedtuple("Case", "name depth guide radius tau max_step min_members")
_frozen = dc._frozen


def reference(case, mirror=fm):
    return _reference(case.name) if mirror is fm else run(case, mirror)


def run(case, mirror=fm, dtype=f32):
    return mirror.fit(case.depth, case.radius, case.tau, case.max_step, case.min_members, case.guide, dtype)


@functools.lru_cache(maxsize=None)
def _reference(name):
    res = run(by_name(name))
    for a in res[:5] + (res.c,):
        a.flags.writeable = False
    return res


def slanted(W, H, seed, noise=0.002, gx=0.004, gy=-0.003, z0=-0.2):
    """a plane with noise, no holes; every value is valid"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    return _frozen((z0 + gx * x + gy * y + rng.uniform(-noise, noise, (H, W))).astype(f32))


def _count_map(k):
    """9 x 9, invalid but for the centre (4, 4) and k - 1 pixels of its 3 x 3 window, no three of the first three on a line"""
    z = np.full((9, 9), np.nan, f32)
    ring = [(4, 4), (3, 3), (3, 4), (5, 5), (4, 3), (5, 3), (3, 5), (4, 5), (5, 4)]
    for i, (r, c) in enumerate(ring[:k]):
        z[r, c] = f32(0.1 + 0.013 * i * i - 0.02 * i)
    return _frozen(z)


def _collinear_guide(kind, W, H):
    """a guide whose levels are 20 apart between the lines of one direction: under tau = 5 only the pixels of p's own row, column or
    diagonal are members, and D = 0"""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    line = {"row": y, "column": x, "diagonal": (x - y) % 12}[kind]
    return _frozen((20 * line).astype(np.uint8))


def _range_map(sign):
    """5 x 5, invalid but for the four pixels of the top left corner, all dyadic: at (0, 0) with radius 1 the plane through them has
    c = (t(0,1) + t(1,0) - t(1,1)) / 4 = 0.5 exactly, so z + c = sign * 1.0 exactly: AT the bound of the open range"""
    z = np.full((5, 5), np.nan, f32)
    z[0, 0], z[0, 1], z[1, 0], z[1, 1] = 0.5, 0.9375, 0.9375, -0.625
    return _frozen((sign * z).astype(f32))


def _line_map(sign):
    """5 x 5, every row the same steep convex profile: the least-squares line of a radius-4 window reaches sign * 1.154 at column 0,
    BEYOND the range, and stays inside it at the other columns"""
    return _frozen((sign * np.tile(np.array([0.99, 0.9, 0.6, 0.3, -0.4]), (5, 1))).astype(f32))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    z, g = dc.surface(37, 19, 0xDF00)            # one tile and a part of the next, both ways; borders and corners with Sx, Sy, Sxy != 0
    for r in RADII:
        out.append(Case("plain_r%d" % r, z, None, r, 255, INF, 6))
        out.append(Case("gated_r%d" % r, z, g, r, 12, f32(0.04), 6))
    for W, H, r in ((9, 5, 4), (TILE[0], TILE[1], 2), (TILE[0] + 1, TILE[1], 3), (TILE[0] - 1, TILE[1], 4), (TILE[0], TILE[1] + 1, 4),
                    (TILE[0], TILE[1] - 1, 3)):
        z, g = dc.surface(W, H, 0xDF10 + W + 64 * H)
        out.append(Case("size_%dx%d" % (W, H), z, g, r, 20, f32(0.05), 4))
    z, g = dc._seam_map()                        # 64 x 16: holes, a depth step and a guide edge on the tile seams
    out.append(Case("seams_gated", z, g, 4, 25, f32(0.06), 5))
    out.append(Case("seams_plain", z, g, 3, 255, f32(0.06), 3))
    out.append(Case("seams_no_gate", z, g, 4, 255, INF, 6))
    z, g = dc._values_map()                      # every kind of value next to each other
    out.append(Case("values_r1", z, g, 1, 255, INF, 3))
    out.append(Case("values_r2", z, g, 2, 255, f32(0.5), 4))
    out.append(Case("values_gated", z, g, 2, 64, f32(0.5), 3))
    out.append(Case("all_invalid", _frozen(np.full((11, 35), np.nan, f32)), _frozen(np.zeros((11, 35), np.uint8)), 2, 255, INF, 3))
    one = np.full((11, 35), 1.0, f32)
    one[8, 33] = f32(-0.625)
    out.append(Case("one_valid", _frozen(one), None, 3, 255, INF, 3))
    z, g, step = dc._gate_map()                  # around (5, 5): guide values tau and tau + 1 away, depths max_step and one ulp more away
    out.append(Case("gate_on", z, g, 1, 17, step, 3))
    out.append(Case("gate_tau_below", z, g, 1, 16, step, 3))
    out.append(Case("gate_step_below", z, g, 1, 17, np.nextafter(step, f32(0.0)), 3))
    out.append(Case("gate_tau0", z, g, 2, 0, INF, 3))
    out.append(Case("gate_step0", z, g, 2, 255, f32(0.0), 3))
    out.append(Case("gate_step_inf", z, g, 2, 255, INF, 3))
    out.append(Case("gate_tau255_no_guide", z, None, 2, 255, step, 3))
    for k in (3, 6, 9):
        out.append(Case("count_%d_of_%d" % (k, k), _count_map(k), None, 1, 255, INF, k))           # n = min_members: fitted
        out.append(Case("count_%d_of_%d" % (k, k + 1), _count_map(k), None, 1, 255, INF, k + 1))   # one less: refused
    z = slanted(13, 9, 0xF170)
    for kind in ("row", "column", "diagonal"):
        out.append(Case("collinear_" + kind, z, _collinear_guide(kind, 13, 9), 2, 5, INF, 3))
    z = slanted(19, 13, 0xF171)                  # the pixels 4 and more from the border have all 81 members
    out.append(Case("full_r4", z, None, 4, 255, INF, 81))
    out.append(Case("full_r4_min80", z, None, 4, 255, INF, 80))
    out.append(Case("range_above", _range_map(1.0), None, 1, 255, INF, 3))
    out.append(Case("range_below", _range_map(-1.0), None, 1, 255, INF, 3))
    out.append(Case("range_line_above", _line_map(1.0), None, 4, 255, INF, 3))
    out.append(Case("range_line_below", _line_map(-1.0), None, 4, 255, INF, 3))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return {c.name: c for c in cases()}[name]


def seeded_state(scene, depth, cost, r, keep, seed_gx, seed_gy):
    """propagate_mirror's init with the slopes mvs_propagate_set_slopes recorded injected: behind rule 5's copy a pixel with a hypothesis
    takes the caller's slopes (a non-finite value as 0), a pixel without one keeps 0; then the cells are evaluated as always"""
    import propagate_mirror as pm

    class SeededState(pm.State):
        def __init__(self):
            self.scene, self.cost, self.r, self.keep = scene, cost, r, keep
            self.views = range(len(scene.sides))
            self.z = pm.seed_maps(depth)[0]
            has = pm.inside(self.z)
            self.gx, self.gy = (np.where(has & np.isfinite(g), g, f32(0.0)).astype(f32) for g in (np.asarray(seed_gx, f32), np.asarray(seed_gy, f32)))
            rows, cols = (a.reshape(-1) for a in np.indices(self.z.shape))
            self.cells = self._eval(rows, cols, self.z.reshape(-1), self.gx.reshape(-1), self.gy.reshape(-1)).reshape(self.z.shape)
            self.t, self.counters, self.wins, self.ties, self.no_random = 0, [0, 0, 0, 0], [], 0, 0

    return SeededState()
