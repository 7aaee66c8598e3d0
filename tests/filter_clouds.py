"""Crafted clouds for the point filter (csrc/filter.hip against oracle/filter_oracle.c), shared by tests/test_filter_cases_cpu.py
and tests/test_filter_cases_gpu.py.  Each case is small enough for tests/filter_mirror.py (except the key-width clouds of group
C, which are checked against the oracle only), names the defects of filter_mirror.DEFECTS it is there for and carries its
premise -- what must be true of the cloud for the case to test what it says -- which the CPU file asserts.

Coordinates and radii are dyadic where the case allows (alpha = 1: radius 0.25, cell side 0.5 up to the library's 2^-18 pad),
so cells and weights can be read off the numbers."""
from collections import namedtuple

import numpy as np

import filter_mirror as fm

f32 = np.float32

# premise keys: iterations, chain_gt, clamped (densities at exactly 2.0), distinct (distinct densities), kept, density (exact list),
# all_nan, split (pairs (i, j) the oracle accepts that the committed arithmetic puts two cells apart), cells (point -> fixed cell),
# same_bucket (pairs of points in different cells of one bucket), shared_27 (point whose 27 cells share a bucket, partner in one of them)
Case = namedtuple("Case", "name group points alpha defects premise mirror")


def _h(xyz, w=1.0):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.concatenate([xyz * w, np.full((len(xyz), 1), w)], 1).astype(f32)


def _case(name, group, points, alpha, defects=(), mirror=True, **premise):
    return Case(name, group, np.ascontiguousarray(points, f32), float(f32(alpha)), tuple(defects), premise, mirror)


# ---- A: neighbour grid ----------------------------------------------------------------------------------------------
def _seam_26(base, scale):
    """a centre in the middle of cell `base` (in cells of side 0.5 * scale) and one partner in each of the 26 cells around it, 9/32 of a
    unit away per axis: d2 <= 3 * 81 / 1024 < 0.25"""
    centre = (np.asarray(base, np.float64) + 0.5) * 0.5
    pts = [centre] + [centre + 0.28125 * np.array(d) for d in fm.NEIGHBOUR_CELLS if d != (0, 0, 0)]
    return _h(np.array(pts) * scale)


def _group_a():
    out = []
    for where, base in (("positive", (2, 3, 4)), ("negative", (-3, -4, -5)), ("straddle", (0, -1, 0))):
        for alpha, scale in ((1.0, 1.0), (0.02, None)):
            # the scaled build: the same figure in units of the cell of alpha = 0.02 (sqrt(0.005) is not dyadic: 9/32 of 0.99 cells per axis)
            s = 1.0 if scale else 0.99 * 2.0 * float(np.sqrt(f32(alpha) / f32(4)))
            pts = _seam_26(base, s)
            out.append(_case("seam_26_%s_a%g" % (where, alpha), "A", pts[::-1].copy(), alpha, ["skip_cell", "bucket_any"],
                             cells={26: tuple(base)}, centre=26))
    for alpha in (0.02, 0.05, 0.2):
        cell = np.sqrt(f32(alpha) / f32(4))                   # sqrtf(radius): fl(cell * cell) <= radius, and fl(cell - -1e-30) = cell
        out.append(_case("straddle_origin_a%g" % alpha, "A", [[-1e-30, 0, 0, 1], [cell, 0, 0, 1]], alpha, density=[1.0, 1.0], split=[(1, 0)], kept=0))
    # consecutive floats at cell index 2^23: fl(x * inv_cell) is off by up to half a cell there
    out.append(_case("large_index_pair", "A", _h([[2717108.75, 0, 0], [2717109.0, 0, 0]]), 0.41965678, density=[1.0, 1.0], split=[(1, 0)]))
    out.append(_case("large_index_path12", "A", _h([[2717108.0 + 0.25 * k, 0, 0] for k in range(12)]), 0.41965678, pairs=11))
    # found by scanning radii with filter_mirror.cells(..., "committed") for an accepted pair on either side of cell index 2^k
    for k, alpha, xa, xb in ((18, 0.24316129088401794, 64633.421875, 64633.66796875), (21, 0.8018807172775269, 938976.625, 938977.0625),
                             (22, 0.6163926124572754, 1646488.25, 1646488.625)):
        out.append(_case("large_index_2p%d" % k, "A", _h([[xa, 1.0, -2.0], [xb, 1.0, -2.0]]), alpha, density=[1.0, 1.0], split=[(1, 0)],
                         index_near=2 ** k))
    out.append(_hash_alias())
    rng = np.random.default_rng(7)
    cluster = rng.integers(-8, 9, (20, 3)) / 16.0              # dyadic, within +-0.5 of the origin
    far = np.array([[1e12, 1e12, 1e12], [1e12, 1e12, 1e12], [2e12, 2e12, 2e12]])
    out.append(_case("far_clamp", "A", _h(np.concatenate([far, cluster])), 1.0, cells={0: (10 ** 9,) * 3, 1: (10 ** 9,) * 3, 2: (10 ** 9,) * 3},
                     far_pair=(1, 0)))
    pts = np.concatenate([_h(cluster[:5], 2.0), _h(cluster[5:10], 0.5), _h(cluster[10:15], -1.0), _h(cluster[15:]),
                          np.array([[1, 2, 3, 0], [0, 0, 0, 0]], f32)])
    out.append(_case("homogeneous", "A", pts, 1.0, zero_density=[20, 21]))
    return out


def _hash_alias():
    """at alpha = 1 (cells of side ~0.5): a cluster in cell (0, 0, 0), a second one in the nearest cell (k, 0, 0), k > 8, of the same bucket
    at this N, and a pair in cells a and a + (1, 0, 0) where another of a's 27 cells shares the partner's bucket"""
    N = 12
    mask = fm.table_size(N) - 1
    k = next(k for k in range(9, 4096) if fm.cell_hash((k, 0, 0), mask) == fm.cell_hash((0, 0, 0), mask))
    a = None
    for ax in range(20, 4096):                                 # cell a whose +x neighbour shares a bucket with another of a's 27 cells
        hs = [fm.cell_hash((ax + dx, 40 + dy, dz), mask) for dx, dy, dz in fm.NEIGHBOUR_CELLS]
        if hs.count(hs[fm.NEIGHBOUR_CELLS.index((1, 0, 0))]) >= 2:
            a = (ax, 40, 0)
            break
    c0 = np.array([[0.25, 0.25, 0.25], [0.125, 0.25, 0.375], [0.375, 0.125, 0.25], [0.25, 0.375, 0.125], [0.3125, 0.25, 0.25]])
    shift = np.array([0.5 * k + 0.0625, 0, 0])                # + 1/16: clear of the padded cell boundary at 0.5 k (1 + 2^-18)
    pa = (np.array(a) + 0.5) * 0.5 + np.array([0.0625, 0.0625, 0.0625])
    pts = np.concatenate([c0, c0 + shift, [pa + [0.375, 0, 0], pa]])
    return _case("hash_alias", "A", _h(pts), 1.0, ["bucket_any", "skip_cell"], same_bucket=[(0, 5)], shared_27=(11, 10), cells={0: (0, 0, 0), 5: (k, 0, 0), 11: a})


# ---- B: power iteration ---------------------------------------------------------------------------------------------
def _random(seed, n, lo=-1.0, hi=1.0):
    return _h(np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(f32))


def _group_b():
    out = [_case("coincident50", "B", np.tile(np.array([[0.5, 0.5, 0.5, 1.0]], f32), (50, 1)), 0.04, ["ties_desc"], iterations=1, kept=50),
           _case("path3", "B", _h([[0, 0, 0], [0.375, 0, 0], [0.75, 0, 0]]), 1.0, ["iter_plus", "iter_minus"], iterations=200, density=[1.0, 1.0, 1.0], kept=0),
           _case("path4", "B", _h([[0.375 * k, 0, 0] for k in range(4)]), 1.0, ["iter_plus", "iter_minus"], iterations=8, keep=[1, 2])]
    rng = np.random.default_rng(1)                             # drawn in this order: 15, 27, 73, 87, 61, 32 iterations
    for n in (40, 80):
        for alpha in (0.3, 0.6, 1.0):
            pts = _h(rng.uniform(-1, 1, (n, 3)))
            # the three denser ones have lists long enough for the order of their float additions to show
            out.append(_case("random_n%d_a%g" % (n, alpha), "B", pts, alpha, ["iter_plus", "iter_minus"] + (["desc_lists"] if n * alpha >= 40 else [])))
    rng = np.random.default_rng(0)
    pts = _h(np.concatenate([rng.normal(0, 0.02, (60, 3)), rng.uniform(-1, 1, (60, 3))]))
    out.append(_case("clamp", "B", pts, 0.3, ["no_clamp", "desc_lists"], clamped=33))
    out.append(_case("all_isolated", "B", _h([[3.0 * k, -2.0 * k, 1.0 * k] for k in range(7)]), 1.0, all_nan=True, kept=0, pairs=0))
    for n in (1, 2, 255, 256, 257):                             # chunk_sums: one element per chunk up to 256, two from 257 on, empty chunks
        box = 0.6 * max(n, 2) ** (1.0 / 3.0)                    # ~ constant density: a handful of neighbours per point at alpha = 1
        out.append(_case("count_%d" % n, "B", _random(100 + n, n, -box / 2, box / 2), 1.0, all_nan=(n == 1)))
    return out


# ---- C: order and greedy pass ---------------------------------------------------------------------------------------
def _group_c():
    g = np.array([-0.375, -0.125, 0.125, 0.375])
    lattice = _h([[x, y, z] for z in g for y in g for x in g])
    perms = {"identity": np.arange(64), "reversed": np.arange(64)[::-1], "shuffled": np.random.default_rng(64).permutation(64)}
    # 62 kept in lattice order; only lower-index neighbours are penalised, so the count follows the permutation (tests compare with the oracle)
    out = [_case("lattice64_" + name, "C", lattice[p], 1.0, ["ties_desc"] if name == "shuffled" else [], distinct=11, **({"kept": 62} if name == "identity" else {}))
           for name, p in perms.items()]
    m = 12                                                      # a path of 2 m points indexed from both ends towards the middle: the density
    xs = [0.375 * i for i in range(m)] + [0.375 * (2 * m - 1 - i) for i in range(m)]   # rises with the index along each half
    out.append(_case("chain", "C", _h([[x, 0, 0] for x in xs]), 1.0, ["ties_desc"], chain_gt=8))
    for n in (256, 257, 1024, 1025):                            # key_bits of the list sorts: 40, 41, 42, 43
        out.append(_case("keys_%d" % n, "C", _random(n, n, 0.0, 0.45 * n ** (1.0 / 3.0)), 1.0, mirror=False))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _group_a() + _group_b() + _group_c()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def by_name(name):
    return next(c for c in cases() if c.name == name)
