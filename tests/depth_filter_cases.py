"""Crafted depth maps for the depth-map filter: every case is a map, a guide and the arguments of one
mvs_depth_filter call, built to sit on an edge of the contract or of the kernel.  tests/test_depth_filter_cpu.py holds the mirror's two
statements against each other on them and shows that each rule decides the bytes of a named case; tests/test_depth_filter_gpu.py runs
them on the device."""
import collections
import functools

import numpy as np

import depth_filter_mirror as dm

f32 = np.float32
MEDIAN, MEAN, FILL = dm.MEDIAN, dm.MEAN, dm.FILL
FLAG_SETS = (MEDIAN, MEAN, MEDIAN | MEAN, MEDIAN | FILL, MEDIAN | MEAN | FILL)   # every combination the call accepts
RADII = (1, 2, 3, 4)
TILE = (32, 8)       # csrc/depth_filter.hip: DF_TW, DF_TH
INF = float("inf")
BELOW_ONE, ABOVE_MINUS_ONE = np.nextafter(f32(1.0), f32(0.0)), np.nextafter(f32(-1.0), f32(0.0))
TINY = np.nextafter(f32(0.0), f32(1.0))      # the smallest denormal

Case = collections.namedtuple("Case", "name depth guide radius tau max_step flags min_members")


def _frozen(a):
    a.flags.writeable = False
    return a


def reference(case):
    return _reference(case.name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = by_name(name)
    return _frozen(dm.filter(c.depth, c.radius, c.tau, c.max_step, c.guide, c.flags, c.min_members))


def surface(W, H, seed, holes=0.12):
    """a slanted surface with a depth step at mid-width, plane-step noise, a quarter of it quantised (runs of equal values), holes of every
    invalid kind; the guide has its own edge, a few columns off the depth step, and noise of a few grey levels"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    z = 0.30 * x / max(W, 1) - 0.20 * y / max(H, 1) + 0.25 * (x >= W // 2) - 0.3 + rng.normal(0.0, 0.01, (H, W))
    z = np.where((x + y) % 4 == 0, np.round(z * 16) / 16, z).astype(f32)
    kinds = np.array([1.0, np.nan, np.inf, -np.inf, -1.0, 1.5, -2.0], f32)
    hole = rng.random((H, W)) < holes
    z = np.where(hole, kinds[rng.integers(0, len(kinds), (H, W))], z).astype(f32)
    g = 60 + 120 * (x >= W // 2 + 2) + rng.integers(-6, 7, (H, W))
    return _frozen(z), _frozen(np.clip(g, 0, 255).astype(np.uint8))


def _values_map():
    """13 x 9: every kind of value next to each other"""
    rng = np.random.Generator(np.random.PCG64(0xDF01))
    z = rng.uniform(-0.9, 0.9, (9, 13)).astype(f32)
    z[0, :7] = [np.nan, np.inf, -np.inf, -1.0, 1.0, BELOW_ONE, ABOVE_MINUS_ONE]
    z[1, :6] = [-0.0, 0.0, TINY, -TINY, f32(1e-40), f32(-1e-40)]
    z[2, :] = f32(0.25)                       # a run of equal values
    z[3, ::2] = f32(0.25)
    z[4, 3:9] = [-0.0, -0.0, 0.0, -0.0, TINY, -TINY]
    z[6:, 8:] = np.nan
    z[7, 10] = -0.0                           # one valid pixel, a negative zero, alone in its 3 x 3 window
    g = rng.integers(0, 256, (9, 13)).astype(np.uint8)
    return _frozen(z), _frozen(g)


def _gate_map():
    """11 x 11 around the centre pixel (5, 5): guide values exactly tau and tau + 1 away on either side, depths exactly max_step and one
    ulp more away; max_step is the mirror's own |m(q) - m(p)|"""
    z = np.full((11, 11), np.nan, f32)
    g = np.full((11, 11), 100, np.uint8)
    z[5, 5] = f32(0.1)
    z[5, 6] = f32(0.1) + f32(0.0123)          # exactly on max_step
    z[5, 4] = np.nextafter(z[5, 6], f32(1.0))  # one ulp beyond
    z[4, 5] = f32(0.093)
    z[6, 5] = f32(0.1)
    z[4, 4], z[6, 6], z[4, 6], z[6, 4] = f32(0.112), f32(0.094), f32(0.107), f32(0.0905)
    g[4, 4], g[6, 6], g[4, 6], g[6, 4] = 100 + 17, 100 - 17, 100 + 18, 100 - 18    # tau = 17: on it, on it, beyond, beyond
    step = abs(f32(z[5, 6] - z[5, 5]))
    return _frozen(z), _frozen(g), step


def _fill_map(k):
    """9 x 9, invalid but for k valid pixels around the invalid centre (4, 4)"""
    z = np.full((9, 9), 1.0, f32)
    ring = [(3, 3), (3, 4), (3, 5), (4, 3), (4, 5), (5, 3), (5, 4), (5, 5)]
    for i, (r, c) in enumerate(ring[:k]):
        z[r, c] = f32(0.1 * (i + 1) - 0.5)
    return _frozen(z), _frozen(np.full((9, 9), 7, np.uint8))


def _seam_map():
    """two tiles each way; holes, a depth step and a guide edge on the tile seams (columns 31 | 32, rows 7 | 8)"""
    W, H = 2 * TILE[0], 2 * TILE[1]
    z, g = surface(W, H, 0xDF5E, holes=0.05)
    z, g = z.copy(), g.copy()
    z[:, 32:] += f32(0.2)                     # the depth step on the vertical seam
    z[7, 5:20] = np.nan                       # holes along the horizontal seam, above and below
    z[8, 12:30] = 1.0
    z[3:12, 31] = np.inf
    g[8:, :] = np.clip(g[8:, :].astype(int) + 40, 0, 255).astype(np.uint8)   # a guide edge on the horizontal seam
    return _frozen(z.astype(f32)), _frozen(g)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    z, g = surface(37, 19, 0xDF00)            # one tile and a part of the next, both ways
    for flags in FLAG_SETS:
        for r in RADII:
            out.append(Case("flags%d_r%d" % (flags, r), z, g, r, 12, f32(0.04), flags, 3))
    for W, H, r in ((9, 5, 4), (TILE[0], TILE[1], 2), (TILE[0] + 1, TILE[1], 3), (TILE[0] - 1, TILE[1], 4), (TILE[0], TILE[1] + 1, 4),
                    (TILE[0], TILE[1] - 1, 3), (2, 2, 1), (2, 23, 2), (45, 2, 4)):      # (a context is 2 x 2 at the least)
        z, g = surface(W, H, 0xDF10 + W + 64 * H)
        out.append(Case("size_%dx%d" % (W, H), z, g, r, 20, f32(0.05), MEDIAN | MEAN | FILL, 2))
    z, g = _seam_map()
    out.append(Case("seams_median", z, g, 4, 25, INF, MEDIAN | FILL, 5))
    out.append(Case("seams_both", z, g, 3, 25, f32(0.06), MEDIAN | MEAN, 1))
    out.append(Case("seams_mean", z, g, 4, 255, f32(0.06), MEAN, 1))
    z, g = _values_map()
    for flags, name in ((MEDIAN, "median"), (MEAN, "mean"), (MEDIAN | MEAN | FILL, "all")):
        out.append(Case("values_%s_r1" % name, z, g, 1, 255, INF, flags, 1))
        out.append(Case("values_%s_r2" % name, z, g, 2, 255, f32(0.5), flags, 4))     # even and odd n along the invalid block's rim
    out.append(Case("values_gated", z, g, 2, 64, f32(0.5), MEDIAN | MEAN, 1))
    out.append(Case("all_invalid", _frozen(np.full((11, 35), np.nan, f32)), _frozen(np.zeros((11, 35), np.uint8)), 2, 255, INF, MEDIAN | MEAN | FILL, 1))
    one = np.full((11, 35), 1.0, f32)
    one[8, 33] = f32(-0.625)
    out.append(Case("one_valid", _frozen(one), _frozen(np.zeros((11, 35), np.uint8)), 3, 255, INF, MEDIAN | MEAN | FILL, 1))
    z, g, step = _gate_map()
    for flags, name in ((MEAN, "mean"), (MEDIAN, "median"), (MEDIAN | MEAN, "both")):
        out.append(Case("gate_%s_on" % name, z, g, 1, 17, step, flags, 1))
        out.append(Case("gate_%s_tau_below" % name, z, g, 1, 16, step, flags, 1))
        out.append(Case("gate_%s_step_below" % name, z, g, 1, 17, np.nextafter(step, f32(0.0)), flags, 1))
    out.append(Case("gate_tau0", z, g, 2, 0, INF, MEDIAN | MEAN, 1))
    out.append(Case("gate_step0", z, g, 2, 255, f32(0.0), MEAN, 1))
    out.append(Case("gate_step_inf", z, g, 2, 255, INF, MEAN, 1))
    out.append(Case("gate_tau255_no_guide", z, None, 2, 255, step, MEDIAN | MEAN, 1))
    for k in (3, 4, 8):
        z, g = _fill_map(k)
        out.append(Case("fill_%d_of_%d" % (k, k), z, g, 1, 255, INF, MEDIAN | FILL, k))            # n = min_members: filled
        out.append(Case("fill_%d_of_%d" % (k, k + 1), z, g, 1, 255, INF, MEDIAN | FILL, k + 1))    # one less: stays a hole
        out.append(Case("fill_%d_then_mean" % k, z, g, 1, 255, INF, MEDIAN | MEAN | FILL, k + 1))  # a hole the median leaves stays one
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return {c.name: c for c in cases()}[name]
