"""Crafted packed cost volumes for the semi-global aggregation, numpy only, and the table of cases that
tests/test_aggregate_edges_gpu.py hands to the kernels.  tests/test_aggregate_cpu.py checks with the mirror alone that every case does
what it is here for (which term of the recurrence wins where, how high the sums climb, which side of a floor boundary a cell lies on),
so that a generator that goes soft fails without a GPU.

Every generator returns uint32 [D, H, W] for cs = 24 (fixed sampler, cells count << 24 | sum) or 16 (exact sampler, count << 16 | sum)."""
import collections
import functools

import numpy as np

import sgm_mirror as sgm

CS = {"fixed": 24, "exact": 16}
CAP = 4080                      # the largest cost_cap: 16 * 255
STD = (8, 16, 128, CAP)         # (paths, P1, P2, cost_cap)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pack(n, s, cs):
    n, s = np.asarray(n, np.int64), np.asarray(s, np.int64)
    assert (s >= 0).all() and (s < (1 << cs)).all() and (n >= 0).all() and (n < (1 << (32 - cs))).all()
    return ((n << cs) | s).astype(np.uint32)


# the two special pixels of noise(): (y, x)
def nobody_sees(W, H):
    return H // 2, W // 2


def one_seen_cell(W, H):
    return 0, 0


def noise(W, H, D, cs, seed):
    """i.i.d. cells: counts 1..3 and about 10 % unseen; mean costs from 0 up to the cap (and, in a few cells, a sum past it); one cell in
    eight is free, which makes equal sums -- ties of the recurrence and of the selection -- common.  Pixel nobody_sees() has no seen
    cell, pixel one_seen_cell() has exactly one (plane 0)."""
    rng = _rng(seed)
    n = rng.integers(1, 4, (D, H, W))
    n[rng.random((D, H, W)) < 0.10] = 0
    per = 255 * 255 if cs == 24 else 255
    s = (rng.integers(0, per + 1, (D, H, W)) * n) // rng.integers(1, 40, (D, H, W))
    s[rng.random((D, H, W)) < 0.125] = 0
    past = rng.random((D, H, W)) < 0.02
    s[past] = (per * n[past] * 5) // 4       # a mean of 1.25 * 255 grey levels: only the cap keeps it at 4080
    y, x = nobody_sees(W, H)
    n[:, y, x] = 0
    y, x = one_seen_cell(W, H)
    n[0, y, x] = 2
    n[1:, y, x] = 0
    s[n == 0] = 0
    return _pack(n, s, cs)


def tri(t, D):
    """triangle wave over 0..D-1 with period 2 (D - 1)"""
    period = 2 * (D - 1)
    t = np.asarray(t) % period
    return np.where(t < D, t, period - t)


def ramp_surface(W, H, D, off):
    y, x = np.mgrid[0:H, 0:W]
    return tri(x + y // 2 + off, D)


def ramp_costs(W, H, D, off, slope=300):
    d = np.arange(D)[:, None, None]
    return np.minimum(CAP, slope * np.abs(d - ramp_surface(W, H, D, off)[None])).astype(np.int64)


def ramp(W, H, D, cs, off, slope=300):
    """a surface whose best plane d*(x, y) = tri(x + y // 2 + off) moves by one plane per pixel: C = min(cap, slope |d - d*|), so the
    +-P1 terms win along every path direction at the planes d* reaches.  Fixed sampler: n = 1, s = ceil(255 C / 16).  Exact sampler:
    floor(16 s / n) with n = 1 gives multiples of 16 only, so n = 16 and s = C."""
    C = ramp_costs(W, H, D, off, slope)
    if cs == 24:
        vol = _pack(np.ones_like(C), (255 * C + 15) // 16, cs)
    else:
        vol = _pack(np.full_like(C, 16), C, cs)
    assert (sgm.cost16(vol, cs, CAP) == C).all()
    return vol


def saturating(W, H, D, cs):
    """plane 0 is free everywhere (n = 1, s = 0); every other plane is unseen in half of the pixels and seen at a mean cost at or past
    the cap in the rest: m = 0 along every path, and L of the planes >= 2 climbs to cap + P2"""
    d, y, x = np.mgrid[0:D, 0:H, 0:W]
    unseen = (d + y + x) % 2 == 0
    n = np.where(unseen, 0, 1 + (d + 2 * y + x) % 3)
    full = 255 * 255 if cs == 24 else 255           # the sum of one view at a mean of 255 grey levels: C = 4080 exactly
    s = np.where((d + x) % 4 == 1, np.minimum((1 << cs) - 1, 2 * full * n), full * n)
    s = np.where(unseen, 0, s)
    n[0], s[0] = 1, 0
    return _pack(n, s, cs)


DIVISION_TARGETS = (0, 1, 2, CAP - 1, CAP, CAP + 1)    # around 0, 1, cap - 1, cap and cap + 1 for cost_cap 4080 and for cost_cap 1


def division_cells(cs):
    """(n, s) of every crafted cell: for every count and every target k the smallest s with floor(16 s / den) >= k, and that s minus
    one (the other side of the floor boundary); then the largest legal sum of the count"""
    field = (1 << cs) - 1
    ns, ss = [], []
    for n in range(1, 256 if cs == 24 else 257):
        den = 255 * n if cs == 24 else n
        for k in DIVISION_TARGETS:
            s = -((-k * den) // 16)
            for v in (s, s - 1):
                ns.append(n)
                ss.append(min(max(v, 0), field))
        ns.append(n)
        ss.append(255 * 255 * n if cs == 24 else field)
    return np.array(ns, np.int64), np.array(ss, np.int64)


def division_edges(D, H, W, cs):
    """cells on both sides of the floor boundaries of rule 1's division, every count the count field of a real sweep can hold (1..255
    fixed; up to 256 exact), laid through the volume in a fixed shuffled order and repeated to fill it"""
    n, s = division_cells(cs)
    assert len(n) <= D * H * W, "the volume is too small for the %d crafted cells" % len(n)
    order = _rng(0xD1).permutation(len(n))
    idx = order[np.arange(D * H * W) % len(n)]
    return _pack(n[idx], s[idx], cs).reshape(D, H, W)


# ---- the cases of the GPU file --------------------------------------------------------------------------------------------------
# name; generator; W, H, D; sampler; args: the generator's own parameter per volume (seeds of noise, offsets of ramp, (None,)
# otherwise); params: the (paths, P1, P2, cost_cap) sets every volume of the case runs with
Case = collections.namedtuple("Case", "name gen W H D sampler args params")

# W, H, D -> the ramp offsets that bring d* across every plane edge of the kernels along a horizontal and along a vertical or diagonal
# path (test_aggregate_cpu.py asserts it)
SHAPES = (
    (2, 2, 2, (0,)),          # the smallest legal context; every diagonal path restarts every row
    (63, 5, 8, (0,)),         # one partial LDS block, odd W, one wave with all 8 planes real
    (64, 4, 9, (0,)),         # one exact block; second wave with a single real plane
    (65, 7, 64, (0,)),        # a block of one pixel; all 64 lanes own a plane; 8 waves
    (129, 6, 65, (0,)),       # second column workgroup holds one path; second lane slot holds one plane; 9 waves
    (128, 3, 128, (0,)),      # exact column groups, 16 waves of 8 planes, two full lane slots
    (131, 5, 129, (0, 100)),  # four planes per lane and 16 planes per wave begin here; last wave has one real plane
    (67, 9, 193, (0, 60, 120, 170)),   # the slot edge 191|192, last slot with one plane
    (33, 70, 17, (0,)),       # H > 2 W: diagonal paths wrap twice
    (130, 4, 256, (0, 120, 240)),      # the largest D
)
# seeds of the noise volumes that are too small to meet the premises of a noise case (a tie of the selection above all) with any seed
SMALL_SEEDS = {(2, 2, 2): 7871, (63, 5, 8): 3, (64, 4, 9): 1}
FOUR_PATHS_TOO = ((63, 5, 8), (131, 5, 129))
EXACT_TOO = ((129, 6, 65), (33, 70, 17))
# 8 (4080 + 4111) = 65528, 4 (4080 + 12303) = 65532, and the same ceiling with P1 = P2
CEILING = ((8, 16, 4111, CAP), (4, 16, 12303, CAP), (8, 4111, 4111, CAP))


def _cases():
    out = []
    for W, H, D, offs in SHAPES:
        params = (STD, (4,) + STD[1:]) if (W, H, D) in FOUR_PATHS_TOO else (STD,)
        shape = "%dx%dx%d" % (W, H, D)
        out.append(Case("noise-" + shape, "noise", W, H, D, "fixed", (SMALL_SEEDS.get((W, H, D), 0x5EED + D),), params))
        out.append(Case("ramp-" + shape, "ramp", W, H, D, "fixed", offs, params))
        if (W, H, D) in EXACT_TOO:
            out.append(Case("noise-exact-" + shape, "noise", W, H, D, "exact", (0xE5AC + D,), (STD,)))
    # L gains at most cost_cap per step, so cap + P2 with P2 = 12303 needs four steps from the start of a path: the vertical paths of
    # both directions reach it in one cell only from H = 9 on.  With P2 = 4111 two steps do, and H = 6 is enough.
    out.append(Case("saturating-33x12x9", "saturating", 33, 12, 9, "fixed", (None,), CEILING))
    out.append(Case("saturating-129x6x130", "saturating", 129, 6, 130, "fixed", (None,), (CEILING[0], CEILING[2])))
    out.append(Case("saturating-129x9x130", "saturating", 129, 9, 130, "fixed", (None,), CEILING))
    for sampler in ("fixed", "exact"):
        out.append(Case("division-%s-65x6x9" % sampler, "division_edges", 65, 6, 9, sampler, (None,), ((8, 0, 0, CAP), (8, 0, 0, 1), (4, 0, 0, CAP))))
    # penalty edges: no small penalty, both penalties equal, the smallest cap
    out.append(Case("noise-penalties-64x4x9", "noise", 64, 4, 9, "fixed", (4,), ((8, 0, 128, CAP), (8, 128, 128, CAP), (8, 1, 1, 1))))
    return tuple(out)


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _volumes(name):
    case = next(c for c in CASES if c.name == name)
    cs = CS[case.sampler]
    out = []
    for arg in case.args:
        if case.gen == "noise":
            vol = noise(case.W, case.H, case.D, cs, arg)
        elif case.gen == "ramp":
            vol = ramp(case.W, case.H, case.D, cs, arg)
        elif case.gen == "saturating":
            vol = saturating(case.W, case.H, case.D, cs)
        else:
            vol = division_edges(case.D, case.H, case.W, cs)
        assert vol.shape == (case.D, case.H, case.W) and vol.dtype == np.uint32
        vol.setflags(write=False)
        out.append(("%s/%s" % (case.name, arg), vol))
    return tuple(out)


def volumes(case):
    """((key, volume), ...) of a case: one volume per entry of case.args, built once and read-only"""
    return _volumes(case.name)
