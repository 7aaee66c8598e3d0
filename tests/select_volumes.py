"""Crafted packed cost volumes for the depth selection and the sub-plane refinement (csrc/select.hip: argmin_volume, combine_best,
refine_depth), numpy only, and the table of cases that tests/test_select_edges_gpu.py hands to the kernels.  tests/test_select_cpu.py
checks with the mirror alone (tests/select_mirror.py) that every generator reaches what it is here for.

Every generator takes (W, H, D, cs, seed) and returns uint32 [D, H, W] (foreign_index: the volume and an int32 index map) within what a
sweep can write: cs = 24 (fixed sampler, count << 24 | sum) with n <= 255 and s <= 255 * 255 * n, or cs = 16 (exact sampler,
count << 16 | sum) with n <= 257 and s <= 255 * n.  Pixels are numbered p = y * W + x and a pixel's class is p modulo the number of
classes, so every class lands in every workgroup and on every lane position of a 16-byte load.

What the layouts cannot reach, by arithmetic and not by choice:
  * cs = 16: two legal cells that differ by 1 / (n1 n2) have different f32 quotients.  Equal quotients need 1 / (n1 n2) below one
    ulp of the quotient; the means are below 256 (ulp 2^-16 from 128 on, less below), so n1 n2 > 2^16, which leaves the counts 256 and
    257 only, and none of their 255 * 256 pairs of sums has it (searched exhaustively by test_select_cpu.py).  `near_equal` and the
    f32-flat parabolas therefore keep their f32 premise for cs = 24 only; for cs = 16 they are still pairs one step of the rational
    order apart.
  * a selection that IS the volume's argmin has ca > cb (a tie goes to the lower plane) and cc >= cb around its plane, so the exact
    den = (ca - cb) + (cc - cb) is positive and the exact vertex lies in (-1/2, +1/2]: `parabolas`, which the tests refine after
    mvs_sweep_argmin, holds flat-in-f32 (den 0 in f32, positive exactly), vertex 0, vertex +1/2 and a vertex just inside -1/2.  The
    exactly flat parabola, den < 0, den 0 in f32 with a negative exact den, the vertex far outside and the vertex at exactly -1/2 need an
    index that is not the argmin: they are classes of `foreign_index`.  (ca - 2 cb is exact in f32 for cb <= ca <= 4 cb and rounding
    keeps signs, so an argmin's den cannot turn negative in f32 either.)"""
import collections
import functools
import math
import zlib

import numpy as np

CS = {"fixed": 24, "exact": 16}
PER = {24: 255 * 255, 16: 255}      # the largest sum of one view
NMAX = {24: 255, 16: 257}           # the largest count
NEAR_MIN_COUNT = {24: 64, 16: 128}  # counts of the near-equal pairs: 1 / (n1 n2) <= 2^-12, far below the ulp 2^-8 of means >= 2^15 (cs 24)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pack(n, s, cs):
    n, s = np.asarray(n, np.int64), np.asarray(s, np.int64)
    assert (n >= 0).all() and (n <= NMAX[cs]).all() and (s >= 0).all() and (s <= PER[cs] * n).all() and (s < (1 << cs)).all()
    return ((n << cs) | s).astype(np.uint32)


def max_cell(cs):
    """(count, sum) of the largest legal cell: 255 * (255 * 255 * 255) = 2^32 - 66716671 is the largest product the comparison forms"""
    return NMAX[cs], PER[cs] * NMAX[cs]


def straddle_cells(cs):
    """cells A (cheaper) and B with the cross products of their comparison on either side of 2^31 (cs 24): A's sum times B's count is
    2146794000 < 2^31 <= 2147483775 = B's sum times A's count -- compared as signed numbers they order the other way round"""
    if cs == 24:
        return (255, 255 * 64760), (130, 8421505)
    return (257, 257 * 200), (129, 129 * 200 + 1)


def near_pair(rng, cs):
    """(n1, s1), (n2, s2) with s1 / n1 - s2 / n2 = 1 / (n1 n2) exactly, means in the upper half of the range"""
    while True:
        n1, n2 = (int(v) for v in rng.integers(NEAR_MIN_COUNT[cs], NMAX[cs] + 1, 2))
        if n1 != n2 and math.gcd(n1, n2) == 1:
            break
    k = int(rng.integers(PER[cs] // 2, PER[cs] - 1))
    s1 = pow(n2, -1, n1) + k * n1            # s1 n2 = 1 (mod n1)
    s2 = (s1 * n2 - 1) // n1
    assert s1 * n2 - s2 * n1 == 1
    return (n1, s1), (n2, s2)


def _cell(rng, cs, mean, n=None):
    """a cell whose mean is `mean` to within 1 / (2 n)"""
    n = int(rng.integers(1, NMAX[cs] + 1)) if n is None else n
    return n, int(min(max(round(mean * n), 0), PER[cs] * n))


def _above(rng, cs, n_ref, s_ref):
    """a cell with a mean strictly above s_ref / n_ref (which is at most PER - 1)"""
    n = int(rng.integers(1, NMAX[cs] + 1))
    least = (s_ref * n) // n_ref + 1
    return n, int(rng.integers(least, PER[cs] * n + 1))


def _top(rng, cs):
    """a cell with a mean above PER - 1: worse than every near-equal pair"""
    n = int(rng.integers(1, NMAX[cs] + 1))
    return n, PER[cs] * n - int(rng.integers(0, n))


def _random_cells(rng, D, H, W, cs, unseen=0.15):
    n = rng.integers(1, NMAX[cs] + 1, (D, H, W))
    s = rng.integers(0, PER[cs] * n + 1)
    n[rng.random((D, H, W)) < unseen] = 0
    s[n == 0] = 0
    return n, s


def _pixels(W, H):
    for p in range(W * H):
        yield p, p // W, p % W


def _put_near_pair(rng, n, s, y, x, cs, D):
    """a near-equal pair as the two best cells of the pixel at two random planes, the cheaper one at the lower or at the higher plane;
    every other plane is worse or unseen"""
    hi, lo = near_pair(rng, cs)
    da, db = sorted(int(v) for v in rng.choice(D, 2, replace=False))
    first, second = (hi, lo) if rng.random() < 0.5 else (lo, hi)
    for d in range(D):
        n[d, y, x], s[d, y, x] = (0, 0) if rng.random() < 0.2 else _top(rng, cs)
    n[da, y, x], s[da, y, x] = first
    n[db, y, x], s[db, y, x] = second


def mixed_counts(W, H, D, cs, seed):
    """random cells with counts all over 1..NMAX: the smallest sum is rarely the smallest mean.  From D = 3 on every pixel has an unseen
    cell and two different counts; every fourth pixel has a near-equal pair as its two best cells."""
    rng = _rng(seed)
    n, s = _random_cells(rng, D, H, W, cs, unseen=0.0)
    for p, y, x in _pixels(W, H):
        if D >= 2 and p % 4 == 0:
            _put_near_pair(rng, n, s, y, x, cs, D)
        if D >= 3:
            if (n[:, y, x] != 0).all():   # the most expensive cell goes
                d = int(np.argmax(s[:, y, x] / n[:, y, x]))
                n[d, y, x] = s[d, y, x] = 0
            while len(set(int(v) for v in n[:, y, x] if v)) < 2:
                d = int(rng.integers(D))
                if n[d, y, x]:
                    n[d, y, x] = int(rng.integers(1, NMAX[cs] + 1))
                    s[d, y, x] = min(int(s[d, y, x]), PER[cs] * int(n[d, y, x]))
    return _pack(n, s, cs)


def near_equal(W, H, D, cs, seed):
    """every pixel: a near-equal pair as the two best cells (D >= 2)"""
    rng = _rng(seed)
    n, s = _random_cells(rng, D, H, W, cs)
    if D >= 2:
        for p, y, x in _pixels(W, H):
            _put_near_pair(rng, n, s, y, x, cs, D)
    return _pack(n, s, cs)


def ties(W, H, D, cs, seed):
    """exact ties of the best mean at 2..D planes: p % 4 = 0 the pair (b - 1, b) with b running over every plane boundary 1..D - 1,
    1 all planes, 2 a random set of 2..D planes, 3 the pair of 0 and a random plane above it.  Even p // 4: the tied cells are
    equal; odd: equal rationals with different counts.  Every fifth tie is at cost 0."""
    rng = _rng(seed)
    n, s = _random_cells(rng, D, H, W, cs)
    if D < 2:
        return _pack(n, s, cs)
    for p, y, x in _pixels(W, H):
        q = p // 4
        b = int(rng.integers(1, 9))
        a = 0 if q % 5 == 0 else int(rng.integers(0, (PER[cs] - 1) * b + 1))
        if p % 4 == 0:
            planes = [q % (D - 1), q % (D - 1) + 1]
        elif p % 4 == 1:
            planes = list(range(D))
        elif p % 4 == 2:
            planes = sorted(int(v) for v in rng.choice(D, 2 + q % (D - 1), replace=False))
        else:
            planes = [0, int(rng.integers(1, D))] + ([int(rng.integers(1, D))] if D > 2 else [])
        m_same = int(rng.integers(1, NMAX[cs] // b + 1))
        for d in range(D):
            if d in planes:
                m = m_same if q % 2 == 0 else int(rng.integers(1, NMAX[cs] // b + 1))
                n[d, y, x], s[d, y, x] = b * m, a * m
            else:
                n[d, y, x], s[d, y, x] = (0, 0) if rng.random() < 0.25 else _above(rng, cs, b, a)
        if q % 2 == 1 and len(set(int(n[d, y, x]) for d in planes)) == 1:   # different counts were asked for
            n[planes[-1], y, x], s[planes[-1], y, x] = (b, a) if n[planes[-1], y, x] != b else (2 * b, 2 * a)
    return _pack(n, s, cs)


EXTREME_CLASSES = ("all planes the largest cell", "A then B across 2^31", "B then A across 2^31", "best at D - 1 by one unit of the sum",
                   "best at 0 by one unit of the sum", "only the last plane seen", "nobody sees", "only one plane of the tail seen")


def tail_plane(D, k):
    """a plane of the tail behind the last full group of 8 (the last plane where there is no tail)"""
    return 8 * (D // 8) + k % (D % 8) if D % 8 else D - 1


def extremes(W, H, D, cs, seed):
    """p % 8 picks the class of EXTREME_CLASSES"""
    rng = _rng(seed)
    nm, sm = max_cell(cs)
    A, B = straddle_cells(cs)
    n, s = np.zeros((D, H, W), np.int64), np.zeros((D, H, W), np.int64)
    for p, y, x in _pixels(W, H):
        k = p % 8
        if k in (0, 1, 2, 3, 4):
            n[:, y, x], s[:, y, x] = nm, sm
        if k in (1, 2) and D >= 2:
            n[0, y, x], s[0, y, x] = A if k == 1 else B
            n[1, y, x], s[1, y, x] = B if k == 1 else A
            n[2::2, y, x] = s[2::2, y, x] = 0
        elif k == 3:
            s[D - 1, y, x] = sm - 1
        elif k == 4:
            s[0, y, x] = sm - 1
        elif k == 5:
            n[D - 1, y, x], s[D - 1, y, x] = _cell(rng, cs, rng.random() * PER[cs])
        elif k == 7:
            d = tail_plane(D, p // 8)
            n[d, y, x], s[d, y, x] = _cell(rng, cs, rng.random() * PER[cs])
    return _pack(n, s, cs)


PARABOLA_CLASSES = ("generic",) * 7 + ("vertex 0", "flat in f32", "vertex +1/2", "generic, largest counts", "lower neighbour unseen",
                                      "upper neighbour unseen", "plane 0 selected", "plane D - 1 selected", "vertex just inside -1/2")


def _double(cell):
    return 2 * cell[0], 2 * cell[1]


def _generic_triple(rng, cs, n=None):
    """cells (lower, selected, upper): the selected mean in the lower 45 % of the range, each neighbour 5 % .. 50 % of the range above it:
    den >= a tenth of the range and |vertex| <= 0.41"""
    per = PER[cs]
    cb = rng.random() * 0.45 * per
    da, dc = (0.05 + 0.45 * rng.random()) * per, (0.05 + 0.45 * rng.random()) * per
    return _cell(rng, cs, cb + da, n), _cell(rng, cs, cb, n), _cell(rng, cs, cb + dc, n)


def parabolas(W, H, D, cs, seed):
    """p % 16 picks the class of PARABOLA_CLASSES around the plane 1 + (p // 16) % (D - 2), which is the pixel's argmin; D < 3: random cells"""
    rng = _rng(seed)
    n, s = _random_cells(rng, D, H, W, cs)
    if D < 3:
        return _pack(n, s, cs)
    half = NMAX[cs] // 2
    for p, y, x in _pixels(W, H):
        k, q = p % 16, p // 16
        i = 1 + q % (D - 2)
        name = PARABOLA_CLASSES[k]
        if name == "vertex just inside -1/2" and q % 2:
            name = "generic"
        lo, mid, up = _generic_triple(rng, cs, NMAX[cs] if name == "generic, largest counts" else None)
        top = False
        if name == "vertex 0":
            lo = _cell(rng, cs, lo[1] / lo[0], int(rng.integers(1, half + 1)))
            up = _double(lo)
        elif name == "flat in f32":
            lo, mid = near_pair(rng, cs)
            up = lo if q % 2 else mid
            top = True
        elif name == "vertex +1/2":
            mid = _cell(rng, cs, mid[1] / mid[0], int(rng.integers(1, half + 1)))
            up = _double(mid)
        elif name == "vertex just inside -1/2":
            lo = (mid[0], mid[1] + 1)
        elif name == "plane 0 selected":
            i = 0
        elif name == "plane D - 1 selected":
            i = D - 1
        for d in range(D):
            if rng.random() < 0.2:
                n[d, y, x], s[d, y, x] = 0, 0
            elif top:
                n[d, y, x], s[d, y, x] = _top(rng, cs)
            else:   # at least 4 % of the range above the selected mean
                f = mid[1] / mid[0] / PER[cs] + 0.04
                n[d, y, x], s[d, y, x] = _cell(rng, cs, (f + (1.0 - f) * rng.random()) * PER[cs])
        for d, cell in ((i - 1, lo), (i, mid), (i + 1, up)):
            if 0 <= d < D:
                n[d, y, x], s[d, y, x] = cell
        if name == "lower neighbour unseen":
            n[i - 1, y, x] = s[i - 1, y, x] = 0
        elif name == "upper neighbour unseen":
            n[i + 1, y, x] = s[i + 1, y, x] = 0
    return _pack(n, s, cs)


def parabola_class(p):
    return PARABOLA_CLASSES[p % 16]


def parabola_plane(p, D):
    k = PARABOLA_CLASSES[p % 16]
    return 0 if k == "plane 0 selected" else D - 1 if k == "plane D - 1 selected" else 1 + (p // 16) % (D - 2)


FOREIGN_CLASSES = ("exactly flat", "den < 0", "vertex far outside", "vertex -1/2", "den 0 in f32, negative exactly", "no index over seen cells",
                   "index 0 or D - 1", "random index")


def foreign_index(W, H, D, cs, seed):
    """a volume and an index map that is not its argmin: p % 8 picks the class of FOREIGN_CLASSES around the plane 1 + (p // 8) % (D - 2);
    D < 3: random cells and a random index"""
    rng = _rng(seed)
    n, s = _random_cells(rng, D, H, W, cs)
    index = rng.integers(-1, D, (H, W)).astype(np.int32)
    if D < 3:
        return _pack(n, s, cs), index
    per = PER[cs]
    half = NMAX[cs] // 2
    for p, y, x in _pixels(W, H):
        k, q = p % 8, p // 8
        i = 1 + q % (D - 2)
        name = FOREIGN_CLASSES[k]
        if name in ("index 0 or D - 1", "random index", "no index over seen cells"):
            index[y, x] = -1 if k == 5 else (0, D - 1)[q % 2] if k == 6 else int(rng.integers(0, D))
            if k == 5:
                n[q % D, y, x], s[q % D, y, x] = _cell(rng, cs, rng.random() * per)
            continue
        index[y, x] = i
        if name == "exactly flat":
            mid = _cell(rng, cs, rng.random() * per, int(rng.integers(1, half + 1)))
            lo, up = _double(mid), (mid if q % 2 else _double(mid))
        elif name == "den < 0":
            cb = (0.5 + 0.5 * rng.random()) * per
            lo, mid, up = _cell(rng, cs, cb * rng.random() * 0.9), _cell(rng, cs, cb), _cell(rng, cs, cb * rng.random() * 0.9)
        elif name == "vertex far outside":   # den = 0.4 of the range, vertex -1 or +1
            cells = [_cell(rng, cs, f * per) for f in (0.1, 0.3, 0.9)]
            lo, mid, up = cells if q % 2 else cells[::-1]
        elif name == "vertex -1/2":
            mid = _cell(rng, cs, rng.random() * 0.5 * per, int(rng.integers(1, half + 1)))
            lo, up = _double(mid), _cell(rng, cs, mid[1] / mid[0] + (0.05 + 0.4 * rng.random()) * per)
        else:
            mid, lo = near_pair(rng, cs)
            up = lo
        for d, cell in ((i - 1, lo), (i, mid), (i + 1, up)):
            n[d, y, x], s[d, y, x] = cell
    return _pack(n, s, cs), index


def sum_bits_in_unseen_cells(vol, cs, seed):
    """the volume with random non-zero sum bits in every cell of count 0.  No sweep writes such a cell, a caller's volume may hold one:
    the count alone says that nobody sees it, in the selection and for both neighbours of the refinement"""
    rng = _rng(seed)
    out = np.array(vol, np.uint32)
    unseen = (out >> cs) == 0
    assert unseen.any()
    out[unseen] = rng.integers(1, 1 << cs, int(unseen.sum())).astype(np.uint32)
    out.setflags(write=False)
    return out


# ---- the cases of the GPU file --------------------------------------------------------------------------------------------------
GENERATORS = {"mixed_counts": mixed_counts, "near_equal": near_equal, "ties": ties, "extremes": extremes, "parabolas": parabolas,
              "foreign_index": foreign_index}
Case = collections.namedtuple("Case", "name gen W H D sampler z_range")

# 132 x 9: P = 1188, a multiple of 4 (16-byte loads, two workgroups, the last one ragged); 131 x 9: P = 1179 (single cells, five
# workgroups, the last one ragged); D: no interior plane (1, 2), the tail loop alone (7), the unrolled loop alone (8), both (9, 17)
SHAPES = ((132, 9, 1), (131, 9, 2), (132, 9, 7), (131, 9, 7), (132, 9, 8), (131, 9, 8), (132, 9, 9), (131, 9, 9), (132, 9, 17), (131, 9, 17),
          (5, 3, 9))
D_PARTIAL = 40
PARTIAL_SHAPES = {"ties": ((132, 9), (131, 9)), "mixed_counts": ((132, 9),), "extremes": ((131, 9),)}
SPLITS = ((40,), (1, 39), (39, 1), (8, 8, 8, 8, 8), (7, 9, 24), (1,) * 40)


def z_range_of(D):
    """plane steps that are no power of two at D = 9 and D = 40"""
    return (0.25, 0.75) if D in (9, D_PARTIAL) else (-1.0, 1.0)


def _cases():
    out, partial = [], []
    for sampler in ("fixed", "exact"):
        for gen in GENERATORS:
            for W, H, D in SHAPES:
                out.append(Case("%s-%s-%dx%dx%d" % (gen, sampler, W, H, D), gen, W, H, D, sampler, z_range_of(D)))
        for gen, shapes in PARTIAL_SHAPES.items():
            for W, H in shapes:
                partial.append(Case("%s-%s-%dx%dx%d" % (gen, sampler, W, H, D_PARTIAL), gen, W, H, D_PARTIAL, sampler, z_range_of(D_PARTIAL)))
    return tuple(out), tuple(partial)


CASES, PARTIAL_CASES = _cases()


def cases_of(gen, which=None):
    return tuple(c for c in (CASES if which is None else which) if c.gen == gen)


@functools.lru_cache(maxsize=None)
def _volume(name):
    case = next(c for c in CASES + PARTIAL_CASES if c.name == name)
    out = GENERATORS[case.gen](case.W, case.H, case.D, CS[case.sampler], zlib.crc32(name.encode()))
    vol, index = out if case.gen == "foreign_index" else (out, None)
    assert vol.shape == (case.D, case.H, case.W) and vol.dtype == np.uint32
    vol.setflags(write=False)
    if index is not None:
        assert index.shape == (case.H, case.W) and index.dtype == np.int32 and index.min() >= -1 and index.max() < case.D
        index.setflags(write=False)
    return vol, index


def volume(case):
    """(volume, index map or None) of a case, built once and read-only"""
    return _volume(case.name)
