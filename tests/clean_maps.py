"""Crafted index maps and volumes for mvs_sweep_clean, numpy only, shared by tests/test_clean_cpu.py (which shows
with the mirror alone that every map holds what it is for) and tests/test_clean_gpu.py (which hands them to the kernels).

Index maps are int32 [H, W] with -1 for a pixel without an index, made for D = 8 planes.  volume_for() turns an index map into a legal
packed volume whose winner-take-all selection is that map; rules_case() builds the cells (and sums S) rules 1 and 2 are read from."""
import functools

import numpy as np

D_MAPS = 8
PER = {24: 255 * 255, 16: 255}     # the largest sum one view adds to a cell


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pack(n, s, cs):
    n, s = np.asarray(n, np.int64), np.asarray(s, np.int64)
    assert (s >= 0).all() and (s < (1 << cs)).all() and (n >= 0).all() and (n < (1 << (32 - cs))).all()
    assert (s <= PER[cs] * n).all(), "a sum no sweep can produce"
    return ((n << cs) | s).astype(np.uint32)


# ---- index maps -----------------------------------------------------------------------------------------------------------------
def constant(W, H, plane=3):
    return np.full((H, W), plane, np.int32)


def checkerboard(W, H, max_diff):
    """indices 0 and max_diff + 1 alternate: no two neighbours are connected with max_diff, all are with max_diff + 1"""
    y, x = np.mgrid[0:H, 0:W]
    return (((x + y) % 2) * (max_diff + 1)).astype(np.int32)


def _along(path, W, H):
    """index map of a path (list of (y, x)): the plane moves by at most one per step (a triangle wave over 0..7, three pixels a plane)"""
    m = np.full((H, W), -1, np.int32)
    pos = np.arange(len(path)) // 3 % 14
    planes = np.where(pos < 8, pos, 14 - pos)
    ys, xs = np.array(path).T
    m[ys, xs] = planes
    return m


def serpentine(W, H):
    """the even rows, joined alternately at their right and left ends through the odd rows, which are walls otherwise -> (map, length)"""
    path = []
    for k, y in enumerate(range(0, H, 2)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, W - 1 if k % 2 == 0 else 0))
    return _along(path, W, H), len(path)


def spiral(W, H):
    """a one-pixel-wide path from the corner inwards with one-pixel walls between its turns -> (map, length)"""
    on = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    path = [(0, 0)]
    on[0, 0] = True

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and not on[yy, xx]

    def can(dy, dx):
        # the next cell is free, the one behind it is not path (it would touch an earlier turn), nor are the next cell's side neighbours
        ny, nx = y + dy, x + dx
        if not free(ny, nx):
            return False
        for ay, ax in ((ny + dy, nx + dx), (ny + dx, nx + dy), (ny - dx, nx - dy)):
            if 0 <= ay < H and 0 <= ax < W and on[ay, ax]:
                return False
        return True

    while True:
        if not can(dy, dx):
            dy, dx = dx, -dy      # turn right (y grows downwards)
            if not can(dy, dx):
                break
        y, x = y + dy, x + dx
        on[y, x] = True
        path.append((y, x))
    return _along(path, W, H), len(path)


def ramp(W, H):
    """index = x // 26: neighbouring stripes differ by one plane, the ends of a row by many"""
    return np.broadcast_to((np.arange(W) // 26).astype(np.int32), (H, W)).copy()


SQUARE_CORNERS = {8: ((8, 8), (24, 8), (40, 8)), 16: ((16, 16), (48, 16), (80, 16)), 32: ((32, 32), (96, 32), (160, 32)),
                  64: ((64, 64), (128, 64), (192, 64))}     # (x, y): corners where four tiles of that size (and no larger one) meet


def threshold_squares(W, H, min_size=16, plane=5):
    """components of min_size - 1, min_size and min_size + 1 pixels (min_size = 16: a 4 x 4 square, one corner less, one pixel more)
    centred on tile corners, so each has pixels in four tiles -> (map, {(x, y): size})"""
    assert min_size == 16
    m = np.full((H, W), -1, np.int32)
    sizes = {}
    for corners in SQUARE_CORNERS.values():
        for (cx, cy), size in zip(corners, (15, 16, 17)):
            m[cy - 2:cy + 2, cx - 2:cx + 2] = plane
            if size == 15:
                m[cy - 2, cx - 2] = -1
            if size == 17:
                m[cy, cx + 2] = plane
            sizes[(cx, cy)] = size
    return m, sizes


def percolation(W, H, seed, planes=(4,), weights=None, p=0.60):
    """site percolation just above the square lattice's threshold (0.593): a pixel has an index with probability p, drawn from `planes`
    (with `weights`, else evenly)"""
    rng = _rng(seed)
    valid = rng.random((H, W)) < p
    return np.where(valid, rng.choice(np.array(planes), (H, W), p=weights), -1).astype(np.int32)


# name, seed, planes, weights.  With max_diff 1, index 0 joins neither 2 nor 3: it is rare, so that the pixels with 2 or 3 (0.594 of all)
# stay above the threshold and one component still spans the image (tests/test_clean_cpu.py asserts it for these seeds).
PERCOLATION_SHAPE = (257, 131)
PERCOLATION = (("one index", 0x9E2C, (4,), None), ("three indices", 0x9E2D, (0, 2, 3), (0.01, 0.495, 0.495)))


# ---- volumes --------------------------------------------------------------------------------------------------------------------
def volume_for(index, D, cs, seed=0xC1EA):
    """a legal packed volume [D, H, W] whose winner-take-all selection is `index`: count 1 and sum 0 at the wanted plane, counts 1..3
    with a sum of 1 .. PER n elsewhere, count 0 on every plane of a pixel without an index"""
    H, W = index.shape
    assert index.max() < D
    rng = _rng(seed)
    n = rng.integers(1, 4, (D, H, W))
    s = 1 + (rng.integers(0, PER[cs], (D, H, W)) * n) % (PER[cs] * n)
    wanted = np.arange(D)[:, None, None] == index[None]
    n[wanted], s[wanted] = 1, 0
    none = np.broadcast_to(index[None] < 0, n.shape)
    n[none], s[none] = 0, 0
    return _pack(n, s, cs)


UNIQUENESS = 10      # the crafted cells of rules_case() sit on the two sides of rule 2's inequality for this u
KINDS = ("alone", "rival one plane away", "distance 2, equal products", "distance 2, one unit below", "far, one unit below",
         "largest sums, below", "largest sums, not below", "rules 1 and 2")


@functools.lru_cache(maxsize=None)
def rules_case(W, H, D, cs, seed):
    """-> (index, vol, S, kind): the selection the maps are to hold, the cells rules 1-2 read, the sums rule 2 reads with
    MVS_CLEAN_SCORES_AGGREGATED, and per pixel the number of its entry in KINDS (-1: the lower rows, i.i.d. cells).
    A crafted pixel has its winner at plane i with count n_i in 0..3 (255 or 257 for the largest sums) and one other seen plane d on a
    random side of i.  With u = 10, s_i = 9 k n_i and s_d = 10 k n_d give equal products s_d n_i 90 = s_i n_d 100 (no rival);
    s_d one smaller is a rival by the smallest step s_d can make.  Likewise S_i = 9 k against S_d = 10 k or 10 k - 1, and 65535 against
    58981 (65535 * 90 = 5898150 >= 5898100) or 58982 (< 5898200).  The unseen cells of kind "alone" hold S = 0: only their count keeps
    them from being rivals."""
    rng = _rng(seed)
    per = PER[cs]
    index = rng.integers(0, D, (H, W)).astype(np.int32)
    index[rng.random((H, W)) < 0.1] = -1
    n = np.zeros((D, H, W), np.int64)
    s = np.zeros((D, H, W), np.int64)
    S = np.full((D, H, W), 65535, np.int64)
    kind = np.full((H, W), -1, np.int64)
    top = max(H // 2, 1)
    for p in range(top * W):
        y, x = divmod(p, W)
        i = int(index[y, x])
        if i < 0:
            continue
        k = p % len(KINDS)
        kind[y, x] = k
        ni = (p // len(KINDS)) % 4
        kk = int(rng.integers(1, per // 20))
        dist = {1: 1, 2: 2, 3: 2}.get(k, int(rng.integers(3, D)))
        side = 1 if rng.random() < 0.5 else -1
        d = i + side * dist
        if not 0 <= d < D:
            d = i - side * dist
        if not 0 <= d < D:       # far rivals: any plane at least 3 away
            d = int(rng.choice([c for c in range(D) if abs(c - i) >= 3]))
        nd = int(rng.integers(1, 4))
        if k in (5, 6):
            ni = nd = 255 if cs == 24 else 257     # the largest count of the fixed sampler's field; 255 * 257 = 65535 fills the exact one's sum
            big = per * nd
            n[i, y, x], n[d, y, x], s[d, y, x] = ni, nd, big
            # s_d n_i 90 < s_i n_d 100 from s_i = floor(0.9 s_d) + 1 on (n_i = n_d)
            s[i, y, x] = (big * 90) // 100 + (1 if k == 5 else 0)
            S[i, y, x], S[d, y, x] = (58982 if k == 5 else 58981), 65535
            continue
        if k == 7:
            ni = 1      # fails min_views 2, and has a rival
        n[i, y, x], s[i, y, x] = ni, 9 * kk * ni
        S[i, y, x] = 9 * min(kk, 6000)
        if k == 0:
            S[:, y, x] = np.where(np.arange(D) == i, S[i, y, x], 0)
            continue
        below = k in (3, 4, 7)
        n[d, y, x] = nd
        s[d, y, x] = 0 if k == 1 else 10 * kk * nd - (1 if below else 0)
        S[d, y, x] = 0 if k == 1 else 10 * min(kk, 6000) - (1 if below else 0)
    # the rows below: i.i.d. cells and sums, about a tenth of the cells unseen
    rows = slice(top, H)
    shape = n[:, rows].shape
    nn = rng.integers(0, 4, shape)
    nn[rng.random(shape) < 0.1] = 0
    n[:, rows] = nn
    s[:, rows] = (rng.integers(0, per + 1, shape) * nn) // rng.integers(1, 8, shape)
    S[:, rows] = rng.integers(0, 65536, shape)
    vol = _pack(n, s, cs)
    for a in (index, vol, kind):
        a.setflags(write=False)
    S = S.astype(np.uint16)
    S.setflags(write=False)
    return index, vol, S, kind
