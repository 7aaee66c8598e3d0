"""numpy restatement of the point filter (oracle/filter_oracle.c: orc_filter_points) for small clouds, with the intermediate
results the kept set hides -- density, iteration count, neighbour pairs, the greedy pass's longest dependency chain -- and
with the library's grid arithmetic (csrc/filter.hip: dehomog_cells, cell_hash, for_lower_neighbours, chunk_sums) restated
next to it, so that a test can ask which cell and bucket a point gets and what a given fault of the grid would change.

Arithmetic: float32 where the oracle computes in float, float64 where it computes in double, in the oracle's operation
order.  `defect=` injects one of DEFECTS; every crafted cloud of tests/filter_clouds.py names the defects it is there for.
Meant for clouds of up to about 300 points (Python loops over points, numpy over their lists)."""
import math
from collections import namedtuple

import numpy as np

f32 = np.float32
f64 = np.float64

DEFECTS = ("trunc", "skip_cell", "bucket_any", "desc_lists", "iter_plus", "iter_minus", "no_clamp", "ties_desc", "nan_last")
GRID_DEFECTS = ("trunc", "skip_cell", "bucket_any")   # these need the grid walk (grid="fixed" or "committed")

Result = namedtuple("Result", "keep density iterations pairs chain normalizers mixed_nan")


def dehomog(points4):
    p = np.ascontiguousarray(points4, f32)
    with np.errstate(all="ignore"):
        return (p[:, :3] / p[:, 3:4]).astype(f32)


def radius_of(alpha):
    return f32(alpha) / f32(4.0)


# ---- the library's grid ---------------------------------------------------------------------------------------------
CELL_PAD = 1.0 + 2.0 ** -18


def cell_side(radius, arith="fixed"):
    """side of a grid cell: f32 sqrt as committed before the fix; with it, f64 sqrt of radius + 2^-150 (the rounding of a subnormal
    square), padded by 2^-18"""
    if arith == "committed":
        return f32(np.sqrt(f32(radius)))
    return math.sqrt(float(f32(radius)) + 2.0 ** -150) * CELL_PAD


def cells(p3, radius, arith="fixed", trunc=False):
    """(N, 3) int64 cell indices of dehomogenised float32 coordinates"""
    p3 = np.asarray(p3, f32)
    with np.errstate(all="ignore"):
        if arith == "committed":
            inv = f32(1.0) / cell_side(radius, "committed")
            q = (p3 * inv).astype(f32)
        else:
            inv = 1.0 / cell_side(radius, "fixed")
            q = p3.astype(f64) * inv
        f = np.trunc(q) if trunc else np.floor(q)
        f = np.fmin(np.fmax(f, -1.0e9), 1.0e9)      # fmax / fmin: a NaN gives the other operand
    return f.astype(np.int64)


def table_size(N):
    t = 1
    while t < 2 * N:
        t <<= 1
    return t


def cell_hash(c, mask):
    m = 0xffffffff
    return (((int(c[0]) & m) * 73856093 & m) ^ ((int(c[1]) & m) * 19349663 & m) ^ ((int(c[2]) & m) * 83492791 & m)) & mask


NEIGHBOUR_CELLS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]   # the walk's order; index 13 is the centre


def _d2(p3, i, js):
    with np.errstate(all="ignore"):
        d = p3[i] - p3[js]                                  # float32
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _weights(d2, radius):
    with np.errstate(all="ignore"):
        return (1.0 - (d2 / f32(radius)).astype(f64)).astype(f32)   # densityFn, (float)(1. - d2 / radius): the division is in float


def lower_lists(p3, radius, grid="oracle", defect=None):
    """per point i the (indices j < i, weights) of its accepted pairs: brute force (grid="oracle") or the library's walk over
    27 cells of the hash grid with the arithmetic named by `grid`"""
    N = len(p3)
    kind, _, arg = (defect or "").partition(":")
    out = []
    if grid == "oracle":
        for i in range(N):
            js = np.arange(i)
            d2 = _d2(p3, i, js)
            ok = d2 <= radius
            out.append((js[ok], _weights(d2[ok], radius)))
        return out
    c = cells(p3, radius, grid, trunc=(kind == "trunc"))
    mask = table_size(N) - 1
    h = np.array([cell_hash(c[i], mask) for i in range(N)])
    skip = int(arg) if kind == "skip_cell" else -1
    for i in range(N):
        found = []
        for k, (dx, dy, dz) in enumerate(NEIGHBOUR_CELLS):
            if k == skip:
                continue
            n = c[i] + (dx, dy, dz)
            bucket = np.nonzero(h == cell_hash(n, mask))[0]
            bucket = bucket[bucket < i]
            if kind != "bucket_any":
                bucket = bucket[np.all(c[bucket] == n, axis=1)]
            found.extend(bucket.tolist())
        js = np.array(sorted(found), np.int64)               # both orderings of the library end ascending by index
        d2 = _d2(p3, i, js) if len(js) else np.zeros(0, f32)
        ok = d2 <= radius
        out.append((js[ok], _weights(d2[ok], radius)))
    return out


# ---- the two global sums --------------------------------------------------------------------------------------------
def chunk_sum(v):
    """chunk_sums + finish_*: 256 chunks of ceil(N / 256) elements, each by 256 thread-strided partial sums folded pairwise
    (strides 128 .. 1), the chunk sums then added in order"""
    v = np.asarray(v, f64)
    N = len(v)
    per = (N + 255) // 256
    start = np.arange(256)[:, None] * per
    end = np.minimum(start + per, N)
    part = np.zeros((256, 256), f64)                          # [chunk, thread]
    with np.errstate(all="ignore"):
        for r in range((per + 255) // 256):                   # thread t adds elements t, t + 256, ... of its chunk in that order
            idx = start + r * 256 + np.arange(256)[None, :]
            live = idx < end
            part = np.where(live, part + v[np.where(live, idx, 0)], part)
        stride = 128
        while stride:
            part[:, :stride] = part[:, :stride] + part[:, stride:2 * stride]
            stride >>= 1
        return _seq_sum(part[:, 0], f64(0.0))


def _seq_sum(v, start):
    """start + v[0] + v[1] + ... in the dtype of start, one rounding per addition"""
    if len(v) == 0:
        return start
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate([[start], v]).astype(type(start)), dtype=type(start))[-1]


# ---- the filter -------------------------------------------------------------------------------------------------------
def filter_points(points4, alpha, defect=None, grid="oracle", sums="sequential"):
    kind = (defect or "").partition(":")[0]
    assert defect is None or kind in DEFECTS, defect
    assert not (kind in GRID_DEFECTS and grid == "oracle"), "grid defects need the grid walk"
    p3 = dehomog(points4)
    N = len(p3)
    radius = radius_of(alpha)
    lo = lower_lists(p3, radius, grid, defect)
    if kind == "desc_lists":
        lo = [(j[::-1], w[::-1]) for j, w in lo]
    ups = [[] for _ in range(N)]
    for i in range(N):                                        # ascending i: every upper list ascends by index
        for j, w in zip(*lo[i]):
            ups[j].append((i, w))
    if kind == "desc_lists":
        ups = [u[::-1] for u in ups]
    up = [(np.array([i for i, _ in u], np.int64), np.array([w for _, w in u], f32)) for u in ups]
    pairs = sum(len(j) for j, _ in lo)

    density = np.ones(N, f32)
    score = np.zeros(N, f32)
    states = [(density, score)]
    normalizers = []
    it = 0

    def iterate(density):
        score = np.zeros(N, f32)
        terms = []                                            # per point: the f64 terms of `sum`, in the oracle's order
        with np.errstate(all="ignore"):
            for i in range(N):
                j, w = lo[i]
                s = _seq_sum(density[j] * w, f32(0.0))        # densityTemp
                s = f32(0.0) + s                              # score[i] += densityTemp, before any higher index scatters
                u, wu = up[i]
                score[i] = _seq_sum(density[u] * wu, s)
                terms.append(((density[i] + density[j]) * w).astype(f64))
            if sums == "sequential":
                total = _seq_sum(np.concatenate(terms) if terms else np.zeros(0), f64(0.0))
            else:
                total = chunk_sum([_seq_sum(t, f64(0.0)) for t in terms])
            normalizer = f32(f64(N) / total)
            nd = score * normalizer
            if kind != "no_clamp":
                nd = np.where(nd > f32(2.0), f32(2.0), nd).astype(f32)
            df = density - nd
            sq = (df * df).astype(f64)
            change = (_seq_sum(sq, f64(0.0)) if sums == "sequential" else chunk_sum(sq)) / N
        return nd, score, normalizer, change

    while True:
        density, score, normalizer, change = iterate(density)
        normalizers.append(normalizer)
        states.append((density, score))
        it += 1
        if not (change > 1e-6 and it < 200):
            break
    if kind == "iter_plus":
        density, score, _, _ = iterate(density)
    elif kind == "iter_minus":
        density, score = states[it - 1]

    nan = np.isnan(density)
    mixed_nan = bool(nan.any() and not nan.all())
    with np.errstate(all="ignore"):
        neg = np.where(nan, f32(0), -density)
    idx = np.arange(N)
    first = nan if kind == "nan_last" else ~nan               # False sorts first: NaN leads (greedy_keys) unless nan_last
    order = np.lexsort((-idx if kind == "ties_desc" else idx, neg, first))
    rank = np.empty(N, np.int64)
    rank[order] = idx
    score = score.copy()
    keep = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for o in order:
            if score[o] < f32(0.7):
                continue
            local = f64(density[o])
            j, w = lo[o]
            for jj, ww in zip(j, w):                          # one at a time: an index may repeat under bucket_any
                score[jj] = f32(f64(score[jj]) - local * f64(ww))
            keep[o] = True
    level = np.zeros(N, np.int64)                             # the round a point is decided in: one past its latest earlier-ranked upper neighbour
    for o in order:
        u = up[o][0]
        u = u[rank[u] < rank[o]]
        level[o] = 1 + (level[u].max() if len(u) else 0)
    return Result(np.nonzero(keep)[0].astype(np.int32), density, it, pairs, int(level.max()) if N else 0, normalizers, mixed_nan)
