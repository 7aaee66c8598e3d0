"""numpy restatement of the semi-global aggregation contract, written from the contract and not from the kernels.

Integer arithmetic throughout (int64 work arrays, results that fit uint16 by rule 3); every path direction is one sequential scan with
all pixels of a scan line and all planes handled per step.  Volumes are [D, H, W]; `cs` is the count shift of the packed cell (24 for
the fixed sampler, 16 for the exact one)."""
import numpy as np

# rule 2: (dy, dx); `paths` = 4 or 8 takes the first 4 or 8
PATHS = ((0, +1), (0, -1), (+1, 0), (-1, 0), (+1, +1), (-1, -1), (+1, -1), (-1, +1))
BACKGROUND_DEPTH = np.float32(1.0)


def split(vol, cs):
    """packed cells -> (sum, count) as int64"""
    v = np.asarray(vol, np.uint32).astype(np.int64)
    return v & ((1 << cs) - 1), v >> cs


def seen_cells(vol, cs):
    return split(vol, cs)[1] != 0


def cost16(vol, cs, cap):
    """rule 1: C = min(floor(16 s / (255 n)), cap) (cs 24) or min(floor(16 s / n), cap) (cs 16); cap where n == 0"""
    s, n = split(vol, cs)
    den = np.where(n == 0, 1, n * 255 if cs == 24 else n)
    c = np.minimum((16 * s) // den, cap)
    return np.where(n == 0, cap, c).astype(np.int64)


def _step(c, prev, p1, p2):
    """one pixel step of rule 2 for any number of scan lines: c, prev are [N, D]"""
    m = prev.min(axis=1, keepdims=True)
    best = np.minimum(prev, m + p2)
    best[:, 1:] = np.minimum(best[:, 1:], prev[:, :-1] + p1)
    best[:, :-1] = np.minimum(best[:, :-1], prev[:, 1:] + p1)
    return c + best - m


def path_costs(C, dy, dx, p1, p2):
    """L_r for r = (dy, dx), [D, H, W] int64"""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    L = np.empty_like(C)
    if dy == 0:   # scan along the rows: a step handles column x of every row
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        prev = None
        for x in xs:
            c = C[:, :, x].T   # [H, D]
            cur = c.copy() if prev is None else _step(c, prev, p1, p2)
            L[:, :, x] = cur.T
            prev = cur
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    prev = None
    for y in ys:   # a step handles row y: the predecessor of column x is column x - dx of the row before
        c = C[:, y, :].T   # [W, D]
        if prev is None:
            cur = c.copy()
        else:
            src = np.arange(W) - dx
            inside = (src >= 0) & (src < W)
            cur = np.where(inside[:, None], _step(c, prev[np.clip(src, 0, W - 1)], p1, p2), c)
        L[:, y, :] = cur.T
        prev = cur
    return L


def winners(C, dy, dx, p1, p2):
    """which term of rule 2 gave L_r(p, d), int8 [D, H, W]: 0 the start of a path (p - r outside the image), 1 the own plane, 2 plane
    d - 1 plus P1, 3 plane d + 1 plus P1, 4 m + P2, -1 where the smallest term is not unique.  Derived from path_costs, and checked
    against it cell by cell."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    L = path_costs(C, dy, dx, p1, p2)
    ys, xs = np.arange(H) - dy, np.arange(W) - dx
    inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    prev = L[:, np.clip(ys, 0, H - 1)][:, :, np.clip(xs, 0, W - 1)]   # L_r(p - r, .), garbage where p - r is outside
    m = prev.min(axis=0, keepdims=True)
    absent = np.int64(1) << 40
    terms = np.full((4,) + C.shape, absent, np.int64)
    terms[0] = prev
    terms[1, 1:] = prev[:-1] + p1
    terms[2, :-1] = prev[1:] + p1
    terms[3] = m + p2
    least = terms.min(axis=0)
    assert (np.where(inside[None], C + least - m, C) == L).all()
    code = np.where((terms == least[None]).sum(axis=0) == 1, terms.argmin(axis=0) + 1, -1)
    return np.where(inside[None], code, 0).astype(np.int8)


def aggregate(C, paths, p1, p2):
    """rule 3: S = sum of L_r over the first `paths` directions, uint16 [D, H, W]"""
    assert paths in (4, 8)
    S = np.zeros(np.asarray(C).shape, np.int64)
    for dy, dx in PATHS[:paths]:
        S += path_costs(C, dy, dx, p1, p2)
    assert S.max() <= 65535
    return S.astype(np.uint16)


def select(S, seen, z, paths):
    """rule 4 -> (depth f32, cost f32, index i32), [H, W] each"""
    S = np.asarray(S)
    masked = np.where(seen, S.astype(np.int64), 1 << 40)
    index = masked.argmin(axis=0).astype(np.int32)   # the first of equal minima: the lowest plane
    any_seen = seen.any(axis=0)
    best = np.take_along_axis(S, index[None].astype(np.int64), axis=0)[0]
    cost = best.astype(np.float32) / np.float32(16 * paths)
    depth = np.asarray(z, np.float32)[index]
    index = np.where(any_seen, index, -1).astype(np.int32)
    return (np.where(any_seen, depth, BACKGROUND_DEPTH).astype(np.float32), np.where(any_seen, cost, np.float32(np.inf)).astype(np.float32), index)


def _fma32(a, b, c):
    """RN32(a b + c) for float32 arrays: the product is exact in float64; the one float64 rounding of the sum is undone where it
    landed on the midpoint of two float32 neighbours (two-sum gives the sign of what was rounded away)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    r = np.where((r64 > s) & (err < 0) & (((r64 - s) * 2) == np.abs(r64 - np.nextafter(r, np.float32(-np.inf)).astype(np.float64))),
                 np.nextafter(r, np.float32(-np.inf)), r)
    r = np.where((r64 < s) & (err > 0) & (((s - r64) * 2) == np.abs(np.nextafter(r, np.float32(np.inf)).astype(np.float64) - r64)),
                 np.nextafter(r, np.float32(np.inf)), r)
    return r.astype(np.float32)


def parabola(ca, cb, cc, ok, z, index):
    """the parabola of mvs_sweep_refine_depth through the f32 costs ca, cb, cc of the planes index - 1, index, index + 1 ([H, W] each; `ok`:
    the pixel has all three), f32 with one rounding per operation and the final fused multiply-add; a pixel that is not `ok`, or whose
    den is not positive, keeps z[index] (the background depth without an index).  Needs at least three planes."""
    z = np.asarray(z, np.float32)
    D = len(z)
    i = np.clip(index, 1, D - 2).astype(np.int64)
    den = (ca - np.float32(2.0) * cb) + cc
    ok = ok & (den > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.float32(0.5) * (ca - cc)) / den
    t = np.where(ok, t, np.float32(0)).astype(np.float32)
    t = np.clip(t, np.float32(-0.5), np.float32(0.5))
    zi = z[i]
    fwd = _fma32(t, z[i + 1] - zi, zi)
    bwd = _fma32(-t, z[i - 1] - zi, zi)
    zr = np.where(t >= 0, fwd, bwd)
    plain = np.where(index >= 0, z[np.clip(index, 0, D - 1)], BACKGROUND_DEPTH)
    return np.where(ok, zr, plain).astype(np.float32)


def refine(S, seen, z, index):
    """rule 5: depth map with the parabola of mvs_sweep_refine_depth on (float)S, f32 with one rounding per operation"""
    S = np.asarray(S)
    D, H, W = S.shape
    i = np.clip(index, 1, D - 2).astype(np.int64)[None]
    ca = np.take_along_axis(S, i - 1, axis=0)[0].astype(np.float32)
    cb = np.take_along_axis(S, i, axis=0)[0].astype(np.float32)
    cc = np.take_along_axis(S, i + 1, axis=0)[0].astype(np.float32)
    ok = (index > 0) & (index < D - 1)
    for k in (-1, 0, 1):
        ok &= np.take_along_axis(seen, i + k, axis=0)[0]
    return parabola(ca, cb, cc, ok, z, index)
