"""Restatement of the depth-map filter, written from the contract and not from the kernel.  It is the arbiter:
mvs_depth_filter must be bit-identical to filter().

Two statements that share nothing: the array path (median(), mean(), filter(): whole maps, one shifted copy of the map per window
position) and brute_pixel() (one pixel, Python loops over the window, Python's sorted()).  tests/test_depth_filter_cpu.py holds them
against each other at every pixel of the crafted maps.  Everything is float32: one rounding per operation."""
import numpy as np

f32 = np.float32
BACKGROUND_DEPTH = f32(1.0)
MEDIAN, MEAN, FILL = 1, 2, 4
INF = float("inf")


def valid(z):
    """rule 1: -1 < z < 1 (false for NaN, the infinities, -1 and 1)"""
    with np.errstate(invalid="ignore"):
        return (z > f32(-1.0)) & (z < f32(1.0))


def read(z):
    """rule 1: a valid value is read as z + 0.0f (-0.0 becomes +0.0); an invalid one as NaN, which nothing below uses as a number"""
    z = np.asarray(z, f32)
    with np.errstate(invalid="ignore"):
        return np.where(valid(z), z + f32(0.0), f32(np.nan)).astype(f32)


def offsets(radius):
    """rule 2: the window's positions (drow, dcol) in row-major order"""
    return [(dr, dc) for dr in range(-radius, radius + 1) for dc in range(-radius, radius + 1)]


def _shifted(a, dr, dc, outside):
    """a[row + dr, col + dc] for every (row, col), `outside` where that is no pixel of the frame"""
    H, W = a.shape
    out = np.full((H, W), outside, a.dtype)
    r0, r1, c0, c1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def _guide_gate(guide, tau, dr, dc, shape):
    """rule 2: |G(q) - G(p)| <= tau in integers; tau = 255: every pixel passes and G is not read"""
    if tau >= 255:
        return np.ones(shape, bool)
    g = np.asarray(guide, np.uint8).astype(np.int64)
    return np.abs(_shifted(g, dr, dc, 0) - g) <= tau


def median(depth, radius, tau=255, guide=None, fill=False, min_members=1):
    """rule 3 -> the median stage's map"""
    v = read(depth)
    ok = valid(v)
    cols = []
    for dr, dc in offsets(radius):
        q = _shifted(v, dr, dc, f32(np.nan))
        member = valid(q) & _guide_gate(guide, tau, dr, dc, v.shape)
        cols.append(np.where(member, q, f32(np.inf)))            # a pixel that is no member sorts behind every member
    stack = np.sort(np.stack(cols), axis=0)
    n = np.isfinite(stack).sum(axis=0)
    rank = np.maximum(n - 1, 0) // 2                             # the lower median
    med = np.take_along_axis(stack, rank[None], axis=0)[0]
    take = ok | (bool(fill) & (n >= min_members) & (n >= 1))
    return np.where(take, med, BACKGROUND_DEPTH).astype(f32)


def mean(m, radius, tau=255, max_step=INF, guide=None, gate=None):
    """rule 4 -> the mean stage's map of m; gate: the map the depth gate compares, which is m itself"""
    v = read(m)
    ok = valid(v)
    gate_v = v if gate is None else read(gate)
    step = f32(max_step)
    total = np.zeros(v.shape, f32)
    n = np.zeros(v.shape, np.int64)
    for dr, dc in offsets(radius):                               # window order: the sum takes its members one at a time
        q, gate_q = _shifted(v, dr, dc, f32(np.nan)), _shifted(gate_v, dr, dc, f32(np.nan))
        with np.errstate(invalid="ignore"):
            near = np.abs(gate_q - gate_v) <= step               # one float32 subtraction; false for NaN on either side
            member = ok & valid(q) & _guide_gate(guide, tau, dr, dc, v.shape) & near
            total = np.where(member, total + q, total).astype(f32)
        n += member
    with np.errstate(invalid="ignore", divide="ignore"):
        out = total / n.astype(f32)
    assert out.dtype == f32
    return np.where(ok, out, BACKGROUND_DEPTH).astype(f32)


def filter(depth, radius, tau=255, max_step=INF, guide=None, flags=MEDIAN | MEAN, min_members=1):
    """mvs_depth_filter -> the filtered map"""
    assert flags & (MEDIAN | MEAN) and not flags & ~(MEDIAN | MEAN | FILL) and (flags & MEDIAN or not flags & FILL)
    m = np.asarray(depth, f32)
    if flags & MEDIAN:
        m = median(m, radius, tau, guide, bool(flags & FILL), min_members)
    if flags & MEAN:
        m = mean(m, radius, tau, max_step, guide)
    return m


# ---- one pixel at a time ------------------------------------------------------------------------------------------------------------
def _is_valid(z):
    z = float(z)
    return -1.0 < z < 1.0          # (False for NaN)


def _window(depth, guide, row, col, radius, tau):
    """the valid pixels of the window that pass the guide gate, as float32 scalars in window order"""
    H, W = depth.shape
    out = []
    for r in range(row - radius, row + radius + 1):
        for c in range(col - radius, col + radius + 1):
            if r < 0 or r >= H or c < 0 or c >= W or not _is_valid(depth[r, c]):
                continue
            if tau < 255 and abs(int(guide[r, c]) - int(guide[row, col])) > tau:
                continue
            out.append(f32(depth[r, c]) + f32(0.0))
    return out


def brute_median_pixel(depth, row, col, radius, tau=255, guide=None, fill=False, min_members=1):
    members = _window(depth, guide, row, col, radius, tau)
    if _is_valid(depth[row, col]) or (fill and len(members) >= max(min_members, 1)):
        return sorted(members, key=float)[(len(members) - 1) // 2]
    return BACKGROUND_DEPTH


def brute_mean_pixel(m, row, col, radius, tau=255, max_step=INF, guide=None):
    if not _is_valid(m[row, col]):
        return BACKGROUND_DEPTH
    centre = f32(m[row, col]) + f32(0.0)
    total, n = f32(0.0), 0
    for q in _window(m, guide, row, col, radius, tau):
        if abs(f32(q - centre)) <= f32(max_step):
            total = f32(total + q)
            n += 1
    return f32(total / f32(n))


def brute_pixel(depth, row, col, radius, tau=255, max_step=INF, guide=None, flags=MEDIAN | MEAN, min_members=1):
    """mvs_depth_filter at one pixel, with Python loops: the mean stage's input is the median of every pixel of ITS window"""
    depth = np.asarray(depth, f32)
    if not flags & MEAN:
        return brute_median_pixel(depth, row, col, radius, tau, guide, bool(flags & FILL), min_members)
    if not flags & MEDIAN:
        return brute_mean_pixel(depth, row, col, radius, tau, max_step, guide)
    H, W = depth.shape
    m = np.full((H, W), np.nan, f32)
    for r in range(max(0, row - radius), min(H, row + radius + 1)):
        for c in range(max(0, col - radius), min(W, col + radius + 1)):
            m[r, c] = brute_median_pixel(depth, r, c, radius, tau, guide, bool(flags & FILL), min_members)
    return brute_mean_pixel(m, row, col, radius, tau, max_step, guide)
