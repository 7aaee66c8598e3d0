"""Restatement of the depth-map plane fit, written from the contract and not from the kernel.  It is the arbiter:
mvs_depth_fit must be bit-identical to fit() with dtype=float32.

Two statements that share nothing but the validity test: the array path (fit(): whole maps, one shifted copy of the map per window
position) and brute_pixel() (one pixel, Python loops over the window).  tests/test_depth_fit_cpu.py holds them against each other on the
crafted maps.  dtype=float32 rounds every operation once, as the kernel does when built without contraction; dtype=float64 runs the same
rules in double on the same members (the gates stay float32 decisions, so both paths fit the same pixels): the reference the float32
path's error is measured against, together with lstsq_pixel(), numpy's own least squares."""
import collections

import numpy as np

import depth_filter_mirror as dm

f32 = np.float32
BACKGROUND_DEPTH = f32(1.0)
INF = float("inf")
valid, read, offsets = dm.valid, dm.read, dm.offsets      # rules F1 and F2 are section 23's rules 1 and 2

Fit = collections.namedtuple("Fit", "z gx gy zfit members report c D")


def fit(depth, radius, tau=255, max_step=INF, min_members=6, guide=None, dtype=f32):
    """mvs_depth_fit -> Fit(z, gx, gy, zfit [H, W] dtype, members [H, W] uint8, report [4] (valid centres, fitted, refused for
    n < min_members, refused for D = 0), c [H, W] dtype: the fitted plane's offset at the centre, 0 unless fitted; D [H, W] int64: rule F5's determinant)"""
    t_ = dtype
    v = read(depth)
    ok = valid(v)
    vt = v if t_ is f32 else np.where(ok, np.asarray(depth, t_) + t_(0.0), t_(np.nan))   # (float64: the map as given, not rounded to float32)
    step = f32(max_step)
    shape = v.shape
    n, Sx, Sy, Sxx, Sxy, Syy = (np.zeros(shape, np.int64) for _ in range(6))
    St, Sxt, Syt = (np.zeros(shape, t_) for _ in range(3))
    for dr, dc in offsets(radius):                               # rule F4: window order, a member at a time
        q = dm._shifted(v, dr, dc, f32(np.nan))
        with np.errstate(invalid="ignore"):
            gate_t = q - v                                       # rule F3: one float32 subtraction, NaN for an invalid q or p
            member = ok & valid(q) & dm._guide_gate(guide, tau, dr, dc, shape) & (np.abs(gate_t) <= step)
            t = gate_t if t_ is f32 else dm._shifted(vt, dr, dc, t_(np.nan)) - vt
            St = np.where(member, St + t, St).astype(t_)
            Sxt = np.where(member, Sxt + t_(dc) * t, Sxt).astype(t_)
            Syt = np.where(member, Syt + t_(dr) * t, Syt).astype(t_)
        m = member.astype(np.int64)
        n += m
        Sx += m * dc
        Sy += m * dr
        Sxx += m * dc * dc
        Sxy += m * dc * dr
        Syy += m * dr * dr
    # rule F5: the adjugate of the moment matrix [[n, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]] in integers
    A00 = Sxx * Syy - Sxy * Sxy
    A01 = Sy * Sxy - Sx * Syy
    A02 = Sx * Sxy - Sy * Sxx
    A11 = n * Syy - Sy * Sy
    A12 = Sx * Sy - n * Sxy
    A22 = n * Sxx - Sx * Sx
    D = n * A00 + Sx * A01 + Sy * A02
    assert all(np.abs(a).max() < 2 ** 24 for a in (A00, A01, A02, A11, A12, A22)) and 0 <= D.min() and D.max() < 2 ** 31
    fitted = ok & (n >= min_members) & (D != 0)
    A00, A01, A02, A11, A12, A22, Df = (a.astype(t_) for a in (A00, A01, A02, A11, A12, A22, D))
    with np.errstate(all="ignore"):
        c = ((A00 * St + A01 * Sxt) + A02 * Syt) / Df
        gx = ((A01 * St + A11 * Sxt) + A12 * Syt) / Df
        gy = ((A02 * St + A12 * Sxt) + A22 * Syt) / Df
        z = np.where(ok, vt, BACKGROUND_DEPTH).astype(t_)
        moved = vt + c
        zfit = np.where(fitted & (moved > t_(-1.0)) & (moved < t_(1.0)), moved, z).astype(t_)
    gx = np.where(fitted, gx, t_(0.0)).astype(t_)
    gy = np.where(fitted, gy, t_(0.0)).astype(t_)
    c = np.where(fitted, c, t_(0.0)).astype(t_)
    members = np.where(fitted, n, 0).astype(np.uint8)
    report = [int(ok.sum()), int(fitted.sum()), int((ok & (n < min_members)).sum()), int((ok & (n >= min_members) & (D == 0)).sum())]
    return Fit(z, gx, gy, zfit, members, report, c, D)


def normals(f, P, C, dtype=f32):
    """mvs_depth_fit_normals: rule N1 (normals_mirror.hypothesis_normals) on the fit's (z, gx, gy), zeros for a pixel that is not fitted"""
    import normals_mirror as nm
    n = nm.hypothesis_normals(f.z, f.gx, f.gy, P, C, dtype)
    return np.where((f.members > 0)[..., None], n, dtype(0.0)).astype(dtype)


# ---- one pixel at a time ------------------------------------------------------------------------------------------------------------
def window_members(depth, row, col, radius, tau=255, max_step=INF, guide=None):
    """rule F3 at one pixel -> [(dc, dr, t float32)] in window order; empty for an invalid centre"""
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    if not dm._is_valid(depth[row, col]):
        return []
    centre = f32(depth[row, col]) + f32(0.0)
    out = []
    for r in range(row - radius, row + radius + 1):
        for c in range(col - radius, col + radius + 1):
            if r < 0 or r >= H or c < 0 or c >= W or not dm._is_valid(depth[r, c]):
                continue
            if tau < 255 and abs(int(guide[r, c]) - int(guide[row, col])) > tau:
                continue
            t = f32((f32(depth[r, c]) + f32(0.0)) - centre)
            if abs(t) <= f32(max_step):
                out.append((c - col, r - row, t))
    return out


def brute_pixel(depth, row, col, radius, tau=255, max_step=INF, min_members=6, guide=None):
    """mvs_depth_fit at one pixel with Python loops, float32 -> (z, gx, gy, zfit, members)"""
    depth = np.asarray(depth, f32)
    if not dm._is_valid(depth[row, col]):
        return BACKGROUND_DEPTH, f32(0.0), f32(0.0), BACKGROUND_DEPTH, 0
    z = f32(depth[row, col]) + f32(0.0)
    mem = window_members(depth, row, col, radius, tau, max_step, guide)
    n = len(mem)
    Sx, Sy = sum(dc for dc, _, _ in mem), sum(dr for _, dr, _ in mem)
    Sxx, Sxy, Syy = sum(dc * dc for dc, _, _ in mem), sum(dc * dr for dc, dr, _ in mem), sum(dr * dr for _, dr, _ in mem)
    St = Sxt = Syt = f32(0.0)
    for dc, dr, t in mem:
        St = f32(St + t)
        Sxt = f32(Sxt + f32(f32(dc) * t))
        Syt = f32(Syt + f32(f32(dr) * t))
    M = [[n, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]]                       # Python integers: the cofactors by their definition

    def cof(i, j):
        r, c = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
        return (-1) ** (i + j) * (M[r[0]][c[0]] * M[r[1]][c[1]] - M[r[0]][c[1]] * M[r[1]][c[0]])

    D = sum(M[0][j] * cof(0, j) for j in range(3))
    if n < min_members or D == 0:
        return z, f32(0.0), f32(0.0), z, 0
    s = (St, Sxt, Syt)
    with np.errstate(all="ignore"):
        sol = [f32(f32(f32(f32(cof(k, 0)) * s[0]) + f32(f32(cof(k, 1)) * s[1])) + f32(f32(cof(k, 2)) * s[2])) / f32(D) for k in range(3)]
        moved = f32(z + sol[0])
    return z, f32(sol[1]), f32(sol[2]), (moved if -1.0 < float(moved) < 1.0 else z), n


def lstsq_pixel(depth, row, col, radius, tau=255, max_step=INF, guide=None):
    """numpy's least squares in float64 over the members of rule F3 -> (c, gx, gy), or None when the members are collinear"""
    mem = window_members(depth, row, col, radius, tau, max_step, guide)
    if len(mem) < 3:
        return None
    A = np.array([[1.0, dc, dr] for dc, dr, _ in mem])
    if np.linalg.matrix_rank(A) < 3:
        return None
    centre = np.float64(f32(depth[row, col]))
    b = np.array([np.float64(f32(depth[row + dr, col + dc])) - centre for dc, dr, _ in mem])
    return np.linalg.lstsq(A, b, rcond=None)[0]
