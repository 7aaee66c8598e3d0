"""Restatement of the ZNCC sweep, written from the contract and not from the kernel.  It is the arbiter:
mvs_sweep_run_zncc must be bit-identical to volume().

Rule 1: B and ok of a (plane, view) are what oracle.warp_by_depth(main_cam, full(z_d), side_cam, frame, sampler="fixed") returns: the
oracle's fixed-sampler sample at every pixel, (dot + 127) / 255 and the frame test.  (That function reads a depth of exactly 1.0 as
"no depth"; a plane table from oracle.plane_table never holds 1.0, and volume() refuses one that does.)  Rules 2-3 are integer arrays
(int64), rule 4 is float32 with one numpy operation per rounding.  Selection and refinement on the volume are
oracle.argmin(..., sampler="fixed") and oracle.refine_depth(..., sampler="fixed")."""
import numpy as np

SCALE = np.float32(32512.0)


def box(x, r):
    """[H, W] int64 -> the sum over the (2 r + 1)^2 window of every pixel; pixels outside the frame add nothing"""
    H, W = x.shape
    ii = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    ii[r + 1:r + 1 + H, r + 1:r + 1 + W] = x
    ii = ii.cumsum(0).cumsum(1)         # ii[i, j] = the sum of the frame, padded by r zeros all round, above row i and left of column j
    n = 2 * r + 1
    return ii[n:n + H, n:n + W] - ii[:H, n:n + W] - ii[n:n + H, :W] + ii[:H, :W]


def cost_of_sums(N, Sa, Sb, Sab, Saa, Sbb, centre_ok):
    """rules 3-4 on integer arrays -> (counted bool, c uint32; c is 0 where the view does not count)"""
    cov, va, vb = N * Sab - Sa * Sb, N * Saa - Sa * Sa, N * Sbb - Sb * Sb
    assert np.abs(cov).max(initial=0) < 2 ** 31 and va.max(initial=0) < 2 ** 31 and vb.max(initial=0) < 2 ** 31
    counted = centre_ok & (va > 0) & (vb > 0)
    den = np.sqrt(np.where(counted, va, 1).astype(np.float32) * np.where(counted, vb, 1).astype(np.float32))
    ncc = cov.astype(np.float32) / den
    ncc = np.minimum(np.maximum(ncc, np.float32(-1.0)), np.float32(1.0))
    c = np.floor(SCALE * (np.float32(1.0) - ncc))
    assert den.dtype == np.float32 and ncc.dtype == np.float32 and c.dtype == np.float32
    return counted, np.where(counted, c, 0).astype(np.uint32)


def view_cost(A, B, ok, r):
    """rules 2-4 for one (plane, view): A the main image, B / ok the warped frame and its frame test -> (counted, c)"""
    A, B = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    m = np.asarray(ok).astype(np.int64)          # the members
    return cost_of_sums(box(m, r), box(m * A, r), box(m * B, r), box(m * A * B, r), box(m * A * A, r), box(m * B * B, r), np.asarray(ok, bool))


def warped(oracle, main_cam, side_cam, frame, z):
    """rule 1 -> (B [H, W] uint8, ok [H, W] bool)"""
    frame = np.asarray(frame, np.uint8)
    out = oracle.warp_by_depth(main_cam, np.full(frame.shape, z, np.float32), side_cam, frame, sampler="fixed")
    return out[..., 0], out[..., 1] != 0


def view_volume(oracle, main_cam, main_img, side_cam, frame, z, r):
    """one view over the planes z -> (ok [D, H, W] bool: the centre's sample is in frame, counted [D, H, W] bool, c [D, H, W] uint32)"""
    z = np.asarray(z, np.float32)
    assert 1 <= r <= 4 and not (z == np.float32(1.0)).any()
    parts = []
    for zd in z:
        B, ok = warped(oracle, main_cam, side_cam, frame, zd)
        parts.append((ok,) + view_cost(main_img, B, ok, r))
    return tuple(np.stack(a) for a in zip(*parts))


def cells(counted, c):
    """rule 5 for one view"""
    return np.where(counted, np.uint32(1 << 24) + c, np.uint32(0)).astype(np.uint32)


def volume(oracle, main_cam, main_img, side_cams, side_imgs, z, r, views=None):
    """the packed volume [D, H, W] uint32 of the ZNCC sweep over the side views `views` (default: all)"""
    views = range(len(side_imgs)) if views is None else views
    vol = np.zeros((len(z),) + np.asarray(main_img).shape, np.uint32)
    for v in views:
        _, counted, c = view_volume(oracle, main_cam, main_img, side_cams[v], side_imgs[v], z, r)
        vol += cells(counted, c)
    return vol


def brute_cell(A, B, ok, r, row, col):
    """rules 2-4 at one pixel with loops and scalars, sharing nothing with the functions above -> (N, counted, c)"""
    H, W = A.shape
    q = [(y, x) for y in range(row - r, row + r + 1) for x in range(col - r, col + r + 1) if 0 <= y < H and 0 <= x < W and ok[y, x]]
    a, b = [int(A[p]) for p in q], [int(B[p]) for p in q]
    N, Sa, Sb = len(q), sum(a), sum(b)
    Sab, Saa, Sbb = sum(x * y for x, y in zip(a, b)), sum(x * x for x in a), sum(y * y for y in b)
    cov, va, vb = N * Sab - Sa * Sb, N * Saa - Sa * Sa, N * Sbb - Sb * Sb          # Python integers
    if not (ok[row, col] and va > 0 and vb > 0):
        return N, False, 0
    f = np.float32
    den = np.sqrt(f(va) * f(vb))
    ncc = min(max(f(cov) / den, f(-1.0)), f(1.0))
    c = np.floor(f(32512.0) * (f(1.0) - ncc))
    assert all(type(x) is np.float32 for x in (den, ncc, c))
    return N, True, int(c)
