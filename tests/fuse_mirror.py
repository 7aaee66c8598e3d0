"""numpy restatement of mvs_fuse_depth (csrc/fuse.hip; the contract: DESIGN.md section 11, include/mvs.h).

fuse(..., dtype=np.float32) follows the kernels' order of operations with the matrices mvs_depth_slot_matrices returns: numpy rounds
every float32 operation once, as the kernels do when built without contraction (-ffp-contract=off), and `/` and sqrt are correctly
rounded on both sides.  So keep mask, count and rows are expected bit for bit -- no value of the contract needs a tolerance.
The one fused operation of the kernels, the sweep's pixel centre fmaf((float)(2 c + 1), 1/W, -1), is restated in float64 and rounded
once: the product of an integer below 2^15 and a float32 is exact in 53 bits, and so is its sum with -1 at these sizes.

dtype=np.float64 runs the same formulas in double (matrices inverted in double, pixel centres unrounded): the analytic checks of
tests/test_fuse_cpu.py use it as the reference the float32 path is compared against.
"""
import numpy as np


def slot_matrices(cam):
    """host-side matrices of one slot in float64: (P, P^-1, centre (x, y, z, 1)).  The library inverts by cofactors (invert4) and rounds
    once; np.linalg.inv may differ from it in the last bit of a double, so for bit-exact work take mvs_depth_slot_matrices instead."""
    P = np.asarray(cam, np.float64).reshape(4, 4)
    Pi = np.linalg.inv(P)
    p = P[[0, 1, 3]]
    h = np.array([(-1.0) ** i * np.linalg.det(np.delete(p, i, axis=1)) for i in range(4)])
    return P, Pi, np.array([h[0] / h[3], h[1] / h[3], h[2] / h[3], 1.0])


def pixel_xn(col, W, t=np.float32):
    if t is np.float64:
        return (2.0 * col + 1.0) / W - 1.0
    invW = np.float32(1.0) / np.float32(W)
    return ((2 * np.asarray(col, np.int64) + 1).astype(np.float64) * np.float64(invW) - 1.0).astype(np.float32)


def pixel_yn(row, H, t=np.float32):
    if t is np.float64:
        return 1.0 - (2.0 * row + 1.0) / H
    invH = np.float32(1.0) / np.float32(H)
    return ((-(2 * np.asarray(row, np.int64) + 1)).astype(np.float64) * np.float64(invH) + 1.0).astype(np.float32)


def _unproject(Pi, xn, yn, z):
    h = [((Pi[i, 0] * xn + Pi[i, 1] * yn) + Pi[i, 2] * z) + Pi[i, 3] for i in range(4)]
    return h[0] / h[3], h[1] / h[3], h[2] / h[3]


def _prow(P, i, X):
    return ((P[i, 0] * X[0] + P[i, 1] * X[1]) + P[i, 2] * X[2]) + P[i, 3]


def _valid(z, cost, max_cost, t):
    ok = (z > t(-1.0)) & (z < t(1.0))
    if max_cost < np.inf:
        ok &= cost <= t(max_cost)
    return ok


def fuse(depths, costs, mats, ref, neighbours, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, max_cost=np.inf, dtype=np.float32):
    """depths / costs: slot -> [H, W] maps (costs may lack entries when max_cost is infinite); mats: slot -> (P, P^-1, centre).
    Returns a dict: keep [H, W] bool, rows (N, 7) in ascending pixel index, and per-pixel intermediates (X, w, normal, agree, has_normal, and
    per neighbour the two quantities the thresholds are compared with)."""
    t = dtype
    H, W = depths[ref].shape
    halfW, halfH = t(W) * t(0.5), t(H) * t(0.5)
    max_rel = t(max_rel_depth)
    reproj2 = t(max_reproj_px) * t(max_reproj_px)
    rows_i, cols_i = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        P0, Pi0, C0 = [np.asarray(m, t) for m in mats[ref]]
        z0 = np.asarray(depths[ref], t)
        ok = _valid(z0, None if max_cost == np.inf else np.asarray(costs[ref], t), max_cost, t)
        X = _unproject(Pi0, pixel_xn(cols_i, W, t), pixel_yn(rows_i, H, t), z0)
        w = _prow(P0, 3, X)
        ok &= w > t(0.0)
        # the kernels' LDS tile: (x, y, z, w) with w = 0 for a pixel that is not valid, zero outside the image
        T = np.zeros((4, H + 2, W + 2), t)
        for k, a in enumerate((X[0], X[1], X[2], w)):
            T[k, 1:-1, 1:-1] = np.where(ok, a, t(0.0))
        c = T[:, 1:-1, 1:-1]

        def usable(n):
            return (n[3] > t(0.0)) & (np.abs(n[3] - c[3]) / c[3] <= max_rel)

        def tangent(lo, hi):
            ul, uh = usable(lo), usable(hi)
            tv = [np.where(ul & uh, hi[k] - lo[k], np.where(uh, hi[k] - c[k], c[k] - lo[k])) for k in range(3)]
            return tv, ul | uh

        tc, hc = tangent(T[:, 1:-1, :-2], T[:, 1:-1, 2:])
        tr, hr = tangent(T[:, :-2, 1:-1], T[:, 2:, 1:-1])
        nx = tc[1] * tr[2] - tc[2] * tr[1]
        ny = tc[2] * tr[0] - tc[0] * tr[2]
        nz = tc[0] * tr[1] - tc[1] * tr[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        has_normal = ok & hc & hr & (ln > t(0.0)) & (ln < t(np.inf))
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        flip = (nx * (C0[0] - c[0]) + ny * (C0[1] - c[1])) + nz * (C0[2] - c[2]) < t(0.0)
        nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)

        Xc = (c[0], c[1], c[2])
        sx, sy, sz = c[0].copy(), c[1].copy(), c[2].copy()
        agree = np.zeros((H, W), np.int32)
        tests = []   # per neighbour: (the sample reached both threshold tests, du^2 + dv^2, |sw - w| / w)
        colf, rowf = cols_i.astype(t), rows_i.astype(t)
        for j in neighbours:
            Pj, Pij, _ = [np.asarray(m, t) for m in mats[j]]
            dj = np.asarray(depths[j], t)
            qw = _prow(Pj, 3, Xc)
            u = (_prow(Pj, 0, Xc) / qw + t(1.0)) * halfW - t(0.5)
            v = (t(1.0) - _prow(Pj, 1, Xc) / qw) * halfH - t(0.5)
            fc, fr = np.floor(u + t(0.5)), np.floor(v + t(0.5))
            inb = (qw > t(0.0)) & (fc >= t(0.0)) & (fc < t(W)) & (fr >= t(0.0)) & (fr < t(H))
            cj = np.where(inb, fc, 0).astype(np.int64)
            rj = np.where(inb, fr, 0).astype(np.int64)
            zj = dj[rj, cj]
            vj = inb & _valid(zj, None if max_cost == np.inf else np.asarray(costs[j], t)[rj, cj], max_cost, t)
            Xj = _unproject(Pij, pixel_xn(cj, W, t), pixel_yn(rj, H, t), zj)
            sw = _prow(P0, 3, Xj)
            ur = (_prow(P0, 0, Xj) / sw + t(1.0)) * halfW - t(0.5)
            vr = (t(1.0) - _prow(P0, 1, Xj) / sw) * halfH - t(0.5)
            du, dv = ur - colf, vr - rowf
            d2, rel = du * du + dv * dv, np.abs(sw - c[3]) / c[3]
            a = vj & (sw > t(0.0)) & (d2 <= reproj2) & (rel <= max_rel)
            tests.append((vj & (sw > t(0.0)), d2, rel))
            sx = np.where(a, sx + Xj[0], sx)
            sy = np.where(a, sy + Xj[1], sy)
            sz = np.where(a, sz + Xj[2], sz)
            agree += a
        keep = has_normal & (agree >= min_consistent)
        n = (agree + 1).astype(t)
        allrows = np.stack([sx / n, sy / n, sz / n, np.ones((H, W), t), nx, ny, nz], axis=-1)
    return {"keep": keep, "rows": allrows[keep].astype(t), "X": np.stack(Xc, -1), "w": c[3], "valid": ok, "has_normal": has_normal,
            "normal": np.stack([nx, ny, nz], -1), "agree": agree, "tests": tests}
