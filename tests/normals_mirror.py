"""numpy restatement of DESIGN.md section 31 (csrc/normals.hip, include/mvs.h "normals"): rule N1 (mvs_propagate_normals), the usable test
of a stored normal, and mvs_fuse_depth_normals (rules 1s-5 of sections 11 / 28 with rules 3n and 5n).

Written from the section's text.  dtype=np.float32 follows the kernels' order of operations: numpy rounds every float32 operation once,
as the kernels do when built without contraction, `/` and sqrt are correctly rounded on both sides, and the pixel centres' fmaf is
fuse_mirror's (float64, rounded once).  So normal maps, keep masks, counts and rows are expected bit for bit.  dtype=np.float64 runs the
same formulas in double: the analytic checks of tests/test_normals_cpu.py use it as the reference the float32 path is compared against.
"""
import numpy as np

import fuse_mirror as fm
import fuse_sequence_mirror as sm


def hypothesis_normals(z, gx, gy, P, C, dtype=np.float32):
    """rule N1: z, gx, gy [H, W] (the propagation's maps), P the main camera (4 x 4, clip = P X), C its centre -> [H, W, 3] unit normals
    toward the camera's side of each pixel's plane, zeros where there is none"""
    t = dtype
    z, gx, gy = (np.asarray(a, t) for a in (z, gx, gy))
    H, W = z.shape
    P = np.asarray(P, t).reshape(4, 4)
    C = np.asarray(C, t).reshape(-1)
    rows_i, cols_i = np.mgrid[0:H, 0:W]
    halfW, halfH = t(W) * t(0.5), t(H) * t(0.5)
    with np.errstate(all="ignore"):
        xn, yn = fm.pixel_xn(cols_i, W, t), fm.pixel_yn(rows_i, H, t)
        a = -gx * halfW
        b = gy * halfH
        d = -((z + a * xn) + b * yn)
        m = [((a * P[0, k] + b * P[1, k]) + P[2, k]) + d * P[3, k] for k in range(4)]
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        ok = (z > t(-1.0)) & (z < t(1.0)) & (ln > t(0.0)) & (ln < t(np.inf))
        n = [m[k] / ln for k in range(3)]
        flip = ((m[0] * C[0] + m[1] * C[1]) + m[2] * C[2]) + m[3] < t(0.0)
        n = [np.where(flip, -v, v) for v in n]
    return np.stack([np.where(ok, v, t(0.0)) for v in n], axis=-1).astype(t)


def usable(n, t=np.float32):
    """a stored normal [..., 3] is usable when 0.5 < (nx nx + ny ny) + nz nz < 2 (false for zeros, NaN and infinities)"""
    n = np.asarray(n, t)
    with np.errstate(all="ignore"):
        s = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        return (s > t(0.5)) & (s < t(2.0))


def fuse_normals(depths, costs, supports, normals, mats, ref, neighbours, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, max_cost=np.inf,
                 min_support=0, min_normal_cos=-np.inf, dtype=np.float32):
    """mvs_fuse_depth_normals.  depths / costs / supports: slot -> [H, W]; normals: slot -> [H, W, 3] (a slot without an entry has no plane);
    mats: slot -> (P, P^-1, centre).  Returns a dict: keep [H, W], rows (N, 7) in ascending pixel index, and per pixel agree, has_normal,
    ref_usable (rule 5n applies), tangent_ok (rule 5's own normal exists), normal, X, w, valid, and per neighbour `tests` as fuse_mirror's
    plus `dots`: (the voter passed rule 3 and both normals are usable, the dot product of rule 3n)"""
    t = dtype
    depths = sm.masked(depths, supports, min_support)   # rule 1s
    H, W = np.asarray(depths[ref]).shape
    halfW, halfH = t(W) * t(0.5), t(H) * t(0.5)
    max_rel = t(max_rel_depth)
    reproj2 = t(max_reproj_px) * t(max_reproj_px)
    min_cos = t(min_normal_cos)
    rows_i, cols_i = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        P0, Pi0, C0 = [np.asarray(m, t) for m in mats[ref]]
        z0 = np.asarray(depths[ref], t)
        ok = fm._valid(z0, None if max_cost == np.inf else np.asarray(costs[ref], t), max_cost, t)
        X = fm._unproject(Pi0, fm.pixel_xn(cols_i, W, t), fm.pixel_yn(rows_i, H, t), z0)
        w = fm._prow(P0, 3, X)
        ok &= w > t(0.0)
        T = np.zeros((4, H + 2, W + 2), t)
        for k, a in enumerate((X[0], X[1], X[2], w)):
            T[k, 1:-1, 1:-1] = np.where(ok, a, t(0.0))
        c = T[:, 1:-1, 1:-1]

        def same_surface(n):
            return (n[3] > t(0.0)) & (np.abs(n[3] - c[3]) / c[3] <= max_rel)

        def tangent(lo, hi):
            ul, uh = same_surface(lo), same_surface(hi)
            tv = [np.where(ul & uh, hi[k] - lo[k], np.where(uh, hi[k] - c[k], c[k] - lo[k])) for k in range(3)]
            return tv, ul | uh

        def toward_camera(nx, ny, nz):
            flip = (nx * (C0[0] - c[0]) + ny * (C0[1] - c[1])) + nz * (C0[2] - c[2]) < t(0.0)
            return np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)

        # rule 5: the normal of the reference map's own neighbours
        tc, hc = tangent(T[:, 1:-1, :-2], T[:, 1:-1, 2:])
        tr, hr = tangent(T[:, :-2, 1:-1], T[:, 2:, 1:-1])
        nx = tc[1] * tr[2] - tc[2] * tr[1]
        ny = tc[2] * tr[0] - tc[0] * tr[2]
        nz = tc[0] * tr[1] - tc[1] * tr[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        tangent_ok = hc & hr & (ln > t(0.0)) & (ln < t(np.inf))
        tnx, tny, tnz = toward_camera(nx / ln, ny / ln, nz / ln)

        # rule 5n: the reference's stored normal starts the sum
        nr = np.asarray(normals[ref], t) if ref in normals else np.zeros((H, W, 3), t)
        ur = usable(nr, t) if ref in normals else np.zeros((H, W), bool)
        ax, ay, az = nr[..., 0].copy(), nr[..., 1].copy(), nr[..., 2].copy()

        Xc = (c[0], c[1], c[2])
        sx, sy, sz = c[0].copy(), c[1].copy(), c[2].copy()
        agree = np.zeros((H, W), np.int32)
        tests, dots = [], []
        colf, rowf = cols_i.astype(t), rows_i.astype(t)
        for j in neighbours:
            Pj, Pij, _ = [np.asarray(m, t) for m in mats[j]]
            dj = np.asarray(depths[j], t)
            qw = fm._prow(Pj, 3, Xc)
            u = (fm._prow(Pj, 0, Xc) / qw + t(1.0)) * halfW - t(0.5)
            v = (t(1.0) - fm._prow(Pj, 1, Xc) / qw) * halfH - t(0.5)
            fc, fr = np.floor(u + t(0.5)), np.floor(v + t(0.5))
            inb = (qw > t(0.0)) & (fc >= t(0.0)) & (fc < t(W)) & (fr >= t(0.0)) & (fr < t(H))
            cj = np.where(inb, fc, 0).astype(np.int64)
            rj = np.where(inb, fr, 0).astype(np.int64)
            zj = dj[rj, cj]
            vj = inb & fm._valid(zj, None if max_cost == np.inf else np.asarray(costs[j], t)[rj, cj], max_cost, t)
            Xj = fm._unproject(Pij, fm.pixel_xn(cj, W, t), fm.pixel_yn(rj, H, t), zj)
            sw = fm._prow(P0, 3, Xj)
            ur_ = (fm._prow(P0, 0, Xj) / sw + t(1.0)) * halfW - t(0.5)
            vr_ = (t(1.0) - fm._prow(P0, 1, Xj) / sw) * halfH - t(0.5)
            du, dv = ur_ - colf, vr_ - rowf
            d2, rel = du * du + dv * dv, np.abs(sw - c[3]) / c[3]
            rule3 = vj & (sw > t(0.0)) & (d2 <= reproj2) & (rel <= max_rel)
            # rule 3n: voter j's stored normal at the pixel it was read at
            if j in normals:
                nj = np.asarray(normals[j], t)[rj, cj]
                both = ur & usable(nj, t)
            else:
                nj = np.zeros((H, W, 3), t)
                both = np.zeros((H, W), bool)
            dot = (nr[..., 0] * nj[..., 0] + nr[..., 1] * nj[..., 1]) + nr[..., 2] * nj[..., 2]
            a = rule3 & (~both | (dot >= min_cos))
            add = a & both
            ax = np.where(add, ax + nj[..., 0], ax)
            ay = np.where(add, ay + nj[..., 1], ay)
            az = np.where(add, az + nj[..., 2], az)
            tests.append((vj & (sw > t(0.0)), d2, rel))
            dots.append((rule3 & both, dot))
            sx = np.where(a, sx + Xj[0], sx)
            sy = np.where(a, sy + Xj[1], sy)
            sz = np.where(a, sz + Xj[2], sz)
            agree += a
        la = np.sqrt((ax * ax + ay * ay) + az * az)
        summed_ok = (la > t(0.0)) & (la < t(np.inf))
        snx, sny, snz = toward_camera(ax / la, ay / la, az / la)
        has_normal = ok & np.where(ur, summed_ok, tangent_ok)
        nx, ny, nz = np.where(ur, snx, tnx), np.where(ur, sny, tny), np.where(ur, snz, tnz)
        keep = has_normal & (agree >= min_consistent)
        n = (agree + 1).astype(t)
        allrows = np.stack([sx / n, sy / n, sz / n, np.ones((H, W), t), nx, ny, nz], axis=-1)
    return {"keep": keep, "rows": allrows[keep].astype(t), "X": np.stack(Xc, -1), "w": c[3], "valid": ok, "has_normal": has_normal,
            "ref_usable": ok & ur, "tangent_ok": ok & tangent_ok, "normal": np.stack([nx, ny, nz], -1), "agree": agree, "tests": tests, "dots": dots}
