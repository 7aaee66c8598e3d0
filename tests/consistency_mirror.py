"""Restatement of the propagation's geometric term (mvs_propagate_set_consistency), written from the contract and
not from the kernel.  It is the arbiter: the device's z, gx, gy, cells, cost map, report and support map must be bit-identical.

Term holds what init takes: the main camera's matrices (M, M^-1), per listed neighbour (P_j, P_j^-1, the slot's depth map), the weight
and the cap.  Term.evaluate does rules 2-6 on arrays of pixels in numpy float32 -- one rounding per operation, `/` and sqrt correctly
rounded, fusion's order of operations through fuse_mirror._unproject / _prow, the pixel centres through fuse_mirror.pixel_xn / pixel_yn
-- and says per (pixel, neighbour) which clause of rule 5 failed.  State is propagate_mirror.State with rule 7 behind the photometric
cell in _eval and rule 8's support map; it takes propagate_mirror.Scene and gated_mirror.Scene alike.  brute_term does one pixel with
scalar loops and shares nothing with the array path but numpy's float32.

With the matrices mvs_depth_slot_matrices returns (and the main camera's made the same way) everything is expected bit for bit."""
import numpy as np

import fuse_mirror as fm
import propagate_mirror as pm

f32 = np.float32
MAX_SLOTS = 8
MAX_PENALTY = 1000000                 # rule 7: floorf(max_px * w255) may not exceed it
# the clauses of rule 5 in the order they are tested; ANSWERS: none failed
ANSWERS, BEHIND, OUTSIDE, INVALID, BACK_BEHIND, FAR = range(6)
CLAUSES = ("answers", "q_w <= 0", "outside the frame", "z_j not valid", "s_w <= 0", "e > max_px")


def w255(weight):
    """rule 6's one product"""
    return f32(weight) * f32(255.0)


def admitted(weight, max_px):
    """what mvs_propagate_set_consistency admits of (weight, max_px)"""
    weight, max_px = f32(weight), f32(max_px)
    if not (np.isfinite(weight) and weight >= 0 and np.isfinite(max_px) and max_px > 0):
        return False
    return bool(np.floor(max_px * w255(weight)) <= f32(MAX_PENALTY))


class Term:
    """what init takes: main = (M, M^-1), neighbours = [(P_j, P_j^-1, depth map [H, W] float32)] in the listed order (a slot listed twice
    is there twice), weight, max_px"""

    def __init__(self, main, neighbours, weight, max_px):
        assert len(neighbours) <= MAX_SLOTS and admitted(weight, max_px)
        self.M, self.Mi = (np.asarray(m, f32).reshape(4, 4) for m in main[:2])
        self.neighbours = [(np.asarray(P, f32).reshape(4, 4), np.asarray(Pi, f32).reshape(4, 4), np.asarray(d, f32)) for P, Pi, d in
                           ((n[0], n[1], n[-1]) for n in neighbours)]
        self.weight, self.max_px = f32(weight), f32(max_px)
        self.w255 = w255(weight)

    def evaluate(self, rows, cols, z, H, W):
        """rules 2-6 for the hypothesis depths z at the pixels (rows, cols) -> (g uint32, answers int64, clause [n, neighbours] int64,
        e [n, neighbours] float32: the error where rule 4 gets that far, whether or not it is within the cap)"""
        rows, cols, z = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(z, f32)
        n, K = len(rows), len(self.neighbours)
        clause, err = np.zeros((n, K), np.int64), np.full((n, K), np.nan, f32)
        total = np.zeros(n, np.int64)
        halfW, halfH = f32(W) * f32(0.5), f32(H) * f32(0.5)
        with np.errstate(all="ignore"):
            X = fm._unproject(self.Mi, fm.pixel_xn(cols, W), fm.pixel_yn(rows, H), z)
            for j, (P, Pi, depth) in enumerate(self.neighbours):
                qw = fm._prow(P, 3, X)
                a, b = fm._prow(P, 0, X) / qw, fm._prow(P, 1, X) / qw
                u = (a + f32(1.0)) * halfW - f32(0.5)
                v = (f32(1.0) - b) * halfH - f32(0.5)
                fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
                front = qw > f32(0.0)
                inframe = (fc >= f32(0.0)) & (fc < f32(W)) & (fr >= f32(0.0)) & (fr < f32(H))
                at = front & inframe
                zj = depth[np.where(at, fr, 0).astype(np.int64), np.where(at, fc, 0).astype(np.int64)]
                valid = pm.inside(zj)
                Xj = fm._unproject(Pi, a, b, zj)
                sw = fm._prow(self.M, 3, Xj)
                ur = (fm._prow(self.M, 0, Xj) / sw + f32(1.0)) * halfW - f32(0.5)
                vr = (f32(1.0) - fm._prow(self.M, 1, Xj) / sw) * halfH - f32(0.5)
                du, dv = ur - cols.astype(f32), vr - rows.astype(f32)
                e = np.sqrt(du * du + dv * dv)
                assert all(x.dtype == f32 for x in (qw, a, u, fc, zj, sw, ur, du, e))
                near = e <= self.max_px
                clause[:, j] = np.where(~front, BEHIND, np.where(~inframe, OUTSIDE, np.where(~valid, INVALID, np.where(~(sw > f32(0.0)), BACK_BEHIND,
                                                                                                                   np.where(~near, FAR, ANSWERS)))))
                err[:, j] = np.where(at & valid & (sw > f32(0.0)), e, f32(np.nan))
                ej = np.where(clause[:, j] == ANSWERS, e, self.max_px).astype(f32)
                gj = np.floor(ej * self.w255)
                assert gj.dtype == f32 and (gj >= 0).all() and (gj <= MAX_PENALTY).all()
                total += gj.astype(np.int64)
        g = (total // max(K, 1)).astype(np.uint32)
        return g, (clause == ANSWERS).sum(1), clause, err


class State(pm.State):
    """propagate_mirror.State with the term: rule 7 in _eval, rule 8 in support().  term None or without neighbours: the term is off"""

    def __init__(self, scene, depth, cost, r, keep=pm.KEEP_ALL, view_first=0, view_count=None, slopes=False, max_step=np.inf, term=None):
        self.term = term if term is not None and len(term.neighbours) else None
        super().__init__(scene, depth, cost, r, keep, view_first, view_count, slopes, max_step)

    def _eval(self, rows, cols, z, gx, gy):
        c = super()._eval(rows, cols, z, gx, gy)
        if self.term is None:
            return c
        k = (c >> np.uint32(24)).astype(np.int64)
        go = k != 0
        out = np.zeros_like(c)
        if go.any():
            g = self.term.evaluate(rows[go], cols[go], z[go], self.scene.H, self.scene.W)[0].astype(np.int64)
            s = (c[go] & np.uint32(0xffffff)).astype(np.int64) + k[go] * g
            assert (s < 1 << 24).all(), "rule 7's bound"
            out[go] = ((k[go] << 24) | s).astype(np.uint32)
        return out

    def support(self):
        """rule 8: the listed neighbours that answer for the hypothesis each pixel holds; 0 without one and without a term"""
        out = np.zeros(self.z.shape, np.uint8)
        if self.term is None:
            return out
        rows, cols = np.nonzero(pm.inside(self.z))
        out[rows, cols] = self.term.evaluate(rows, cols, self.z[rows, cols], *self.z.shape)[1]
        return out


def brute_term(main, neighbours, weight, max_px, W, H, row, col, cz):
    """rules 2-6 for the one hypothesis depth cz at (row, col) with scalar loops -> (g, the number of neighbours that answer, per neighbour
    the clause of rule 5 that failed (ANSWERS: none) and e_j)"""
    def dot4(m, i, x):                                            # ((m0 x0 + m1 x1) + m2 x2) + m3, the last coordinate 1
        return ((m[i][0] * x[0] + m[i][1] * x[1]) + m[i][2] * x[2]) + m[i][3]

    def lift(mi, x, y, z):
        h = [dot4(mi, i, (x, y, z)) for i in range(4)]
        return h[0] / h[3], h[1] / h[3], h[2] / h[3]

    def pixel(a, b):
        return (a + f32(1.0)) * (f32(W) * f32(0.5)) - f32(0.5), (f32(1.0) - b) * (f32(H) * f32(0.5)) - f32(0.5)

    M, Mi = ([[f32(x) for x in r] for r in np.asarray(m, f32).reshape(4, 4)] for m in main[:2])
    max_px, scale = f32(max_px), f32(weight) * f32(255.0)
    xn = f32(float(2 * col + 1) * float(f32(1.0) / f32(W)) - 1.0)          # fmaf((float)(2 c + 1), 1 / W, -1): exact in double, rounded once
    yn = f32(-float(2 * row + 1) * float(f32(1.0) / f32(H)) + 1.0)
    total, answers, detail = 0, 0, []
    with np.errstate(all="ignore"):
        X = lift(Mi, xn, yn, f32(cz))
        for n in neighbours:
            P, Pi = ([[f32(x) for x in r] for r in np.asarray(m, f32).reshape(4, 4)] for m in n[:2])
            depth = n[-1]
            clause, e = ANSWERS, max_px
            qw = dot4(P, 3, X)
            a, b = dot4(P, 0, X) / qw, dot4(P, 1, X) / qw
            u, v = pixel(a, b)
            fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
            if not qw > 0:
                clause = BEHIND
            elif not (0 <= fc < W and 0 <= fr < H):
                clause = OUTSIDE
            else:
                zj = f32(depth[int(fr), int(fc)])
                if not -1.0 < float(zj) < 1.0:
                    clause = INVALID
                else:
                    Xj = lift(Pi, a, b, zj)
                    sw = dot4(M, 3, Xj)
                    ur, vr = pixel(dot4(M, 0, Xj) / sw, dot4(M, 1, Xj) / sw)
                    du, dv = ur - f32(col), vr - f32(row)
                    d = np.sqrt(du * du + dv * dv)
                    assert all(type(t) is f32 for t in (qw, a, u, sw, ur, du, d))
                    if not sw > 0:
                        clause = BACK_BEHIND
                    elif not d <= max_px:
                        clause = FAR
                    else:
                        e = d
            if clause == ANSWERS:
                answers += 1
            total += int(np.floor(e * scale))
            detail.append((clause, e))
    return total // len(neighbours), answers, detail
