"""Restatement of the guide-gated windows (mvs_sweep_run_bestk_gated, mvs_propagate_set_gate), written from the
contract and not from the kernels.  It is the arbiter: the device's cells must be bit-identical.

The sweep.  q is a member of M(p) iff it is inside the frame within the window, ok(q), and |G(q) - G(p)| <= tau.  The gate depends on
neither plane nor view: gates() holds it as (2 r + 1)^2 boolean maps, one per window offset, and gated_sums() adds (2 r + 1)^2 shifted
slices of each field on int64 under it.  The raw samples come from the oracle (zncc_mirror.warped for the ZNCC cost; the one-view packed
cell ok << 24 | e of the oracle's fixed-sampler sweep for the absolute difference), the sums feed zncc_mirror.cost_of_sums or section 22's
integer mean, the views are merged by bestk_mirror.merge.  brute_cell does one cell with loops and Python integers, the absolute
difference's samples through the oracle's single-sample entry, and shares nothing with the array path.

The propagation.  Scene is propagate_mirror.Scene with one added clause in cells(): live &= |a - a_centre| <= tau on the guide.
propagate_mirror.State takes it unchanged.  brute_prop_cell is propagate_mirror.brute_cell's loop with the same clause."""
import numpy as np

import bestk_mirror as bm
import propagate_mirror as pm
import zncc_mirror as zm

COST_ABSDIFF, COST_ZNCC, KEEP_ALL = bm.COST_ABSDIFF, bm.COST_ZNCC, bm.KEEP_ALL
f32 = np.float32


def gates(guide, tau, r):
    """-> [(2 r + 1)^2, H, W] bool: entry (dy + r) (2 r + 1) + (dx + r) at p says that q = p + (dy, dx) is inside the frame and
    |G(q) - G(p)| <= tau"""
    assert 1 <= r <= 4 and 0 <= tau <= 255
    g = np.asarray(guide).astype(np.int64)
    H, W = g.shape
    pad = np.full((H + 2 * r, W + 2 * r), 1 << 20, np.int64)       # outside the frame: no grey level is within tau of it
    pad[r:r + H, r:r + W] = g
    return np.stack([np.abs(pad[dy:dy + H, dx:dx + W] - g) <= tau for dy in range(2 * r + 1) for dx in range(2 * r + 1)])


def gated_sums(fields, gate, r):
    """fields: [..., H, W] int64 arrays (0 where the sample is not ok) -> for each the sum over the gated window of every pixel"""
    H, W = gate.shape[1:]
    out = []
    for x in fields:
        x = np.asarray(x, np.int64)
        pad = np.zeros(x.shape[:-2] + (H + 2 * r, W + 2 * r), np.int64)
        pad[..., r:r + H, r:r + W] = x
        s = np.zeros(x.shape, np.int64)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                s += np.where(gate[dy * (2 * r + 1) + dx], pad[..., dy:dy + H, dx:dx + W], 0)
        out.append(s)
    return out


def raw_view(oracle, cost, main_cam, main_img, side_cam, frame, D, z_lo, z_hi):
    """the samples of one view over the D planes of [z_lo, z_hi], before any window -> (ok [D, H, W] bool, x [D, H, W] int64): x is the
    warped grey level B for the ZNCC cost and e = |dot - 255 A| for the absolute difference, 0 where not ok"""
    if cost == COST_ZNCC:
        z = oracle.plane_table(D, z_lo, z_hi)
        assert not (z == f32(1.0)).any()
        parts = [zm.warped(oracle, main_cam, side_cam, frame, zd) for zd in z]
        ok = np.stack([p[1] for p in parts])
        return ok, np.where(ok, np.stack([p[0] for p in parts]).astype(np.int64), 0)
    assert cost == COST_ABSDIFF
    one = oracle.sweep(main_cam, main_img, np.asarray(side_cam, f32)[None], [frame], D, z_lo, z_hi, want_volume=True, sampler="fixed")[3]
    ok, e = (one >> 24).astype(np.int64), (one & 0xffffff).astype(np.int64)
    assert ok.max(initial=0) <= 1 and (e[ok == 0] == 0).all() and e.max(initial=0) <= 65025
    return ok != 0, e


def view_costs(cost, main_img, raw, gate, r):
    """rule 1 over the gated members: raw = raw_view(...) -> (counted, c), [D, H, W] each"""
    ok, x = raw
    m = ok.astype(np.int64)
    if cost == COST_ZNCC:
        A = np.asarray(main_img).astype(np.int64)[None]
        N, Sa, Sb, Sab, Saa, Sbb = gated_sums([m, m * A, x, x * A, m * A * A, x * x], gate, r)
        return zm.cost_of_sums(N, Sa, Sb, Sab, Saa, Sbb, ok)
    N, S = gated_sums([m, x], gate, r)
    assert S.max(initial=0) < 2 ** 23
    return ok, np.where(ok, S // np.maximum(N, 1), 0).astype(np.uint32)


def volume(oracle, cost, main_cam, main_img, side_cams, side_imgs, D, z_lo, z_hi, r, keep, tau, guide=None, views=None):
    """the packed volume [D, H, W] uint32 of mvs_sweep_run_bestk_gated over the side views `views` (default: all)"""
    views = range(len(side_imgs)) if views is None else views
    gate = gates(main_img if guide is None else guide, tau, r)
    per_view = [view_costs(cost, main_img, raw_view(oracle, cost, main_cam, main_img, side_cams[v], side_imgs[v], D, z_lo, z_hi), gate, r) for v in views]
    return bm.merge(per_view, keep, (D,) + np.asarray(main_img).shape)


def brute_cell(oracle, cost, main_cam, main_img, side_cams, side_imgs, z, r, keep, tau, guide, row, col, views=None):
    """the cell of plane depth z at (row, col) with loops and Python integers -> (per view (members, counted, c), the packed cell)"""
    main_img = np.asarray(main_img, np.uint8)
    guide = main_img if guide is None else np.asarray(guide, np.uint8)
    H, W = main_img.shape
    views = range(len(side_imgs)) if views is None else views
    per_view, costs = [], []
    for v in views:
        if cost == COST_ZNCC:
            B, okmap = zm.warped(oracle, main_cam, side_cams[v], side_imgs[v], z)
        else:
            q = oracle.view_matrix(main_cam, side_cams[v], W, H)
            pad = oracle.pad_image(np.asarray(side_imgs[v], np.uint8))
        a, b, e, centre = [], [], [], False
        for y in range(row - r, row + r + 1):
            for x in range(col - r, col + r + 1):
                if not (0 <= y < H and 0 <= x < W):
                    continue
                if abs(int(guide[y, x]) - int(guide[row, col])) > tau:
                    continue
                if cost == COST_ZNCC:
                    if not okmap[y, x]:
                        continue
                    a.append(int(main_img[y, x]))
                    b.append(int(B[y, x]))
                else:
                    good, dot = oracle.sweep_sample_fx(q, oracle.lib.orc_pixel_xn(x, W), oracle.lib.orc_pixel_yn(y, H), float(z), pad)
                    if not good:
                        continue
                    e.append(abs(int(dot) - 255 * int(main_img[y, x])))
                centre = centre or (y, x) == (row, col)
        if cost == COST_ZNCC:
            N, Sa, Sb = len(a), sum(a), sum(b)
            Sab, Saa, Sbb = sum(s * t for s, t in zip(a, b)), sum(s * s for s in a), sum(t * t for t in b)
            cov, va, vb = N * Sab - Sa * Sb, N * Saa - Sa * Sa, N * Sbb - Sb * Sb          # Python integers
            counted, c = bool(centre and va > 0 and vb > 0), 0
            if counted:
                den = np.sqrt(f32(va) * f32(vb))
                ncc = min(max(f32(cov) / den, f32(-1.0)), f32(1.0))
                c = np.floor(f32(32512.0) * (f32(1.0) - ncc))
                assert all(type(t) is f32 for t in (den, ncc, c))
            per_view.append((N, counted, int(c)))
        else:
            counted = bool(centre)
            per_view.append((len(e), counted, sum(e) // len(e) if counted else 0))
        if counted:
            costs.append(per_view[-1][2])
    best = sorted(costs)
    if keep != KEEP_ALL:
        best = best[:keep]
    return per_view, (len(best) << 24) | sum(best)


class Scene(pm.Scene):
    """propagate_mirror.Scene with the gate of mvs_propagate_set_gate: (tau, guide), the guide the main image when None"""

    def __init__(self, oracle, main_cam, main_img, side_cams, side_imgs, tau=255, guide=None):
        super().__init__(oracle, main_cam, main_img, side_cams, side_imgs)
        assert 0 <= tau <= 255
        self.tau = int(tau)
        self.guide = self.main_img if guide is None else np.asarray(guide, np.uint8)
        assert self.guide.shape == self.main_img.shape

    def cells(self, cost, r, keep, views, rows, cols, z, gx, gy):
        """rules 1-3 of section 25 with rule 1's added clause: member q is live iff it is live there and |G(q) - G(p)| <= tau"""
        assert (cost == COST_ZNCC and 1 <= r <= 4) or (cost == COST_ABSDIFF and 0 <= r <= 4)
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        z, gx, gy = (np.asarray(a, f32)[:, None] for a in (z, gx, gy))
        if len(rows) == 0:
            return np.zeros(0, np.uint32)
        dr, dc = (a.reshape(-1) for a in np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij"))
        centre = len(dr) // 2
        qr, qc = rows[:, None] + dr[None], cols[:, None] + dc[None]
        inframe = (qr >= 0) & (qr < self.H) & (qc >= 0) & (qc < self.W)
        with np.errstate(invalid="ignore", over="ignore"):
            zq = (z + gx * dc[None].astype(f32)) + gy * dr[None].astype(f32)       # rule 1, one rounding per operation
        assert zq.dtype == f32
        live = inframe & pm.inside(zq)
        qr, qc = np.clip(qr, 0, self.H - 1), np.clip(qc, 0, self.W - 1)
        g = self.guide[qr, qc].astype(np.int64)
        live &= np.abs(g - g[:, centre:centre + 1]) <= self.tau                     # the gate
        a = self.main_img[qr, qc].astype(np.int64)
        per_view = []
        for v in views:
            ok, dot = self.sample(v, qr, qc, np.where(live, zq, f32(0.0)))
            ok = ok & live
            m = ok.astype(np.int64)
            if cost == COST_ZNCC:
                b = m * ((dot + 127) // 255)
                am = m * a
                per_view.append(zm.cost_of_sums(m.sum(1), am.sum(1), b.sum(1), (am * b).sum(1), (am * a).sum(1), (b * b).sum(1), ok[:, centre]))
            else:
                N, S = m.sum(1), (m * np.abs(dot - 255 * a)).sum(1)
                assert S.max(initial=0) < 2 ** 23
                per_view.append((ok[:, centre], np.where(ok[:, centre], S // np.maximum(N, 1), 0).astype(np.uint32)))
        return bm.merge(per_view, keep, (len(rows),))


def brute_prop_cell(oracle, cost, main_cam, main_img, side_cams, side_imgs, z, gx, gy, r, keep, tau, guide, row, col, views=None):
    """the cell of hypothesis (z, gx, gy) at (row, col) under the gate, with loops and scalars -> (per view (members, counted, c), the cell)"""
    main_img = np.asarray(main_img, np.uint8)
    guide = main_img if guide is None else np.asarray(guide, np.uint8)
    H, W = main_img.shape
    views = range(len(side_imgs)) if views is None else views
    z, gx, gy = f32(z), f32(gx), f32(gy)
    per_view, costs = [], []
    for v in views:
        q = oracle.view_matrix(main_cam, side_cams[v], W, H)
        pad = oracle.pad_image(np.asarray(side_imgs[v], np.uint8))
        dots = {}
        for y in range(row - r, row + r + 1):
            for x in range(col - r, col + r + 1):
                if not (0 <= y < H and 0 <= x < W):
                    continue
                if abs(int(guide[y, x]) - int(guide[row, col])) > tau:
                    continue
                zq = (z + gx * f32(x - col)) + gy * f32(y - row)
                assert type(zq) is f32
                if not -1.0 < float(zq) < 1.0:
                    continue
                good, dot = oracle.sweep_sample_fx(q, oracle.lib.orc_pixel_xn(x, W), oracle.lib.orc_pixel_yn(y, H), float(zq), pad)
                if good:
                    dots[y, x] = int(dot)
        if cost == COST_ZNCC:
            B, ok = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
            for (y, x), d in dots.items():
                B[y, x], ok[y, x] = (d + 127) // 255, True
            _, counted, c = zm.brute_cell(main_img, B, ok, r, row, col)          # (its members are the ok pixels: the gated ones)
        else:
            counted = (row, col) in dots
            c = sum(abs(d - 255 * int(main_img[p])) for p, d in dots.items()) // len(dots) if counted else 0
        per_view.append((len(dots), bool(counted), int(c)))
        if counted:
            costs.append(int(c))
    best = sorted(costs)
    if keep != KEEP_ALL:
        best = best[:keep]
    return per_view, (len(best) << 24) | sum(best)
