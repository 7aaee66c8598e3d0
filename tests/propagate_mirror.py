"""Restatement of the hypothesis propagation (mvs_propagate_init / mvs_propagate_run), written from the contract
and not from the kernel.  It is the arbiter: the device's z, gx, gy, cells, cost map and report must be bit-identical to State's.

The array path evaluates the hypotheses of a list of pixels at once.  Every window member of every pixel has its own depth, so the sample
is restated here in numpy float32: the fixed sampler of DESIGN.md section 2b, with each fmaf emulated exactly (the product of two float32
is exact in float64; the sum is rounded to odd with the error term of TwoSum and then to float32, which is the single rounding of the
fused operation).  tests/test_propagate_cpu.py holds that sampler against oracle.warp_by_depth on whole maps and against
oracle.sweep_sample_fx.  Rules 3-4 of section 21 are zncc_mirror.cost_of_sums, the merge of section 22 is bestk_mirror.merge.
brute_cell does one pixel's hypothesis with loops, Python integers and the oracle's single-sample entry and shares nothing with the
array path."""
import numpy as np

import bestk_mirror as km
import zncc_mirror as zm

COST_ABSDIFF, COST_ZNCC, KEEP_ALL = km.COST_ABSDIFF, km.COST_ZNCC, km.KEEP_ALL
BACKGROUND_DEPTH = np.float32(1.0)
KEPT, NEAR, FAR, RANDOM = 0, 1, 2, 3
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-5, 0), (5, 0), (0, -5), (0, 5))     # (dc, dr): near, then far
f32 = np.float32
MAGIC = f32(12582912.0)


def inside(z):
    """-1 < z < 1 (false for NaN)"""
    with np.errstate(invalid="ignore"):
        return (z > -1.0) & (z < 1.0)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays with its single rounding"""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                    # exact: 24 x 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)              # TwoSum: p + c = s + err exactly
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        above = inexact & ((err < 0) == (s > 0))     # |s| is above the exact sum's magnitude: step back to the truncated sum
        bits = np.ascontiguousarray(s).view(np.uint64) - above.astype(np.uint64)
        bits = bits | inexact.astype(np.uint64)      # rounding to odd: the sticky bit
        return bits.view(np.float64).astype(f32)


def mix(x):
    """the contract's hash on uint32 arrays (in uint64, masked)"""
    x = np.asarray(x, np.uint64) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    return x ^ (x >> np.uint64(16))


def uniform(x):
    """u = ((float)(int32)(x >> 8) - 2^23) * 2^-23, every operation exact"""
    return (((np.asarray(x, np.uint64) >> np.uint64(8)).astype(np.int32).astype(f32) - f32(8388608.0)) * (f32(1.0) / f32(8388608.0))).astype(f32)


def better(c, b):
    """rule 4 on packed cells (arrays)"""
    c, b = np.asarray(c, np.int64), np.asarray(b, np.int64)
    return ((c >> 24) != 0) & ((b == 0) | ((c & 0xffffff) * (b >> 24) < (b & 0xffffff) * (c >> 24)))


def _tied(c, b):
    c, b = np.asarray(c, np.int64), np.asarray(b, np.int64)
    return ((c >> 24) != 0) & (b != 0) & ((c & 0xffffff) * (b >> 24) == (b & 0xffffff) * (c >> 24))


def cost_map(cells):
    """(float)sum / (float)(255 k), +inf for cell 0"""
    cells = np.asarray(cells, np.uint32)
    k, s = cells >> 24, cells & np.uint32(0xffffff)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = s.astype(f32) / (np.uint32(255) * k).astype(f32)
    assert c.dtype == f32
    return np.where(cells != 0, c, f32(np.inf)).astype(f32)


class Scene:
    """the staged frames: main view, side views, and the tables the sampler reads"""

    def __init__(self, oracle, main_cam, main_img, side_cams, side_imgs):
        self.main_img = np.asarray(main_img, np.uint8)
        self.H, self.W = self.main_img.shape
        self.main_cam, self.side_cams, self.sides = main_cam, side_cams, [np.asarray(s, np.uint8) for s in side_imgs]
        self.q = [np.asarray(oracle.view_matrix(main_cam, c, self.W, self.H), f32).reshape(12) for c in side_cams]
        self.pads = [oracle.pad_image(s).astype(np.int64) for s in self.sides]
        self.lut = oracle.fx_weight_table().astype(np.int64)                       # [ky][kx][w00, w01, w10, w11]
        self.xn = np.array([oracle.lib.orc_pixel_xn(c, self.W) for c in range(self.W)], f32)
        self.yn = np.array([oracle.lib.orc_pixel_yn(r, self.H) for r in range(self.H)], f32)
        # the part of the sample that depends on the pixel alone, per view: three maps (ax, ay, aw)
        xn, yn = np.broadcast_to(self.xn[None, :], (self.H, self.W)), np.broadcast_to(self.yn[:, None], (self.H, self.W))
        self.affine = [tuple(fma32(q[4 * i], xn, fma32(q[4 * i + 1], yn, q[4 * i + 3])) for i in range(3)) for q in self.q]

    def sample(self, v, rows, cols, z):
        """rule 2: the fixed sampler's sample of view v at the pixels (rows, cols) and depths z -> (ok bool, dot int64; 0 where not ok)"""
        q, pad = self.q[v], self.pads[v]
        ax, ay, aw = (a[rows, cols] for a in self.affine[v])
        sx, sy, sw = fma32(z, q[2], ax), fma32(z, q[6], ay), fma32(z, q[10], aw)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            r256 = (f32(1.0) / sw) * f32(256.0)
            tx, ty = fma32(sx, r256, MAGIC + f32(4.0)), fma32(sy, r256, MAGIC + f32(4.0))
            lo = MAGIC + f32(132.0)
            ok = (sw > 0) & (tx > lo) & (tx < lo + f32(256.0) * f32(self.W)) & (ty > lo) & (ty < lo + f32(256.0) * f32(self.H))
            ux = np.where(ok, tx - MAGIC, 0).astype(np.int64)
            uy = np.where(ok, ty - MAGIC, 0).astype(np.int64)
        ix, iy, w = ux >> 8, uy >> 8, self.lut[(uy >> 3) & 31, (ux >> 3) & 31]
        dot = w[..., 0] * pad[iy, ix] + w[..., 1] * pad[iy, ix + 1] + w[..., 2] * pad[iy + 1, ix] + w[..., 3] * pad[iy + 1, ix + 1]
        return ok, np.where(ok, dot, 0)

    def cells(self, cost, r, keep, views, rows, cols, z, gx, gy):
        """rules 1-3: the packed cells of the hypotheses (z, gx, gy) at the pixels (rows, cols), arrays of one length"""
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
        live = inframe & inside(zq)
        qr, qc = np.clip(qr, 0, self.H - 1), np.clip(qc, 0, self.W - 1)
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
        return km.merge(per_view, keep, (len(rows),))


def seed_maps(depth, slopes=False, max_step=np.inf):
    """rule 5's copy: the start map -> (z, gx, gy)"""
    depth = np.asarray(depth, f32)
    has = inside(depth)
    z = np.where(has, depth, BACKGROUND_DEPTH).astype(f32)
    g = [np.zeros_like(z), np.zeros_like(z)]
    if slopes:
        max_step = f32(max_step)
        for axis in (1, 0):                              # gx along columns, gy along rows
            zp = np.moveaxis(z, axis, 1)
            hp = np.moveaxis(has, axis, 1)
            n = zp.shape[1]
            zm_, zq = np.full_like(zp, np.nan), np.full_like(zp, np.nan)
            zm_[:, 1:], zq[:, :n - 1] = zp[:, :n - 1], zp[:, 1:]
            with np.errstate(invalid="ignore"):
                um = inside(zm_) & (np.abs(zm_ - zp) <= max_step)
                uq = inside(zq) & (np.abs(zq - zp) <= max_step)
                both, fwd, back = (zq - zm_) * f32(0.5), zq - zp, zp - zm_
            out = np.where(um & uq, both, np.where(uq, fwd, np.where(um, back, f32(0.0))))
            out = np.where(hp, out, f32(0.0)).astype(f32)
            g[1 - axis] = np.moveaxis(out, 1, axis)
    return z, np.ascontiguousarray(g[0]), np.ascontiguousarray(g[1])


class State:
    """the stage's state after init(...) and any number of run(...)"""

    def __init__(self, scene, depth, cost, r, keep=KEEP_ALL, view_first=0, view_count=None, slopes=False, max_step=np.inf):
        self.scene, self.cost, self.r, self.keep = scene, cost, r, keep
        view_count = len(scene.sides) - view_first if view_count is None else view_count
        self.views = range(view_first, view_first + view_count)
        self.z, self.gx, self.gy = seed_maps(depth, slopes, max_step)
        rows, cols = (a.reshape(-1) for a in np.indices(self.z.shape))
        self.cells = self._eval(rows, cols, self.z.reshape(-1), self.gx.reshape(-1), self.gy.reshape(-1)).reshape(self.z.shape)
        self.t = 0
        self.counters = [0, 0, 0, 0]
        self.wins = []                                   # per half: (t, h, rows, cols, class) of the active pixels, for the tests
        self.ties = 0                                    # candidates whose mean cost equalled the held one's: kept out by the strict rule
        self.no_random = 0                               # random candidates not taken because the pixel had no hypothesis

    def _eval(self, rows, cols, z, gx, gy):
        """cells of the candidates; a candidate whose centre is not live has cell 0"""
        out = np.zeros(len(rows), np.uint32)
        go = inside(z)
        if go.any():
            out[go] = self.scene.cells(self.cost, self.r, self.keep, self.views, rows[go], cols[go], z[go], gx[go], gy[go])
        return out

    def copy_maps(self):
        return self.z.copy(), self.gx.copy(), self.gy.copy(), self.cells.copy()

    def cost_map(self):
        return cost_map(self.cells)

    def report(self):
        return self.counters + [int((self.cells != 0).sum())]

    def run(self, iterations, dz, dg, nrandom=2, seed=0):
        assert iterations >= 1 and 0 <= nrandom <= 4
        H, W = self.z.shape
        for _ in range(iterations):
            dz_t, dg_t = f32(dz), f32(dg)
            for _ in range(self.t):
                dz_t, dg_t = dz_t * f32(0.5), dg_t * f32(0.5)
            for h in (0, 1):
                rows, cols = np.nonzero((np.add.outer(np.arange(H), np.arange(W)) + h) % 2 == 0)
                z, gx, gy, cell = self.z[rows, cols], self.gx[rows, cols], self.gy[rows, cols], self.cells[rows, cols]
                cls = np.zeros(len(rows), np.int64)
                for i, (dc, dr) in enumerate(OFFSETS):
                    nr, nc = rows + dr, cols + dc
                    inframe = (nr >= 0) & (nr < H) & (nc >= 0) & (nc < W)
                    nr, nc = np.clip(nr, 0, H - 1), np.clip(nc, 0, W - 1)
                    zn, cgx, cgy = self.z[nr, nc], self.gx[nr, nc], self.gy[nr, nc]
                    have = inframe & inside(zn)
                    cz = ((zn - cgx * f32(dc)) - cgy * f32(dr)).astype(f32)
                    cz = np.where(have, cz, f32(np.nan))
                    cc = self._eval(rows, cols, cz, cgx, cgy)
                    win = better(cc, cell)
                    self.ties += int(_tied(cc, cell).sum())
                    z, gx, gy, cell = np.where(win, cz, z), np.where(win, cgx, gx), np.where(win, cgy, gy), np.where(win, cc, cell)
                    cls[win] = NEAR if i < 4 else FAR
                base = mix(mix((int(seed) + 2 * self.t + h) & 0xffffffff) ^ (rows * W + cols).astype(np.uint64))
                for j in range(nrandom):
                    u = [uniform(mix(base ^ np.uint64(4 * j + c))) for c in range(3)]
                    have = inside(z)
                    self.no_random += int((~have).sum())
                    cz = np.where(have, z + dz_t * u[0], f32(np.nan)).astype(f32)
                    cgx, cgy = (gx + dg_t * u[1]).astype(f32), (gy + dg_t * u[2]).astype(f32)
                    cc = self._eval(rows, cols, cz, cgx, cgy)
                    win = better(cc, cell)
                    z, gx, gy, cell = np.where(win, cz, z), np.where(win, cgx, gx), np.where(win, cgy, gy), np.where(win, cc, cell)
                    cls[win] = RANDOM
                self.z[rows, cols], self.gx[rows, cols], self.gy[rows, cols], self.cells[rows, cols] = z, gx, gy, cell
                for k in range(4):
                    self.counters[k] += int((cls == k).sum())
                self.wins.append((self.t, h, rows, cols, cls))
            self.t += 1
        return self


def brute_cell(oracle, cost, main_cam, main_img, side_cams, side_imgs, z, gx, gy, r, keep, row, col, views=None):
    """the cell of hypothesis (z, gx, gy) at (row, col) with loops and scalars -> (per view (members, counted, c), the packed cell)"""
    main_img = np.asarray(main_img, np.uint8)
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
            _, counted, c = zm.brute_cell(main_img, B, ok, r, row, col)
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
