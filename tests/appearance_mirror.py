"""numpy restatement of the TSDF volume's appearance (csrc/tsdf.hip: mvs_tsdf_integrate_frames; csrc/appearance.hip: mvs_tsdf_shade,
mvs_tsdf_sample_appearance; the contract: DESIGN.md section 15 rules A-F, include/mvs.h).

The votes are integers; the reads are float32 with one rounding per operation, as the kernels compute them without contraction; `/` is
correctly rounded on both sides.  The volume is tsdf_mirror.Volume with one more field, the w-maps are tsdf_mirror.wmap's, the pixel centres,
the back-projection and the projection rows are fuse_mirror's, the cell and its fractions raycast_mirror's.  With the matrices
mvs_depth_slot_matrices returns everything is expected bit for bit.

  Volume.integrate_frames(maps, mats, frames, pairs)   rule B: Volume.integrate's rules 2-4 and the votes, for (depth slot, frame slot) pairs
  appearance(vol, X)                                   rule C at points X [N, 3] -> (have [N] bool, value [N] f32)
  shade(vol, mats, depth)                              rule D -> [H, W, 2] u8
  sample(vol, points4)                                 rule E -> [N] f32, NaN = none
`cells` is [G, G, G] uint32, count << 24 | sum, indexed [k][j][i] like mvs_tsdf_appearance_fetch's download; None = no appearance.
"""
import numpy as np

import fuse_mirror as fm
import raycast_mirror as rm
import tsdf_mirror as tm

f32 = np.float32
u32 = np.uint32
FULL = u32(0xFF000000)   # a cell at count 255 takes no more votes
VOTE = u32(0x01000000)


class Volume(tm.Volume):
    """tsdf_mirror.Volume and the appearance cells (rule A)"""

    def __init__(self, G, origin, h, truncation):
        super().__init__(G, origin, h, truncation)
        self.cells = None

    def integrate_frames(self, maps, mats, frames, pairs):
        """rule B for the listed (depth slot, frame slot) pairs in list order; maps: depth slot -> w-map [H, W] (tsdf_mirror.wmap),
        mats: depth slot -> (P, P^-1, centre), frames: frame slot -> [H, W] u8"""
        if self.cells is None:
            self.cells = np.zeros((self.G,) * 3, u32)
        x = self.x[None, None, :]
        y = self.y[None, :, None]
        z = self.z[:, None, None]
        for s, fs in pairs:
            wm = maps[s]
            I = np.asarray(frames[fs], np.uint8)
            H, W = wm.shape
            P = np.asarray(mats[s][0], f32)
            halfW, halfH = f32(W) * f32(0.5), f32(H) * f32(0.5)
            with np.errstate(all="ignore"):
                # section 12 rules 2-4, as tsdf_mirror.Volume.integrate states them
                q = [P[r, 0] * x + ((P[r, 1] * y + P[r, 2] * z) + P[r, 3]) for r in (0, 1, 3)]
                qx, qy, qw = (np.broadcast_to(a, (self.G,) * 3).astype(f32) for a in q)
                inv = f32(1.0) / qw
                u = (qx * inv + f32(1.0)) * halfW - f32(0.5)
                v = (f32(1.0) - qy * inv) * halfH - f32(0.5)
                fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
                hit = (qw > f32(0.0)) & (fc >= f32(0.0)) & (fc < f32(W)) & (fr >= f32(0.0)) & (fr < f32(H))
                r, c = fr[hit].astype(np.int64), fc[hit].astype(np.int64)
                wd = np.full(qw.shape, np.nan, f32)
                wd[hit] = wm[r, c]
                t = (wd - qw) * self.inv_tau
                upd = (wd == wd) & (t >= f32(-1.0))
                # the vote: the intensity of the very pixel the w-map was read at, into the unclamped band, unless the cell is full
                inten = np.zeros(qw.shape, u32)
                inten[hit] = I[r, c]
                vote = upd & (t < f32(1.0)) & (self.cells < FULL)
            self.sum = np.where(upd, self.sum + np.minimum(t, f32(1.0)), self.sum).astype(f32)
            self.count = self.count + upd.astype(np.int32)
            self.cells = np.where(vote, self.cells + (VOTE + inten), self.cells).astype(u32)
        return self


def split(cells):
    """(count [..] , sum [..]) of packed cells"""
    cells = np.asarray(cells, u32)
    return (cells >> u32(24)).astype(np.int64), (cells & u32(0xFFFFFF)).astype(np.int64)


def appearance(vol, X):
    """rule C at X = [x [N], y [N], z [N]] (f32) -> (have [N], value [N] f32; 0 where there is none)"""
    G = vol.G
    inv_h = f32(1.0) / vol.h
    top = f32(G - 1)
    with np.errstate(all="ignore"):
        g = [((np.asarray(X[a], f32) - vol.origin[a]) * inv_h).astype(f32) for a in range(3)]
        inside = np.ones(g[0].shape, bool)
        for a in range(3):
            inside &= (g[a] >= f32(0.0)) & (g[a] <= top)
        cells = [rm._cell_axis(g[a], G) for a in range(3)]
        (ix, fx), (iy, fy), (iz, fz) = cells
        num = np.zeros(g[0].shape, f32)
        den = np.zeros(g[0].shape, f32)
        for d in range(8):
            di, dj, dk = d & 1, (d >> 1) & 1, d >> 2
            wx = fx if di else f32(1.0) - fx
            wy = fy if dj else f32(1.0) - fy
            wz = fz if dk else f32(1.0) - fz
            w = ((wx * wy) * wz).astype(f32)
            n, s = split(vol.cells[iz + dk, iy + dj, ix + di])
            present = n > 0
            a_d = (s.astype(f32) / n.astype(f32)).astype(f32)
            num = np.where(present, num + w * a_d, num).astype(f32)
            den = np.where(present, den + w, den).astype(f32)
        have = inside & (den > f32(0.0))
        value = np.where(have, num / den, f32(0.0)).astype(f32)
    return have, value


def shade(vol, mats, depth):
    """rule D: mvs_tsdf_shade of the depth map `depth` [H, W] f32 of the camera with slot matrices mats -> [H, W, 2] u8"""
    P, Pi = (np.asarray(m, f32) for m in mats[:2])
    z = np.asarray(depth, f32)
    H, W = z.shape
    rows, cols = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        ok = fm._valid(z, None, np.inf, f32)
        X = fm._unproject(Pi, fm.pixel_xn(cols, W), fm.pixel_yn(rows, H), z)
        ok &= fm._prow(P, 3, X) > f32(0.0)
        have, value = appearance(vol, X)
        ok &= have
        grey = np.minimum(np.floor(value + f32(0.5)), f32(255.0))
    out = np.zeros((H, W, 2), np.uint8)
    out[..., 0] = np.where(ok, grey, 0).astype(np.uint8)
    out[..., 1] = np.where(ok, 255, 0).astype(np.uint8)
    return out


def sample(vol, points4):
    """rule E: mvs_tsdf_sample_appearance of rows (x, y, z, w) -> [N] f32, NaN where there is none"""
    p = np.asarray(points4, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        X = [(p[:, a] / p[:, 3]).astype(f32) for a in range(3)]
        have, value = appearance(vol, X)
    return np.where(have, value, f32(np.nan)).astype(f32)
