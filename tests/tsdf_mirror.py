"""numpy restatement of mvs_tsdf_integrate and mvs_tsdf_surface (csrc/tsdf.hip; the contract: DESIGN.md section 12, include/mvs.h).

Everything is float32 with one rounding per operation, as the kernels compute it without contraction (-ffp-contract=off); `/` is correctly
rounded on both sides.  The w-map reads a stored map exactly as mvs_fuse_depth does, so it is built from tests/fuse_mirror.py's helpers
(validity, the sweep's pixel centres, the back-projection through P^-1, the projection's w row).  With the matrices that
mvs_depth_slot_matrices returns the fields are expected bit for bit.

The volume is (sum [G, G, G] f32, count [G, G, G] i32), indexed [k][j][i] like mvs_tsdf_fetch's download.
"""
import os
import sys

import numpy as np

import fuse_mirror as fm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import meshing_oracle as mo  # noqa: E402

f32 = np.float32


def wmap(depth, cost, mats, max_cost=np.inf):
    """contract step 1: linear depth w of every valid pixel whose back-projection lies in front of the camera, NaN elsewhere"""
    P, Pi = (np.asarray(m, f32) for m in mats[:2])
    z = np.asarray(depth, f32)
    H, W = z.shape
    rows, cols = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        ok = fm._valid(z, None if max_cost == np.inf else np.asarray(cost, f32), max_cost, f32)
        X = fm._unproject(Pi, fm.pixel_xn(cols, W), fm.pixel_yn(rows, H), z)
        w = fm._prow(P, 3, X)
    return np.where(ok & (w > f32(0.0)), w, f32(np.nan)).astype(f32)


class Volume:
    """mvs_tsdf_volume's state: G^3 nodes at origin + h (i, j, k), a zeroed (sum, count) pair"""

    def __init__(self, G, origin, h, truncation):
        self.G = int(G)
        self.origin = np.asarray(origin, f32).reshape(3)
        self.h = f32(h)
        self.inv_tau = f32(1.0) / f32(truncation)
        self.sum = np.zeros((G, G, G), f32)
        self.count = np.zeros((G, G, G), np.int32)
        idx = np.arange(self.G).astype(f32)
        self.x = (self.origin[0] + self.h * idx).astype(f32)   # node coordinates: a product, then a sum
        self.y = (self.origin[1] + self.h * idx).astype(f32)
        self.z = (self.origin[2] + self.h * idx).astype(f32)

    def integrate(self, maps, mats, slots):
        """contract steps 2-4 for the listed slots in list order; maps: slot -> w-map [H, W], mats: slot -> (P, P^-1, centre)"""
        x = self.x[None, None, :]
        y = self.y[None, :, None]
        z = self.z[:, None, None]
        for s in slots:
            wm = maps[s]
            H, W = wm.shape
            P = np.asarray(mats[s][0], f32)
            halfW, halfH = f32(W) * f32(0.5), f32(H) * f32(0.5)
            with np.errstate(all="ignore"):
                q = [P[r, 0] * x + ((P[r, 1] * y + P[r, 2] * z) + P[r, 3]) for r in (0, 1, 3)]
                qx, qy, qw = (np.broadcast_to(a, (self.G,) * 3).astype(f32) for a in q)
                inv = f32(1.0) / qw
                u = (qx * inv + f32(1.0)) * halfW - f32(0.5)
                v = (f32(1.0) - qy * inv) * halfH - f32(0.5)
                fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
                hit = (qw > f32(0.0)) & (fc >= f32(0.0)) & (fc < f32(W)) & (fr >= f32(0.0)) & (fr < f32(H))
                wd = np.full(qw.shape, np.nan, f32)
                wd[hit] = wm[fr[hit].astype(np.int64), fc[hit].astype(np.int64)]
                t = (wd - qw) * self.inv_tau
                upd = (wd == wd) & (t >= f32(-1.0))
            self.sum = np.where(upd, self.sum + np.minimum(t, f32(1.0)), self.sum).astype(f32)
            self.count = self.count + upd.astype(np.int32)
        return self

    def field(self, min_observations=1):
        """contract step 5: (F, node mask of the meshed cells)"""
        seen = self.count >= min_observations
        with np.errstate(all="ignore"):
            F = np.where(seen, self.sum / self.count.astype(f32), f32(1.0)).astype(f32)
        G = self.G
        mask = np.zeros((G, G, G), bool)
        c = np.ones((G - 1,) * 3, bool)
        for d in range(8):
            dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
            c &= seen[dz:dz + G - 1, dy:dy + G - 1, dx:dx + G - 1]
        mask[:G - 1, :G - 1, :G - 1] = c
        return F, mask

    def surface(self, min_observations=1):
        """the mesh mvs_tsdf_surface returns: surface nets of F at iso 0 over the supported cells"""
        F, mask = self.field(min_observations)
        return mo.surface_nets(F, f32(0.0), self.origin, self.h, mask)
