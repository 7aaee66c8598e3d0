"""numpy restatement of mvs_tsdf_raycast (csrc/raycast.hip; the contract: DESIGN.md section 14, include/mvs.h).

Everything is float32 with one rounding per operation, as the kernel computes it without contraction; `/` and sqrt are correctly rounded on
both sides.  The field and the cell mask are tsdf_mirror.Volume.field's, the pixel centres, the back-projection and the projection rows are
fuse_mirror's.  With the matrices mvs_depth_slot_matrices returns the maps are expected bit for bit.

Vectorised over rays, with a loop over the sample index k (only the rays still marching are touched).
  march(...)    rules 2-5 for rays given by origin and unit direction (the low-level entry: rule 2's d_a = 0 branch is reachable here)
  raycast(...)  rule 1 for every pixel of a camera, march, and rule 5's depth
"""
import numpy as np

import fuse_mirror as fm

f32 = np.float32


def _cell_axis(g, G):
    """rule 3: (clamp(floor(g), 0, G - 2), clamp(g - (float)i, 0, 1)); NaN gives 0 for both"""
    fl = np.floor(g)
    i = np.where(fl >= f32(0.0), np.where(fl <= f32(G - 2), fl, f32(G - 2)), f32(0.0)).astype(np.int64)
    r = g - i.astype(f32)
    f = np.where(r > f32(0.0), np.where(r < f32(1.0), r, f32(1.0)), f32(0.0)).astype(f32)
    return i, f


def _point(O, d, t):
    return [O[..., a] + t * d[..., a] for a in range(3)]


def _locate(X, origin, inv_h, G):
    cells = [_cell_axis((X[a] - origin[a]) * inv_h, G) for a in range(3)]
    return [c[0] for c in cells], [c[1] for c in cells]


def _corners(F, idx):
    """v[dk * 4 + dj * 2 + di] of the cell with low corner idx = (ix, iy, iz); F is [k][j][i]"""
    ix, iy, iz = idx
    return [F[iz + (c >> 2), iy + ((c >> 1) & 1), ix + (c & 1)] for c in range(8)]


def _lerp(a, b, f):
    return a + f * (b - a)


def _sample(F, mask, X, origin, inv_h, G):
    idx, (fx, fy, fz) = _locate(X, origin, inv_h, G)
    v = _corners(F, idx)
    c00, c10, c01, c11 = _lerp(v[0], v[1], fx), _lerp(v[2], v[3], fx), _lerp(v[4], v[5], fx), _lerp(v[6], v[7], fx)
    return mask[idx[2], idx[1], idx[0]], _lerp(_lerp(c00, c10, fy), _lerp(c01, c11, fy), fz)


def k_max(G, step_nodes):
    return int(np.floor(1.75 * (G - 1) / float(f32(step_nodes)))) + 2


def march(F, mask, origin, h, O, d, step_nodes):
    """rules 2-5 without the projection.  F, mask: [G, G, G] ([k][j][i]); origin [3], h: the volume; O [N, 3] ray origins, d [N, 3] unit
    directions; -> dict: hit [N] (a crossing was found), ok [N] (and rule 5's cell and gradient tests passed), t [N] (t*), X [N, 3] (X*),
    normal [N, 3], k [N] (index of the hit's current sample, -1: none), t_in, t_out, inside [N] (rule 2 passed), samples (evaluated in all)"""
    F = np.asarray(F, f32)
    G = F.shape[0]
    origin = np.asarray(origin, f32).reshape(3)
    h = f32(h)
    O = np.asarray(O, f32).reshape(-1, 3)
    d = np.asarray(d, f32).reshape(-1, 3)
    N = O.shape[0]
    inv_h = f32(1.0) / h
    delta = f32(step_nodes) * h
    K = k_max(G, step_nodes)
    with np.errstate(all="ignore"):
        hi = (origin + h * f32(G - 1)).astype(f32)
        t_in = np.zeros(N, f32)
        t_out = np.full(N, np.inf, f32)
        inside = np.ones(N, bool)
        for a in range(3):
            nz = d[:, a] != f32(0.0)
            t1 = (origin[a] - O[:, a]) / d[:, a]
            t2 = (hi[a] - O[:, a]) / d[:, a]
            tn = np.where(t1 < t2, t1, t2)
            tf = np.where(t1 < t2, t2, t1)
            t_in = np.where(nz & (tn > t_in), tn, t_in)
            t_out = np.where(nz & (tf < t_out), tf, t_out)
            inside &= nz | ((origin[a] <= O[:, a]) & (O[:, a] <= hi[a]))
        inside &= t_in <= t_out
        hit = np.zeros(N, bool)
        khit = np.full(N, -1, np.int64)
        t_star = np.zeros(N, f32)
        live = np.nonzero(inside)[0]
        prev_ok = np.zeros(N, bool)
        prev_F = np.zeros(N, f32)
        t_prev = t_in.copy()
        samples = 0
        for k in range(K + 1):
            if live.size == 0:
                break
            t = (t_in[live] + delta * f32(k)).astype(f32)
            go = t <= t_out[live]
            live, t = live[go], t[go]
            if live.size == 0:
                break
            samples += live.size
            ok, Fk = _sample(F, mask, _point(O[live], d[live], t), origin, inv_h, G)
            if k >= 1:
                h_now = ok & (Fk <= f32(0.0)) & prev_ok[live] & (prev_F[live] > f32(0.0))
                who = live[h_now]
                pf = prev_F[who]
                t_star[who] = t_prev[who] + delta * (pf / (pf - Fk[h_now]))
                hit[who] = True
                khit[who] = k
                live, t, ok, Fk = live[~h_now], t[~h_now], ok[~h_now], Fk[~h_now]
            prev_ok[live] = ok
            prev_F[live] = Fk
            t_prev[live] = t
        # rule 5
        Xs = _point(O, d, t_star)
        idx, (fx, fy, fz) = _locate(Xs, origin, inv_h, G)
        v = _corners(F, idx)
        gx = _lerp(_lerp(v[1] - v[0], v[3] - v[2], fy), _lerp(v[5] - v[4], v[7] - v[6], fy), fz)
        gy = _lerp(_lerp(v[2] - v[0], v[3] - v[1], fx), _lerp(v[6] - v[4], v[7] - v[5], fx), fz)
        gz = _lerp(_lerp(v[4] - v[0], v[5] - v[1], fx), _lerp(v[6] - v[2], v[7] - v[3], fx), fy)
        gl = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = hit & mask[idx[2], idx[1], idx[0]] & (gl > f32(0.0)) & (gl < f32(np.inf))
        normal = np.stack([gx / gl, gy / gl, gz / gl], -1).astype(f32)
    normal[~ok] = 0
    return {"hit": hit, "ok": ok, "t": t_star, "X": np.stack(Xs, -1).astype(f32), "normal": normal, "k": khit, "t_in": t_in, "t_out": t_out,
            "inside": inside, "samples": samples}


def pixel_rays(mats, W, H):
    """rule 1: (alive [H*W], origins [H*W, 3], unit directions [H*W, 3]) of every pixel, row-major"""
    P, Pi, C = (np.asarray(m, f32) for m in mats[:3])
    rows, cols = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        X1 = fm._unproject(Pi, fm.pixel_xn(cols, W), fm.pixel_yn(rows, H), f32(0.0))
        alive = fm._prow(P, 3, X1) > f32(0.0)
        dv = [(X1[a] - C[a]).astype(f32) for a in range(3)]
        ln = np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
        alive &= (ln > f32(0.0)) & (ln < f32(np.inf))
        d = np.stack([dv[a] / ln for a in range(3)], -1).astype(f32).reshape(-1, 3)
    O = np.broadcast_to(C[:3], d.shape).astype(f32)
    return alive.ravel(), O, d


def raycast(vol, mats, W, H, min_observations=1, step_nodes=0.5, want_info=False):
    """mvs_tsdf_raycast of tsdf_mirror.Volume `vol` for the camera with slot matrices mats = (P, P^-1, centre):
    -> (depth [H, W] f32, normals [H, W, 3] f32) (and march's dict with want_info)"""
    P = np.asarray(mats[0], f32)
    F, mask = vol.field(min_observations)
    alive, O, d = pixel_rays(mats, W, H)
    depth = np.ones(H * W, f32)
    normals = np.zeros((H * W, 3), f32)
    who = np.nonzero(alive)[0]
    m = march(F, mask, vol.origin, vol.h, O[who], d[who], step_nodes)
    with np.errstate(all="ignore"):
        X = [m["X"][:, a] for a in range(3)]
        z = (fm._prow(P, 2, X) / fm._prow(P, 3, X)).astype(f32)
        ok = m["ok"] & (z > f32(-1.0)) & (z < f32(1.0))
    depth[who[ok]] = z[ok]
    normals[who[ok]] = m["normal"][ok]
    out = depth.reshape(H, W), normals.reshape(H, W, 3)
    if want_info:
        m["pixels"] = who
        m["final"] = ok
        return out + (m,)
    return out
