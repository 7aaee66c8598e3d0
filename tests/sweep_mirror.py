"""numpy restatement of the sweep's parity contracts (DESIGN.md sections 2, 2a, 2b), written from the text and not from the kernels or from
oracle/sweep_oracle.c, and calling nothing of the oracle.  Every rounding the contract names is performed explicitly:

  * fma          one float32 rounding of the exact a b + c (sgm_mirror._fma32);
  * r            the correctly rounded float32 reciprocal (IEEE division).  The kernels' Newton step misses it only for a significand of
                 all ones; `sweep` asserts that no s.w it inverts is such a number (a condition on the inputs with cap 0);
  * u            ONE round-to-nearest-even of the real s (256 r) + 4: the product of two float32 is exact in float64, and so are its floor
                 and its fraction, so the tie is decided on exact numbers;
  * c, i, a, res the exact sampler's float32 chain of section 2a, one rounding per operation.

`project` and `sample_fixed` take the planes as the table [D] or as a per-pixel map [D, H, W] (the band sweeps and the windowed kernels'
cases, tests/window_cameras.py).  Volumes are [D, H, W] uint32, cells count << 24 | sum (fixed) resp. count << 16 | sum (exact).  `exact_u` is the scalar, exact-rational
form of u before its rounding (fractions.Fraction), for the premises of crafted cases."""
from fractions import Fraction

import numpy as np

from sgm_mirror import _fma32

F = np.float32
BACKGROUND_DEPTH = F(1.0)


def plane_table(D, z_lo=-1.0, z_hi=1.0):
    """plane d sits at the centre of the d-th of D equal slices of [z_lo, z_hi]: double precision, one rounding to float32"""
    d = np.arange(D, dtype=np.float64)
    return (np.float64(z_lo) + (np.float64(z_hi) - np.float64(z_lo)) * (d + 0.5) / np.float64(D)).astype(F)


def weight_table():
    """section 2b: table[b][a] = the four 8-bit weights of sub-texel position (a, b) / 32, [32, 32, 4] uint8, each entry sums to 255"""
    t = np.empty((32, 32, 4), np.uint8)
    for b in range(32):
        for a in range(32):
            p = ((32 - a) * (32 - b), a * (32 - b), (32 - a) * b, a * b)
            w = [(255 * x + 512) >> 10 for x in p]
            w[p.index(max(p))] += 255 - sum(w)   # list.index: the first of the largest
            t[b, a] = w
    return t


def pad_frame(img):
    """GL_REPEAT by padding: one texel of wrap on every side, [H + 2, W + 2]"""
    return np.pad(np.asarray(img, np.uint8), 1, mode="wrap")


def pixel_ndc(W, H):
    """(xn [W], yn [H]) float32: fma(2 col + 1, 1 / W, -1) and fma(-(2 row + 1), 1 / H, 1) with the float32 reciprocals of the sizes"""
    col = (2 * np.arange(W) + 1).astype(F)
    row = (2 * np.arange(H) + 1).astype(F)
    xn = _fma32(col, np.full(W, F(1) / F(W), F), np.full(W, F(-1), F))
    yn = _fma32(-row, np.full(H, F(1) / F(H), F), np.full(H, F(1), F))
    return xn, yn


def project(Q, z, W, H):
    """s = fma(z, B, A) for one view: three [D, H, W] float32 arrays (x, y, w).  z is the plane table [D] or a per-pixel plane map
    [D, H, W]: every pixel of plane d at its own depth (the band sweeps)"""
    Q = np.asarray(Q, F).reshape(3, 4)
    z = np.asarray(z, F)
    assert z.ndim == 1 or z.shape[1:] == (H, W), z.shape
    xn, yn = pixel_ndc(W, H)
    xn = np.broadcast_to(xn[None, :], (H, W)).copy()
    yn = np.broadcast_to(yn[:, None], (H, W)).copy()
    out = []
    for k in range(3):
        full = lambda v: np.full((H, W), v, F)
        A = _fma32(full(Q[k, 0]), xn, _fma32(full(Q[k, 1]), yn, full(Q[k, 3])))
        zz = np.broadcast_to(z[:, None, None] if z.ndim == 1 else z, (len(z), H, W)).copy()
        out.append(_fma32(zz, np.full_like(zz, Q[k, 2]), np.broadcast_to(A[None], zz.shape).copy()))
    return out


def _all_ones(x):
    return (x.view(np.uint32) & np.uint32(0x7fffff)) == np.uint32(0x7fffff)


def reciprocal(sw):
    """(front, r): s.w > 0 and RN(1 / s.w) there (1 elsewhere); asserts the guard of the Newton step"""
    front = sw > 0
    safe = np.where(front, sw, F(1)).astype(F)
    assert not _all_ones(safe).any(), "an s.w with a significand of all ones: outside what the kernels' reciprocal guarantees"
    with np.errstate(over="ignore"):
        return front, (F(1) / safe).astype(F)


def rne_u(s, r):
    """u = RNE(s (256 r) + 4) as int64, and a mask of the samples where the real number was an exact tie (fraction 1/2).  Products too
    large for any frame (or not finite) come back as -1 resp. 2^40: out of every frame either way."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = s.astype(np.float64) * (r.astype(np.float64) * 256.0)   # both exact
    ok = np.isfinite(p) & (np.abs(p) < 2.0 ** 40)
    q = np.where(ok, p, 0.0)
    fl = np.floor(q)
    frac = q - fl                                                    # exact: the bits of q below the binary point
    fi = fl.astype(np.int64)
    up = (frac > 0.5) | ((frac == 0.5) & ((fi & 1) == 1))            # + 4 keeps the parity
    u = fi + 4 + up.astype(np.int64)
    u = np.where(ok, u, np.where(p > 0, np.int64(1) << 40, np.int64(-1)))   # (NaN: -1)
    return u, ok & (frac == 0.5)


def sample_fixed(Q, z, pad, W, H, table=None):
    """section 2b for one view -> dict(valid, dot, ux, uy, tie, kx, ky), [D, H, W] each; z as in `project`.  A sample at a z that is
    not finite (a per-pixel map's dead plane) is not valid"""
    table = weight_table() if table is None else table
    z = np.asarray(z, F)
    finite = np.isfinite(z)
    sx, sy, sw = project(Q, np.where(finite, z, F(0)), W, H)        # (the dead samples are projected at z = 0 and dropped below)
    front, r = reciprocal(sw)
    front = front & np.broadcast_to(finite[:, None, None] if z.ndim == 1 else finite, front.shape)
    ux, tx = rne_u(sx, r)
    uy, ty = rne_u(sy, r)
    valid = front & (ux > 132) & (ux < 256 * W + 132) & (uy > 132) & (uy < 256 * H + 132)
    uxs, uys = np.where(valid, ux, 256), np.where(valid, uy, 256)
    ix, iy, kx, ky = uxs >> 8, uys >> 8, (uxs >> 3) & 31, (uys >> 3) & 31
    pad = np.asarray(pad, np.int64)
    w = table[ky, kx].astype(np.int64)
    dot = w[..., 0] * pad[iy, ix] + w[..., 1] * pad[iy, ix + 1] + w[..., 2] * pad[iy + 1, ix] + w[..., 3] * pad[iy + 1, ix + 1]
    return dict(valid=valid, dot=np.where(valid, dot, 0), ux=ux, uy=uy, tie=front & tx & ty, tie_x=front & tx, tie_y=front & ty, kx=kx, ky=ky, front=front)


def sample_exact(Q, z, pad, W, H):
    """section 2a for one view -> dict(valid, Iq, cx, cy, half): `half` marks the samples whose REAL bilinear value (of the float32 a's)
    has fraction exactly 1/2"""
    sx, sy, sw = project(Q, z, W, H)
    front, r = reciprocal(sw)
    with np.errstate(over="ignore", invalid="ignore"):
        cx, cy = (sx * r).astype(F), (sy * r).astype(F)
        valid = front & (cx > F(0.5)) & (cx < F(W) + F(0.5)) & (cy > F(0.5)) & (cy < F(H) + F(0.5))
    cxs, cys = np.where(valid, cx, F(1)).astype(F), np.where(valid, cy, F(1)).astype(F)
    ix, iy = np.trunc(cxs).astype(np.int64), np.trunc(cys).astype(np.int64)
    ax, ay = (cxs - ix.astype(F)).astype(F), (cys - iy.astype(F)).astype(F)
    pad = np.asarray(pad, np.uint8).astype(F)
    t00, t01, t10, t11 = pad[iy, ix], pad[iy, ix + 1], pad[iy + 1, ix], pad[iy + 1, ix + 1]
    dxt, dy = t01 - t00, t10 - t00
    dxy = (t11 - t10) - dxt
    res = _fma32(ay, _fma32(ax, dxy, dy), _fma32(ax, dxt, (t00 + F(0.5)).astype(F)))
    Iq = np.trunc(res).astype(np.int64)
    a64, b64 = ax.astype(np.float64), ay.astype(np.float64)   # |taps| <= 510 and a < 1 with 24 bits: every term below is exact in float64
    real = t00.astype(np.float64) + a64 * dxt + b64 * dy
    cross = (a64 * b64) * dxy                                  # 48-bit product times a 10-bit integer: exact
    total = real + cross                                       # may round; a fraction of exactly 1/2 needs few bits and is then exact
    half = valid & ((total - np.floor(total)) == 0.5) & ((total - real) == cross)
    return dict(valid=valid, Iq=np.where(valid, Iq, 0), cx=cx, cy=cy, half=half, front=front)


def select(vol, z, cs):
    """section 2's selection: s / c by exact cross multiplication, strict (ties keep the lowest plane), no valid plane -> depth 1.0,
    cost inf, index -1; cost = s / c (cs 16) resp. s / (255 c) (cs 24) in float32"""
    vol = np.asarray(vol, np.uint32).astype(np.int64)
    D, H, W = vol.shape
    bs = np.zeros((H, W), np.int64)
    bc = np.zeros((H, W), np.int64)
    bi = np.full((H, W), -1, np.int64)
    for d in range(D):
        s, c = vol[d] & ((1 << cs) - 1), vol[d] >> cs
        take = (c > 0) & ((bi < 0) | (s * bc < bs * c))
        bs, bc, bi = np.where(take, s, bs), np.where(take, c, bc), np.where(take, d, bi)
    have = bi >= 0
    den = np.where(have, bc * (255 if cs == 24 else 1), 1)
    cost = np.where(have, bs.astype(F) / den.astype(F), F(np.inf)).astype(F)
    depth = np.where(have, np.asarray(z, F)[np.clip(bi, 0, D - 1)], BACKGROUND_DEPTH).astype(F)
    return depth, cost, bi.astype(np.int32)


def sweep(Q, z, main_img, sides, sampler="fixed", details=False):
    """the whole contract: view matrices [V, 3, 4] float32, plane table, main frame and unpadded side frames ->
    (depth, cost, index, volume); with `details` also the per-view sample dictionaries"""
    main = np.asarray(main_img, np.uint8).astype(np.int64)
    H, W = main.shape
    Q = np.asarray(Q, F).reshape(-1, 3, 4)
    z = np.asarray(z, F)
    fixed = sampler == "fixed"
    table = weight_table() if fixed else None
    vol = np.zeros((len(z), H, W), np.int64)
    views = []
    for v in range(len(Q)):
        pad = pad_frame(sides[v])
        if fixed:
            sm = sample_fixed(Q[v], z, pad, W, H, table)
            vol += np.where(sm["valid"], (1 << 24) + np.abs(sm["dot"] - 255 * main[None]), 0)
        else:
            sm = sample_exact(Q[v], z, pad, W, H)
            vol += np.where(sm["valid"], (1 << 16) + np.abs(sm["Iq"] - main[None]), 0)
        views.append(sm)
    vol = vol.astype(np.uint32)
    out = select(vol, z, 24 if fixed else 16) + (vol,)
    return out + (views,) if details else out


def exact_u(Q, col, row, z, W, H, axis=0):
    """the REAL u of section 2b (before its rounding) of pixel (col, row) on the plane at z, as a Fraction, for axis 0 (x) or 1 (y): the
    float32 numbers Q, xn, yn, z taken as exact rationals, s and 1 / s.w without any rounding.  For the premises of crafted cases whose
    float32 projection is exact anyway (dyadic cameras): there it is THE number the contract rounds."""
    Q = np.asarray(Q, F).reshape(3, 4)
    fr = lambda x: Fraction(float(x))
    xn = fr(F(2 * col + 1)) * fr(F(1) / F(W)) - 1
    yn = -fr(F(2 * row + 1)) * fr(F(1) / F(H)) + 1
    s = [fr(Q[k, 0]) * xn + fr(Q[k, 1]) * yn + fr(Q[k, 3]) + fr(F(z)) * fr(Q[k, 2]) for k in range(3)]
    return s[axis] * 256 / s[2] + 4
