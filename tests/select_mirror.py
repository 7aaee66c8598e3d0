"""numpy restatement of the depth selection over the packed volume and of the sub-plane refinement (include/mvs.h: mvs_sweep_argmin,
mvs_sweep_argmin_partial, mvs_sweep_combine_partials, mvs_sweep_refine_depth), written from the contract and not from the kernels.

Volumes are uint32 [D, H, W]; `cs` is the count shift of the packed cell (24: fixed sampler, count << 24 | sum; 16: exact sampler,
count << 16 | sum).  With s the sum and n the count of a cell:

  selection   a cell with n = 0 is never selected; the winner is the LOWEST plane among those with the smallest s / n, compared as
              rationals (exact integers here: s_d n_e <= s_e n_d for every seen e; the products reach 2^32 and live in int64);
              cost = f32(s) / f32(n) (cs 16) or f32(s) / f32(255 n) (cs 24), depth = z[index]; nothing seen: -1, +inf, 1.0
  partial     the same over a slice of planes, as 8-byte records (packed best cell, absolute plane) or (0, 0xffffffff) for none
  combine     records merged in list order; a later part wins only if strictly better
  refinement  with c = s / n of the planes index - 1, index, index + 1 (all three seen, 0 < index < D - 1; everything else keeps
              z[index]): den = ca - 2 cb + cc; den <= 0 keeps z[index]; t = (ca - cc) / (2 den) clamped to [-1/2, 1/2];
              depth = z[index] + t (z[index + 1] - z[index]) for t >= 0, z[index] - t (z[index - 1] - z[index]) otherwise.
              `refine` evaluates it in f32 with one rounding per operation and the final fused multiply-add (the library's
              arithmetic, shared with sgm_mirror.parabola); `refine_exact` in fractions.Fraction.

How far `refine` may be from `refine_exact` (REFINE_K).  u = 2^-24 is the unit roundoff of f32, m = max(ca, cb, cc) >= 0, den* the exact
den.  s < 2^24 and n < 2^16 convert exactly, so each of the three divisions leaves a relative error <= u: |e(ca)|, |e(cb)|, |e(cc)| <= u m.
  2 cb is exact (error <= 2 u m); ca - 2 cb lies in [-2 m, m]: inherited error <= 3 u m, its rounding <= 2 u m;
  adding cc (den in [-2 m, 2 m]): inherited <= 6 u m, its rounding <= 2 u m                          =>  |e(den)| <= 8 u m
  ca - cc lies in [-m, m]: inherited <= 2 u m, rounding <= u m; the halving is exact                  =>  |e(num)| <= 1.5 u m
  t = num / den with |t*| <= 1/2 inside the clamp: |e(t)| <= (|e(num)| + |t*| |e(den)|) / den* + u |t| <= 5.5 u m / den* + u / 2,
  and den* <= 2 m makes u / 2 <= u m / den*                                                            =>  |e(t)| <= 6.5 u m / den*
to first order.  The neglected terms carry the factor 1 / (1 - |e(den)| / den*) <= 1 / (1 - 8 u 2^10) for the pixels compared
(den* >= 2^-10 m), less than 1.001; REFINE_K = 7 covers them.  Beyond the clamp the relative error of t is <= (3 + 8) u m / den* + u, so
t and t* are clamped alike unless |t*| is within 5.75 u m / den* < REFINE_K u m / den* of 1/2: such pixels are left out of the comparison.
The last step multiplies e(t) by the plane step |z[index +- 1] - z[index]| <= 2/3 (D >= 3, planes inside [-1, 1]) and adds the rounding
of that difference (<= u step / 2 after the factor |t| <= 1/2) and of the fused multiply-add (<= u / 2 for |depth| < 1): together < u.
  |z_f32 - z_exact| <= step REFINE_K 2^-24 m / den* + 2^-24."""
import collections
import fractions

import numpy as np

import sgm_mirror as sgm

BACKGROUND_DEPTH = sgm.BACKGROUND_DEPTH
NONE_RECORD = (0, 0xffffffff)
REFINE_K = 7


def _winners(s, n):
    """[D, H, W] bool: the seen cells whose s / n no seen cell of the pixel undercuts"""
    lhs = s[:, None] * n[None, :]          # s_d n_e
    rhs = s[None, :] * n[:, None]          # s_e n_d
    return ((lhs <= rhs) | (n[None, :] == 0)).all(axis=1) & (n != 0)


def cost_of(s, n, cs):
    """f32 mean cost in grey levels of cells with n != 0"""
    den = n.astype(np.float32) if cs == 16 else (255 * n).astype(np.float32)
    return s.astype(np.float32) / den


def select(vol, cs, z):
    """-> (index i32, cost f32, depth f32), [H, W] each"""
    s, n = sgm.split(vol, cs)
    win = _winners(s, n)
    any_seen = win.any(axis=0)
    first = win.argmax(axis=0)             # the first True: the lowest plane
    bs, bn = (np.take_along_axis(a, first[None], axis=0)[0] for a in (s, n))
    cost = cost_of(bs, np.where(any_seen, bn, 1), cs)
    z = np.asarray(z, np.float32)
    return (np.where(any_seen, first, -1).astype(np.int32), np.where(any_seen, cost, np.float32(np.inf)).astype(np.float32),
            np.where(any_seen, z[first], BACKGROUND_DEPTH).astype(np.float32))


def select_partial(vol_slice, cs, plane_first):
    """-> uint32 [H, W, 2]: (packed best cell, absolute plane) of the slice's planes, NONE_RECORD where the slice shows the pixel nothing"""
    vol_slice = np.asarray(vol_slice, np.uint32)
    s, n = sgm.split(vol_slice, cs)
    win = _winners(s, n)
    any_seen = win.any(axis=0)
    first = win.argmax(axis=0)
    cell = np.take_along_axis(vol_slice, first[None], axis=0)[0]
    rec = np.empty(vol_slice.shape[1:] + (2,), np.uint32)
    rec[..., 0] = np.where(any_seen, cell, NONE_RECORD[0])
    rec[..., 1] = np.where(any_seen, first + plane_first, NONE_RECORD[1])
    return rec


def combine(records, cs, z):
    """records (a sequence of [H, W, 2] uint32) merged in list order -> (index, cost, depth) as select"""
    records = [np.asarray(r, np.uint32) for r in records]
    shape = records[0].shape[:2]
    bs, bn, bi = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.full(shape, -1, np.int64)
    for r in records:
        s, n = sgm.split(r[..., 0], cs)
        there = (r[..., 1] != NONE_RECORD[1]) & (n != 0)
        better = there & ((bi < 0) | (s * bn < bs * n))
        bs, bn, bi = np.where(better, s, bs), np.where(better, n, bn), np.where(better, r[..., 1].astype(np.int64), bi)
    have = bi >= 0
    z = np.asarray(z, np.float32)
    cost = cost_of(bs, np.where(have, bn, 1), cs)
    return (bi.astype(np.int32), np.where(have, cost, np.float32(np.inf)).astype(np.float32),
            np.where(have, z[np.clip(bi, 0, len(z) - 1)], BACKGROUND_DEPTH).astype(np.float32))


def plain_depth(z, index):
    z = np.asarray(z, np.float32)
    return np.where(index >= 0, z[np.clip(index, 0, len(z) - 1)], BACKGROUND_DEPTH).astype(np.float32)


def neighbour_costs(vol, cs, index):
    """-> (ca, cb, cc, ok): the f32 means s / n (both layouts: the refinement does not divide by 255) of the planes index - 1, index,
    index + 1 and where all three exist and are seen; D >= 3"""
    vol = np.asarray(vol, np.uint32)
    D = vol.shape[0]
    s, n = sgm.split(vol, cs)
    i = np.clip(index, 1, D - 2).astype(np.int64)[None]
    ok = (index > 0) & (index < D - 1)
    c = []
    for k in (-1, 0, 1):
        sk, nk = np.take_along_axis(s, i + k, axis=0)[0], np.take_along_axis(n, i + k, axis=0)[0]
        ok &= nk != 0
        c.append(sk.astype(np.float32) / np.where(nk == 0, 1, nk).astype(np.float32))
    return c[0], c[1], c[2], ok


def refine(vol, cs, z, index):
    """the refined depth map, f32: the library's arithmetic"""
    index = np.asarray(index, np.int32)
    if np.asarray(vol).shape[0] < 3:       # no plane has two neighbours
        return plain_depth(z, index)
    ca, cb, cc, ok = neighbour_costs(vol, cs, index)
    return sgm.parabola(ca, cb, cc, ok, z, index)


# z: the refined depth (float64 of the exact value); den, m, t: the exact den*, max(ca, cb, cc) and clamped-free vertex t* as float64 (0 where
# the pixel has no parabola); parabola: all three cells seen around an interior index; refined: parabola and den* > 0
Exact = collections.namedtuple("Exact", "z den m t parabola refined")


def refine_exact(vol, cs, z, index):
    """the same rule in fractions.Fraction (the f32 plane depths taken as the exact numbers they are) -> Exact"""
    vol = np.asarray(vol, np.uint32)
    D, H, W = vol.shape
    zf = [fractions.Fraction(float(v)) for v in np.asarray(z, np.float32)]
    mask = (1 << cs) - 1
    out = Exact(*(np.zeros((H, W), np.float64) for _ in range(4)), np.zeros((H, W), bool), np.zeros((H, W), bool))
    half = fractions.Fraction(1, 2)
    for y in range(H):
        for x in range(W):
            i = int(index[y, x])
            if i < 0:
                out.z[y, x] = float(BACKGROUND_DEPTH)
                continue
            zr = zf[i]
            if 0 < i < D - 1:
                cells = [int(vol[i + k, y, x]) for k in (-1, 0, 1)]
                if all(c >> cs for c in cells):
                    ca, cb, cc = (fractions.Fraction(c & mask, c >> cs) for c in cells)
                    den = ca - 2 * cb + cc
                    out.parabola[y, x] = True
                    out.den[y, x], out.m[y, x] = float(den), float(max(ca, cb, cc))
                    if den > 0:
                        t = (ca - cc) / (2 * den)
                        out.t[y, x] = float(t)
                        out.refined[y, x] = True
                        t = max(-half, min(half, t))
                        zr = zf[i] + t * (zf[i + 1] - zf[i]) if t >= 0 else zf[i] - t * (zf[i - 1] - zf[i])
            out.z[y, x] = float(zr)
    return out
