"""Restatement of the resolution pyramid, written from the contract and not from the kernels.  It is the arbiter:
mvs_pyramid_downsample_device and the frames of mvs_pyramid_stage must be bit-identical to downsample(), mvs_pyramid_prior to prior().

Rule D is integer arithmetic.  Rule U is float32 with one rounding per operation: every product and every sum below is a numpy float32
operation on float32 operands, the division too."""
import numpy as np

BACKGROUND_DEPTH = np.float32(1.0)


def inside(z):
    """-1 < z < 1 (false for NaN)"""
    with np.errstate(invalid="ignore"):
        return (z > -1.0) & (z < 1.0)


def downsample(frame):
    """rule D: (f[2r][2c] + f[2r][2c+1] + f[2r+1][2c] + f[2r+1][2c+1] + 2) >> 2 on one frame [H, W] or a stack [..., H, W] of u8"""
    f = np.asarray(frame, np.uint8).astype(np.int64)
    assert f.shape[-1] % 2 == 0 and f.shape[-2] % 2 == 0
    s = f[..., 0::2, 0::2] + f[..., 0::2, 1::2] + f[..., 1::2, 0::2] + f[..., 1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint8)


def taps(n_fine):
    """along one axis of n_fine pixels: (i0, i1, w0, w1) per fine index -- i0 = (i - 1) >> 1 and i1 = i0 + 1, clamped; w0 = 3 for an odd
    index, 1 for an even one; w1 = 4 - w0 (a clamped tap keeps its weight)"""
    i = np.arange(n_fine)
    lo = (i - 1) >> 1                      # arithmetic shift: -1 for i = 0
    n = n_fine // 2
    w0 = np.where(i & 1, 3, 1)
    return np.clip(lo, 0, n - 1), np.clip(lo + 1, 0, n - 1), w0, 4 - w0


def prior(coarse_depth, tau=255, coarse_guide=None, fine_guide=None):
    """rule U: the coarse map [Hc, Wc] float32 -> the prior [2 Hc, 2 Wc] float32"""
    zc = np.asarray(coarse_depth, np.float32)
    Hc, Wc = zc.shape
    H, W = 2 * Hc, 2 * Wc
    r0, r1, wy0, wy1 = taps(H)
    c0, c1, wx0, wx1 = taps(W)
    order = ((r0, c0, wy0, wx0), (r0, c1, wy0, wx1), (r1, c0, wy1, wx0), (r1, c1, wy1, wx1))
    z = [zc[np.ix_(r, c)] for r, c, _, _ in order]
    w = [np.outer(wy, wx).astype(np.int64) for _, _, wy, wx in order]
    valid = [inside(t) for t in z]
    member = valid
    if tau < 255:
        gc, gf = np.asarray(coarse_guide, np.uint8).astype(np.int64), np.asarray(fine_guide, np.uint8).astype(np.int64)
        assert gc.shape == (Hc, Wc) and gf.shape == (H, W)
        like = [v & (np.abs(gc[np.ix_(r, c)] - gf) <= tau) for v, (r, c, _, _) in zip(valid, order)]
        some = like[0] | like[1] | like[2] | like[3]
        member = [np.where(some, l, v) for l, v in zip(like, valid)]
    num = np.zeros((H, W), np.float32)
    sw = np.zeros((H, W), np.int64)
    with np.errstate(invalid="ignore"):
        for t, wk, m in zip(z, w, member):
            p = wk.astype(np.float32) * t                                # (float)w * z, rounded once
            assert p.dtype == np.float32
            num = np.where(m, np.where(sw > 0, num + p, p), num)         # the sum starts at the first member's product
            sw = np.where(m, sw + wk, sw)
        q = num / np.maximum(sw, 1).astype(np.float32)
    assert q.dtype == np.float32
    return np.where((sw > 0) & inside(q), q, BACKGROUND_DEPTH).astype(np.float32)
