"""The lens contract of DESIGN.md section 17 in numpy: rules 1-4 (the source position of every output pixel) on float32 arrays with one
rounding per operation, rule 5 (the fixed-point bicubic sample with a replicated border) on integers.  Written from the section, not
from csrc/lens.hip; the device is compared with it for equality."""
import numpy as np

from sgm_mirror import _fma32

F = np.float32


def center_of(W, H, center=None):
    """the centre in pixels, y from the bottom; None: the frame's centre"""
    return (W / 2.0, H / 2.0) if center is None else (float(center[0]), float(center[1]))


def k_of(k):
    """three float32 coefficients from up to three numbers"""
    kk = np.zeros(3, F)
    k = np.asarray(k, F).reshape(-1)
    kk[:min(3, len(k))] = k[:3]
    return kk


def radial_factor(r2, k):
    """rule 3: k = 1 + r2 (k1 + r2 (k2 + r2 k3)), Horner, every product and sum rounded to float32"""
    r2 = np.asarray(r2, F)
    k = k_of(k)
    return F(1) + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))


def positions(W, H, k, center=None):
    """rules 1-4 -> (mx, my): [H, W] float32 source positions in pixel indices of the distorted frame"""
    cx, cy = center_of(W, H, center)
    a = F(H) / F(W)                       # rounded once
    hc = F(H) - F(cy)                     # rounded once (the centre's y is measured from the bottom)
    inv_w, inv_h = F(1) / F(W), F(1) / F(H)
    col = (2 * np.arange(W) + 1).astype(F)[None, :].repeat(H, 0)
    row = (2 * np.arange(H) + 1).astype(F)[:, None].repeat(W, 1)
    xn = _fma32(col, np.full_like(col, inv_w), np.full_like(col, F(-1)))     # rule 1: the sweep's pixel centres, one fma each
    yn = _fma32(-row, np.full_like(row, inv_h), np.full_like(row, F(1)))
    r2 = (xn * xn + ((yn * yn) * a) * a) * F(0.25)                           # rule 2
    kf = radial_factor(r2, k)                                                # rule 3
    X = F(cx) + ((xn * kf) * F(W)) * F(0.5)                                  # rule 4, left to right
    Y = hc - ((yn * kf) * F(H)) * F(0.5)
    mx, my = X - F(0.5), Y - F(0.5)
    assert mx.dtype == F and my.dtype == F
    return mx, my


_TABLE = None


def cubic_table():
    """the Q15 bicubic table (a = -0.75) for 32 x 32 fractions, [1024, 16] int16: entry (fy * 32 + fx) holds the weights of the 4 x 4 taps,
    rows first.  float32 coefficients c0..c2 from the cubic, c3 = 1 - c0 - c1 - c2; weight = rint(cy cx 32768) saturated to int16; a
    sum that is not 32768 is corrected on the largest (sum too small) or smallest (too large) of the four central taps."""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    A = F(-0.75)
    t1 = np.zeros((32, 4), F)
    for i in range(32):
        x = F(i) * (F(1) / F(32))
        x1, xm = x + F(1), F(1) - x
        c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
        c1 = ((A + F(2)) * x - (A + F(3))) * x * x + F(1)
        c2 = ((A + F(2)) * xm - (A + F(3))) * xm * xm + F(1)
        t1[i] = (c0, c1, c2, F(1) - c0 - c1 - c2)
    tab = np.zeros((1024, 16), np.int64)
    for i in range(32):
        for j in range(32):
            w = np.clip(np.rint((t1[i][:, None] * t1[j][None, :]) * F(32768)).astype(np.int64), -32768, 32767).reshape(16)
            diff = int(w.sum()) - 32768
            if diff:
                big = small = 10
                for t in (10, 11, 14, 15):          # the central taps (k1, k2 in 2..3), in scan order
                    if w[t] < w[small]:
                        small = t
                    elif w[t] > w[big]:
                        big = t
                w[big if diff < 0 else small] -= diff
            tab[i * 32 + j] = w
    _TABLE = tab.astype(np.int16)
    return _TABLE


def sample(frame, mx, my, raw=False):
    """rule 5: q = rint(32 m) (ties to even), integer part and 5-bit fraction, 16 taps with replicated border, (sum + 2^14) >> 15,
    saturated to 0..255.  raw=True: the value before the saturation"""
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape
    qx = np.rint(np.asarray(mx, F) * F(32)).astype(np.int64)
    qy = np.rint(np.asarray(my, F) * F(32)).astype(np.int64)
    sx = np.clip((qx >> 5) - 1, -32767, 32767)
    sy = np.clip((qy >> 5) - 1, -32767, 32767)
    w = cubic_table().astype(np.int64)[(qy & 31) * 32 + (qx & 31)]           # [..., 16]
    img = frame.astype(np.int64)
    total = np.zeros(qx.shape, np.int64)
    for k1 in range(4):
        yy = np.clip(sy + k1, 0, H - 1)
        for k2 in range(4):
            xx = np.clip(sx + k2, 0, W - 1)
            total += img[yy, xx] * w[..., k1 * 4 + k2]
    v = (total + (1 << 14)) >> 15
    return v if raw else np.clip(v, 0, 255).astype(np.uint8)


def undistort(frame, k, center=None):
    """a distorted H x W u8 frame -> the pinhole frame (every pixel written)"""
    H, W = np.asarray(frame).shape
    mx, my = positions(W, H, k, center)
    return sample(frame, mx, my)


def undistort_map(W, H, k, center=None):
    """what mvs_undistort_map returns: [H, W, 2] float32"""
    return np.stack(positions(W, H, k, center), -1)


def folds_over(W, H, k):
    """mvs_set_lens's fold-over test: d(rho k(rho^2))/d rho <= 0 at one of 1024 radii up to the farthest corner (double)"""
    k = k_of(k).astype(np.float64)
    a = H / W
    rho = np.sqrt((1.0 + a * a) * 0.25) * np.arange(1, 1025) / 1024.0
    s = rho * rho
    return bool((~(1.0 + s * (3.0 * k[0] + s * (5.0 * k[1] + s * 7.0 * k[2])) > 0.0)).any())
