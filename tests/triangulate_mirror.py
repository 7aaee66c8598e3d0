"""Whole-image numpy restatement of triangulatePixels() as oracle/triangulate_oracle.c's header comment and SURVEY.md A-2, A-14 ... A-17
state it, WITH the per-pixel diagnostics that neither the oracle nor the library expose.  Test infrastructure only.

Every statement of the oracle is one vectorised statement here, with the same roundings: `f32(...)` wherever the oracle stores a float,
f64 accumulation of every matrix product term by term in the oracle's order, f32 arithmetic where the oracle's operands are floats.
What is restated:
  - pixel -> NDC without the half pixel; the flow's y ADDED to an upward y
  - goodSample with C's truncating (int) cast; sampleImage<float> with the LEFT texel weighted by frac(x) (weights swapped)
  - the Sobel gradient read as two int32, interpolated in integer arithmetic (every product rounded to nearest even and saturated,
    sums wrapping), the int bits stored back as a float
  - (A A^T)^-1 / variance with an exact `det == 0` test that yields the zero matrix
  - the `mz < -1` drop
  - Newton on the NDC depth, at most 50 steps, masked: a pixel leaves the iteration at the step where |dz| < 1e-7
  - pdf = 0.159 prod det(icov) exp(exponent / 2)
  - PCA over the valid points of the 21 x 21 window, ACCUMULATED IN WINDOW SCAN ORDER (row by row, left to right), so that the f64 sums
    of mean and covariance are the oracle's; cyclic Jacobi with its `== 0` skips and its `off < 1e-300` exit; orientation vote
  - fewer than 3 neighbours: sum_i v_i / |v_i|^2 with the un-dehomogenised point
  - scaling by pdf^(1/V) / |n|
Columns 0-3 of the rows are the oracle's bit for bit; columns 4-6 go through numpy's exp / power instead of libm's and agree within the
project's stated rtol = 1e-5 (tests/test_triangulate_cases_cpu.py asserts both).

Diagnostics (dense H x W maps unless noted), the reason this file exists -- a test can prove that a crafted case reaches the branch
it was built for:
  status         STATUS_BACKGROUND / STATUS_DROPPED (some side view saw the measured point at NDC z < -1) / STATUS_POINT
  steps          the Newton step at which the pixel stopped, 0 .. 50 (0 elsewhere than at points)
  good_sample    (V, H, W) bool: goodSample() held for that view          } evaluated for every view of every non-background pixel,
  det0           (V, H, W) bool: that view's 2 x 2 was exactly singular   } including views after the one that dropped the pixel
  n_neigh        valid points in the pixel's window, itself included (0 elsewhere than at points)
  normal_branch  BRANCH_NONE / BRANCH_PCA / BRANCH_FALLBACK
  pdf            the pdf before the V-th root (NaN elsewhere than at points)
"""
import numpy as np

f32, f64 = np.float32, np.float64
BACKGROUND = f32(1.0)
RADIUS = 10
MAX_STEPS = 50
STATUS_BACKGROUND, STATUS_DROPPED, STATUS_POINT = 0, 1, 2
BRANCH_NONE, BRANCH_PCA, BRANCH_FALLBACK = 0, 1, 2


def _acc(terms):
    """s = 0; s += (double)a * (double)b for every (a, b), in order"""
    s = f64(0.0)
    for a, b in terms:
        s = s + np.asarray(a, f64) * np.asarray(b, f64)
    return s


def inv44_f32(m):
    """cv::Mat::inv() of the 4 x 4 camera: the double cofactor inverse rounded to f32"""
    a = np.asarray(m, f32).astype(f64).ravel()
    c = [None] * 16
    c[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10]
    c[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10]
    c[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9]
    c[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9]
    c[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10]
    c[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10]
    c[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9]
    c[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9]
    c[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6]
    c[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6]
    c[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5]
    c[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5]
    c[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6]
    c[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6]
    c[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5]
    c[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5]
    det = a[0] * c[0] + a[1] * c[4] + a[2] * c[8] + a[3] * c[12]
    rd = f64(1.0) / det
    return np.array([ci * rd for ci in c], f64).astype(f32).reshape(4, 4)


def camera_center(cam):
    """util.cpp:33-41: the null vector of rows 0, 1, 3, normalised in double, stored as f32, dehomogenised in f32"""
    p = np.asarray(cam, f32).astype(f64).reshape(4, 4)[[0, 1, 3]]

    def det3(c0, c1, c2):
        return (p[0][c0] * (p[1][c1] * p[2][c2] - p[1][c2] * p[2][c1]) - p[0][c1] * (p[1][c0] * p[2][c2] - p[1][c2] * p[2][c0]) +
                p[0][c2] * (p[1][c0] * p[2][c1] - p[1][c1] * p[2][c0]))
    c = [det3(1, 2, 3), -det3(0, 2, 3), det3(0, 1, 3), -det3(0, 1, 2)]
    n = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3])
    t = np.array([ci / n if n > 0 else ci for ci in c], f64).astype(f32)
    return t[:3] / t[3]


def image_gradient(img):
    """imageGradient: separable 3 x 3 Sobel in f32, BORDER_REFLECT_101 -> (H, W, 2)"""
    v = np.pad(np.asarray(img, f32), 1, mode="reflect")
    H, W = img.shape
    t = [[v[j:j + H, i:i + W] for i in range(3)] for j in range(3)]
    rdx = [t[j][2] - t[j][0] for j in range(3)]
    rsm = [t[j][0] + t[j][1] * f32(2.0) + t[j][2] for j in range(3)]
    return np.stack([rdx[0] + rdx[1] * f32(2.0) + rdx[2], rsm[2] - rsm[0]], -1)


def _round_sat(v):
    """cv::saturate_cast<int>(float): round to nearest even, saturating (NaN -> INT_MIN)"""
    lo = ~(v > f32(-2147483648.0))
    hi = ~(v < f32(2147483648.0)) & ~lo
    r = np.rint(np.where(lo | hi, f32(0), v)).astype(np.int64)
    return np.where(lo, -2 ** 31, np.where(hi, 2 ** 31 - 1, r)).astype(np.int32)


def _wrap_add(a, b):
    return (a.view(np.uint32) + b.view(np.uint32)).view(np.int32)


def _sample_point_punned(grad_bits, W, H, x, y):
    """sampleImage<cv::Point> on the CV_32FC2 gradient: (N, 2) floats holding the int results' bits"""
    one = f32(1)
    lw = np.fmod(x, one)
    rw = one - lw
    tw = np.fmod(y, one)
    bw = one - tw
    ix, iy = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
    ix1, iy1 = np.where(ix + 1 < W, ix + 1, ix), np.where(iy + 1 < H, iy + 1, iy)
    out = np.empty((len(x), 2), np.int32)
    for c in range(2):
        g = grad_bits[..., c]
        b00, b01, b10, b11 = (g[iy, ix].astype(f32), g[iy, ix1].astype(f32), g[iy1, ix].astype(f32), g[iy1, ix1].astype(f32))
        top = _wrap_add(_round_sat(b00 * lw), _round_sat(b01 * rw))
        bot = _wrap_add(_round_sat(b10 * lw), _round_sat(b11 * rw))
        out[:, c] = _wrap_add(_round_sat(top.astype(f32) * tw), _round_sat(bot.astype(f32) * bw))
    return out.view(f32)


def _mat44_vec(M, v):
    """(4 x 4 f32) times N column vectors given as a list of four f32 arrays -> list of four f32 arrays"""
    return [_acc((M[i, k], v[k]) for k in range(4)).astype(f32) for i in range(4)]


def _smallest_eigvec3(a):
    """cyclic Jacobi on M symmetric 3 x 3 matrices at once; every matrix follows the oracle's own sequence of rotations"""
    a = a.copy()
    M = a.shape[0]
    Vm = np.broadcast_to(np.eye(3), (M, 3, 3)).copy()
    running = np.ones(M, bool)
    for _ in range(32):
        off = np.abs(a[:, 0, 1]) + np.abs(a[:, 0, 2]) + np.abs(a[:, 1, 2])
        running &= ~(off < 1e-300)
        if not running.any():
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            j = np.nonzero(running & ~(a[:, p, q] == 0.0))[0]
            if not len(j):
                continue
            s_ = a[j]
            theta = (s_[:, q, q] - s_[:, p, p]) / (2.0 * s_[:, p, q])
            t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            c, s = c[:, None], s[:, None]
            akp, akq = s_[:, :, p].copy(), s_[:, :, q].copy()
            s_[:, :, p] = c * akp - s * akq
            s_[:, :, q] = s * akp + c * akq
            apk, aqk = s_[:, p, :].copy(), s_[:, q, :].copy()
            s_[:, p, :] = c * apk - s * aqk
            s_[:, q, :] = s * apk + c * aqk
            a[j] = s_
            v_ = Vm[j]
            vkp, vkq = v_[:, :, p].copy(), v_[:, :, q].copy()
            v_[:, :, p] = c * vkp - s * vkq
            v_[:, :, q] = s * vkp + c * vkq
            Vm[j] = v_
    m = np.where(a[:, 1, 1] < a[:, 0, 0], 1, 0)
    amm = np.where(m == 1, a[:, 1, 1], a[:, 0, 0])
    m = np.where(a[:, 2, 2] < amm, 2, m)
    return Vm[np.arange(M), :, m]


class Result:
    """rows: (N, 7) f32 in pixel scan order; the diagnostics of the module docstring as attributes"""


# Defects a kernel could plausibly have, injectable here so that the CPU test can show which case catches each (the defect's rows fail
# triangulate_cases.compare_rows against the oracle).  None of them is a defect of the library.  (Not in the list: truncating instead of
# rounding the punned gradient's products.  The gradient's bit patterns are integers near 1e9, so a product is a whole number unless
# its weight is below 2^-7, and then it moves the result's last mantissa bit: 1e-7 of a gradient, far inside the pdf's tolerance.)
DEFECTS = (
    "gs_low_inclusive",    # goodSample accepts column 0 / row 0
    "weights_unswapped",   # sampleImage<float> with the conventional weights
    "det0_inverted",       # a singular 2 x 2 inverted anyway (1 / 0) instead of giving the zero matrix
    "no_drop",             # the mz < -1 test missing
    "cap_49",              # the Newton cap one step early
    "window_short_cols",   # the window's last column (+10) not visited: an apron one cell short
    "window_short_rows",   # the window's last row (+10) not visited
    "n_gt_3",              # PCA only from 4 neighbours on
    "fallback_dehomog",    # the fallback normal from the dehomogenised point
    "no_flip",             # the orientation vote ignored
    "no_root",             # pdf not taken to the power 1 / V
)


def triangulate_pixels(flows, main_cam, side_cams, depth, defect=None):
    assert defect is None or defect in DEFECTS
    with np.errstate(all="ignore"):
        return _triangulate(flows, main_cam, side_cams, depth, defect)


def _triangulate(flows, main_cam, side_cams, depth, defect):
    max_steps = MAX_STEPS - 1 if defect == "cap_49" else MAX_STEPS
    depth = np.ascontiguousarray(depth, f32)
    H, W = depth.shape
    V = len(flows)
    flows = [np.asarray(f, f32).reshape(H * W, 4) for f in flows]
    main_cam = np.asarray(main_cam, f32).reshape(4, 4)
    side_cams = np.asarray(side_cams, f32).reshape(V, 4, 4)
    Minv = inv44_f32(main_cam)
    CM, B, projDeriv, projW = [], [], [], []
    for Cm in side_cams:
        CM.append(np.array([[_acc((Cm[i, k], Minv[k, j]) for k in range(4)) for j in range(4)] for i in range(4)], f64).astype(f32))
        B.append(np.array([[_acc((Cm[r, k], Minv[k, c]) for k in range(3)) for c in range(3)] for r in range(2)], f64).astype(f32))
        projDeriv.append(np.array([_acc((Cm[r, k], Minv[k, 2]) for k in range(4)) for r in range(2)], f64).astype(f32))
        projW.append(np.array([_acc((Cm[3, k], Minv[k, c]) for k in range(4)) for c in range(4)], f64).astype(f32))
    grad_bits = image_gradient(depth).view(np.int32)

    res = Result()
    res.status = np.zeros((H, W), np.uint8)
    res.steps = np.zeros((H, W), np.int32)
    res.good_sample = np.zeros((V, H, W), bool)
    res.det0 = np.zeros((V, H, W), bool)
    res.n_neigh = np.zeros((H, W), np.int32)
    res.normal_branch = np.zeros((H, W), np.uint8)
    res.pdf = np.full((H, W), np.nan, f32)

    # ---- measured points and inverse covariances, every non-background pixel at once -------------------------------------------
    fg = np.nonzero(depth.ravel() != BACKGROUND)[0]
    row, col = fg // W, fg % W
    d0 = depth.ravel()[fg]
    one = f32(1)
    centerX, centerY, scaleX, scaleY = f32(W) / f32(2), f32(H) / f32(2), f32(2) / f32(W), f32(2) / f32(H)
    colf, rowf = col.astype(f32), row.astype(f32)
    x, y = (colf - centerX) * scaleX, (centerY - rowf) * scaleY
    meas, icov = [], []
    dropped = np.zeros(len(fg), bool)
    for i in range(V):
        flx, fly, variance = flows[i][fg, 0], flows[i][fg, 1], flows[i][fg, 2]
        xs, ys = colf + flx, rowf + fly
        ix, iy = np.trunc(xs).astype(np.int64), np.trunc(ys).astype(np.int64)
        if defect == "gs_low_inclusive":
            inside = ~((ix < 0) | (ix >= W - 1) | (iy < 0) | (iy >= H - 1))
        else:
            inside = ~((ix <= 0) | (ix >= W - 1) | (iy <= 0) | (iy >= H - 1))
        jx, jy = np.where(inside, ix, 0), np.where(inside, iy, 0)
        gs = inside & (depth[jy, jx] != BACKGROUND) & (depth[jy, jx + 1] != BACKGROUND) & (depth[jy + 1, jx] != BACKGROUND) & \
            (depth[jy + 1, jx + 1] != BACKGROUND)
        lw = np.fmod(xs, one)
        rw = one - lw
        tw = np.fmod(ys, one)
        bw = one - tw
        if defect == "weights_unswapped":
            lw, rw, tw, bw = rw, lw, bw, tw
        zs = (depth[jy, jx] * lw + depth[jy, jx + 1] * rw) * tw + (depth[jy + 1, jx] * lw + depth[jy + 1, jx + 1] * rw) * bw
        z = np.where(gs, zs, d0)
        mp = _mat44_vec(CM[i], [x + flx * scaleX, y + fly * scaleY, z, np.ones_like(z)])
        g = _sample_point_punned(grad_bits, W, H, np.where(gs, xs, colf), np.where(gs, ys, rowf))
        A = [[None, None], [None, None]]
        for r in range(2):
            for c in range(2):
                s = f64(B[i][r, 0]) * (1.0 if c == 0 else 0.0) + f64(B[i][r, 1]) * (1.0 if c == 1 else 0.0) + f64(B[i][r, 2]) * g[:, c].astype(f64)
                A[r][c] = s.astype(f32) / mp[3]
        S = [[(A[r][0].astype(f64) * A[c][0].astype(f64) + A[r][1].astype(f64) * A[c][1].astype(f64)).astype(f32) for c in range(2)]
             for r in range(2)]
        det = S[0][0].astype(f64) * S[1][1].astype(f64) - S[0][1].astype(f64) * S[1][0].astype(f64)
        nz = det != 0.0
        if defect == "det0_inverted":
            nz = np.ones_like(nz)
        rd = 1.0 / det
        zero = np.zeros(len(fg), f32)
        inv = [np.where(nz, (S[1][1].astype(f64) * rd).astype(f32), zero), np.where(nz, ((-S[0][1]).astype(f64) * rd).astype(f32), zero),
               np.where(nz, ((-S[1][0]).astype(f64) * rd).astype(f32), zero), np.where(nz, (S[0][0].astype(f64) * rd).astype(f32), zero)]
        icov.append([v / variance for v in inv])
        if defect != "no_drop":
            dropped |= (mp[2] / mp[3]) < -1
        meas.append((mp[0] / mp[3], mp[1] / mp[3]))
        res.good_sample[i].ravel()[fg] = gs
        res.det0[i].ravel()[fg] = det == 0.0
    res.status.ravel()[fg] = np.where(dropped, STATUS_DROPPED, STATUS_POINT)

    # ---- triangulatePixel: masked Newton -------------------------------------------------------------------------------------------
    keep = np.nonzero(~dropped)[0]
    pix = fg[keep]
    N = len(pix)
    kx, ky, kz = x[keep], y[keep], d0[keep].copy()
    meas = [(m0[keep], m1[keep]) for m0, m1 in meas]
    icov = [[v[keep] for v in ic] for ic in icov]
    steps = np.zeros(N, np.int32)
    pdf = np.ones(N, f32)
    act = np.arange(N)
    for it in range(max_steps + 1):
        if not len(act):
            break
        k = [kx[act], ky[act], kz[act], np.ones(len(act), f32)]
        firstDz, secondDz = np.zeros(len(act)), np.zeros(len(act))
        diffs = []
        for i in range(V):
            ep = _mat44_vec(CM[i], k)
            px, py = ep[0] / ep[3], ep[1] / ep[3]
            pw = _acc((projW[i][c], k[c]) for c in range(4)).astype(f32)
            dpx, dpy = projDeriv[i][0] / pw, projDeriv[i][1] / pw
            d = (px - meas[i][0][act], py - meas[i][1][act])
            ic = [v[act].astype(f64) for v in icov[i]]
            t0 = (ic[0] * dpx.astype(f64) + ic[1] * dpy.astype(f64)).astype(f32)
            t1 = (ic[2] * dpx.astype(f64) + ic[3] * dpy.astype(f64)).astype(f32)
            firstDz = firstDz + (d[0].astype(f64) * t0.astype(f64) + d[1].astype(f64) * t1.astype(f64))
            secondDz = secondDz + (dpx.astype(f64) * t0.astype(f64) + dpy.astype(f64) * t1.astype(f64))
            diffs.append(d)
        delta = -firstDz / secondDz
        done = (delta < 1e-7) & (delta > -1e-7) if it < max_steps else np.ones(len(act), bool)
        if done.any():
            exponent, product = np.zeros(int(done.sum())), np.ones(int(done.sum()))
            for i in range(V):
                d0_, d1_ = diffs[i][0][done].astype(f64), diffs[i][1][done].astype(f64)
                ic = [v[act][done].astype(f64) for v in icov[i]]
                t0 = (ic[0] * d0_ + ic[1] * d1_).astype(f32)
                t1 = (ic[2] * d0_ + ic[3] * d1_).astype(f32)
                exponent = exponent - (d0_ * t0.astype(f64) + d1_ * t1.astype(f64))
                product = product * (ic[0] * ic[3] - ic[1] * ic[2])
            pdf[act[done]] = (0.159 * product * np.exp(0.5 * exponent)).astype(f32)
            steps[act[done]] = it
        go = ~done
        kz[act[go]] = (kz[act[go]].astype(f64) + delta[go]).astype(f32)
        act = act[go]
    pts = np.stack(_mat44_vec(Minv, [kx, ky, kz, np.ones(N, f32)]), 1) if N else np.zeros((0, 4), f32)
    res.steps.ravel()[pix] = steps
    res.pdf.ravel()[pix] = pdf

    # ---- normals ---------------------------------------------------------------------------------------------------------------------
    centers = [camera_center(main_cam)] + [camera_center(c) for c in side_cams]
    R = RADIUS
    validp = np.zeros((H + 2 * R, W + 2 * R), bool)
    quot = np.zeros((H + 2 * R, W + 2 * R, 3))
    prow, pcol = pix // W, pix % W
    validp[prow + R, pcol + R] = True
    if N:
        quot[prow + R, pcol + R] = (pts[:, :3] / pts[:, 3:4]).astype(f64)     # the f32 quotient q[c] / q[3], widened
    window = [(dy, dx) for dy in range(2 * R + 1) for dx in range(2 * R + 1)]     # the oracle's scan order
    if defect in ("window_short_cols", "window_short_rows"):
        window = [(dy, dx) for dy, dx in window if (dx if defect == "window_short_cols" else dy) < 2 * R]
    n = np.zeros(N, np.int32)
    mean = np.zeros((N, 3))
    for dy, dx in window:
        m = validp[prow + dy, pcol + dx]
        mean = mean + np.where(m[:, None], quot[prow + dy, pcol + dx], 0.0)
        n += m
    normal = np.zeros((N, 3), f32)
    pca = n > 3 if defect == "n_gt_3" else n >= 3
    pq = (pts[:, :3] / pts[:, 3:4]) if N else np.zeros((0, 3), f32)
    if pca.any():
        j = np.nonzero(pca)[0]
        jr, jc = prow[j], pcol[j]
        mu = mean[j] / n[j, None]
        cov = np.zeros((len(j), 3, 3))
        for dy, dx in window:
            m = validp[jr + dy, jc + dx]
            if not m.any():
                continue
            d = quot[jr + dy, jc + dx] - mu
            for a in range(3):
                for b in range(a, 3):
                    cov[:, a, b] = cov[:, a, b] + np.where(m, d[:, a] * d[:, b], 0.0)
        for a in range(3):
            for b in range(a, 3):
                cov[:, a, b] = cov[:, a, b] / n[j]
                cov[:, b, a] = cov[:, a, b]
        nv = _smallest_eigvec3(cov).astype(f32)
        dot = np.zeros(len(j), f32)
        for ctr in centers:
            s = _acc((nv[:, c], ctr[c] - pq[j, c]) for c in range(3))
            dot = dot + (1.0 / s).astype(f32)
        normal[j] = nv if defect == "no_flip" else np.where((dot < 0)[:, None], -nv, nv)
    if (~pca).any():
        j = np.nonzero(~pca)[0]
        nf = np.zeros((len(j), 3), f32)
        for ctr in centers:
            vec = [ctr[c] - (pq if defect == "fallback_dehomog" else pts)[j, c] for c in range(3)]   # not dehomogenised: util.cpp:319
            vv = _acc((vec[c], vec[c]) for c in range(3))
            for c in range(3):
                nf[:, c] = nf[:, c] + (vec[c].astype(f64) / vv).astype(f32)
        normal[j] = nf
    scale = pdf
    if V > 1 and defect != "no_root":
        scale = np.power(pdf.astype(f64), 1.0 / V).astype(f32)
    nd = normal.astype(f64)
    nn = np.sqrt(nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1] + nd[:, 2] * nd[:, 2])
    scaled = (nd * scale.astype(f64)[:, None] / nn[:, None]).astype(f32)
    res.n_neigh.ravel()[pix] = n
    res.normal_branch.ravel()[pix] = np.where(pca, BRANCH_PCA, BRANCH_FALLBACK)
    res.rows = np.concatenate([pts, scaled], 1).astype(f32) if N else np.zeros((0, 7), f32)
    return res
