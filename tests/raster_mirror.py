"""Two references of the rasteriser's contract (oracle/raster_oracle.c, csrc/raster.hip) in plain Python / numpy.  Neither knows of a bounding
box, a tile, a bin or a clipped polygon: every face is tested at every pixel centre of the frame.

exact_render    rational arithmetic, for power-of-two frames and dyadic cameras / vertices.  With such inputs every fma of xform, dop, det and
                of the edge functions is exact in f32 (checked here: an input that is not makes the mirror raise), so coverage, owner and, where
                1 / det is a power of two, z must equal the f32 code bit for bit.  It restates the contract from its text: homogeneous edge
                functions from the cofactors of [x y w], sign normalisation by det, the tie rule on (a, b), -1 <= zn <= 1, nearest zn wins and
                the lower face id wins ties, clear depth 1.0 never replaced by an equal value.
classify        float64 edge functions of f32-rounded vertices for any frame and camera: which pixels are surely inside some face, which are
                impossible for every face, and which are too close to an edge or a depth limit to call."""
from fractions import Fraction

import numpy as np

f32 = np.float32


def soup_of(verts4, faces3):
    """mvs_load_mesh / orc_load_mesh: the dehomogenised triangle soup, divided in f32"""
    v = np.asarray(verts4, f32)
    with np.errstate(all="ignore"):
        xyz = (v[:, :3] / v[:, 3:4]).astype(f32)
    return xyz[np.asarray(faces3, np.int64)].reshape(-1, 9)


def _is_f32(q):
    return Fraction(float(f32(float(q)))) == q


def _need_f32(q, what):
    if not _is_f32(q):
        raise ValueError("exact mirror: %s = %s is not an f32 value; the case is not dyadic enough" % (what, q))
    return q


def exact_face(v9, cam):
    """the contract's face record in rationals: (a[3], b[3], c[3], zp[3], det) with zn(px, py) = (zp[0] px + zp[1] py + zp[2]) / det and
    det > 0, or None for a face the contract drops (a coordinate that is not finite, det == 0)"""
    if not np.all(np.isfinite(v9)):
        return None
    m = [[Fraction(float(e)) for e in row] for row in np.asarray(cam, f32).reshape(4, 4)]
    P = [[Fraction(float(e)) for e in v9[3 * i:3 * i + 3]] for i in range(3)]
    clip = [[_need_f32(r[0] * p[0] + r[1] * p[1] + r[2] * p[2] + r[3], "clip coordinate") for r in m] for p in P]
    x, y, z, w = ([clip[i][k] for i in range(3)] for k in range(4))
    a = [y[1] * w[2] - w[1] * y[2], w[0] * y[2] - y[0] * w[2], y[0] * w[1] - w[0] * y[1]]
    b = [w[1] * x[2] - x[1] * w[2], x[0] * w[2] - w[0] * x[2], w[0] * x[1] - x[0] * w[1]]
    c = [x[1] * y[2] - y[1] * x[2], y[0] * x[2] - x[0] * y[2], x[0] * y[1] - y[0] * x[1]]
    for q in a + b + c:
        _need_f32(q, "edge coefficient")
    det = _need_f32(x[0] * a[0] + y[0] * b[0] + w[0] * c[0], "det")
    if det == 0:
        return None
    if det < 0:
        det, a, b, c = -det, [-q for q in a], [-q for q in b], [-q for q in c]
    zp = [sum(k[i] * z[i] for i in range(3)) for k in (a, b, c)]
    return a, b, c, zp, det


def _pow2_scale(qs):
    d = 1
    for q in qs:
        d = max(d, q.denominator)
    if d & (d - 1):
        raise ValueError("exact mirror: a denominator %d is no power of two" % d)
    return d


def exact_render(soup, cam, W, H):
    """-> owner (H, W) int32 (-1: background), zn (H, W) float64 (1.0: background; the exact rational rounded once), hits (H, W) int32: how
    many faces produce a fragment at the pixel.  Rows top-down, pixel centres ((2 col + 1) / W - 1, 1 - (2 row + 1) / H)."""
    if W & (W - 1) or H & (H - 1):
        raise ValueError("exact mirror: frame %d x %d is no power of two" % (W, H))
    # integer pixel coordinates: px = X / W, py = Y / H
    X = (2 * np.arange(W, dtype=np.int64) + 1 - W)[None, :]
    Y = (H - 2 * np.arange(H, dtype=np.int64) - 1)[:, None]
    owner = np.full((H, W), -1, np.int32)
    hits = np.zeros((H, W), np.int32)
    best_n = np.ones((H, W), object)       # best zn as numerator / denominator of Python integers: compared exactly
    best_d = np.ones((H, W), object)
    best_n[:] = 1
    best_d[:] = 1
    for f in range(soup.shape[0]):
        rec = exact_face(soup[f], cam)
        if rec is None:
            continue
        a, b, c, zp, det = rec
        s = _pow2_scale(a + b + c + zp + [det])
        inside = np.ones((H, W), bool)
        for i in range(3):
            ai, bi, ci = int(a[i] * s), int(b[i] * s), int(c[i] * s)
            # e W H s = a X H + b Y W + c W H, every partial sum of the f32 code's fma chain an f32 value: |.| < 2^24 units of 1 / (s W H)
            inner = bi * Y * W + ci * W * H
            e = ai * X * H + inner
            if np.abs(inner).max() >= (1 << 24) * _gran(bi * W, ci * W * H) or np.abs(e).max() >= (1 << 24) * _gran(ai * H, bi * W, ci * W * H):
                raise ValueError("exact mirror: an edge function of face %d needs more than 24 bits" % f)
            inside &= (e > 0) | ((e == 0) & ((ai > 0) or (ai == 0 and bi > 0)))
        zn_num = (int(zp[0] * s) * X * H + int(zp[1] * s) * Y * W + int(zp[2] * s) * W * H).astype(object)   # zn = zn_num / zn_den
        zn_den = int(det * s) * W * H
        inside &= (zn_num >= -zn_den) & (zn_num <= zn_den)
        hits += inside
        # GL_LESS in submission order: strictly nearer than what is there (the clear value 1.0 included)
        nearer = inside & (zn_num * best_d < best_n * zn_den)
        owner[nearer] = f
        best_n[nearer] = zn_num[nearer]
        best_d[nearer] = zn_den
    zn = np.ones((H, W), np.float64)
    cov = owner >= 0
    zn[cov] = [float(Fraction(int(n), int(d))) for n, d in zip(best_n[cov], best_d[cov])]
    return owner, zn, hits


def _gran(*ints):
    """the largest power of two dividing every non-zero integer given (the unit the sums are multiples of)"""
    g = 0
    for v in ints:
        g |= abs(int(v))
    return (g & -g) if g else 1


def classify(soup, cam, W, H, eps=1e-4, chunk=64):
    """-> sure (H, W) bool: the pixel is surely a fragment of some face; possible (H, W) bool: it is not impossible for every face.
    Per face and edge: surely inside when e > eps (|a| + |b| + |c|), impossible when e < -eps (...); zn surely in range inside
    (-1 + eps, 1 - eps), impossible outside [-1 - eps, 1 + eps].  A face with det == 0 or a non-finite coordinate draws nothing."""
    m = np.asarray(cam, f32).reshape(4, 4).astype(np.float64)
    v = np.asarray(soup, f32).astype(np.float64).reshape(-1, 3, 3)
    px = ((2.0 * np.arange(W) + 1.0) / W - 1.0)[None, None, :]
    py = (1.0 - (2.0 * np.arange(H) + 1.0) / H)[None, :, None]
    sure = np.zeros((H, W), bool)
    possible = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        clip = np.einsum("kj,fij->fik", m[:, :3], v) + m[:, 3]                     # (F, 3 vertices, 4)
        x, y, z, w = (clip[..., k] for k in range(4))
        i1, i2 = [1, 2, 0], [2, 0, 1]
        a = y[:, i1] * w[:, i2] - w[:, i1] * y[:, i2]
        b = w[:, i1] * x[:, i2] - x[:, i1] * w[:, i2]
        c = x[:, i1] * y[:, i2] - y[:, i1] * x[:, i2]
        det = (x * a + y * b + w * c)[:, 0]
        ok = np.isfinite(det) & (det != 0) & np.isfinite(clip).all((1, 2))
        sgn = np.where(det < 0, -1.0, 1.0)[:, None]
        a, b, c, det = a * sgn, b * sgn, c * sgn, np.abs(det)
        zp = np.stack([(k * z).sum(1) for k in (a, b, c)], 1) / det[:, None]
    for f0 in range(0, v.shape[0], chunk):
        sel = np.nonzero(ok[f0:f0 + chunk])[0] + f0
        if not len(sel):
            continue
        s_in = np.ones((len(sel), H, W), bool)
        s_out = np.zeros((len(sel), H, W), bool)
        for i in range(3):
            ai, bi, ci = (k[sel, i][:, None, None] for k in (a, b, c))
            e = ai * px + bi * py + ci
            thr = eps * (np.abs(ai) + np.abs(bi) + np.abs(ci))
            s_in &= e > thr
            s_out |= e < -thr
        zn = zp[sel, 0][:, None, None] * px + zp[sel, 1][:, None, None] * py + zp[sel, 2][:, None, None]
        s_in &= (zn > -1.0 + eps) & (zn < 1.0 - eps)
        s_out |= (zn < -1.0 - eps) | (zn > 1.0 + eps)
        sure |= s_in.any(0)
        possible |= (~s_out).any(0)
    return sure, possible


def mip_chain(frame):
    """the u8 levels of the frame texture's mip chain as the contract states them (oracle/raster_oracle.c: mip_build): level l has
    max(1, w >> 1) x max(1, h >> 1) texels, each (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2 i, 2 j) with indices clamped to the parent"""
    levels = [np.asarray(frame, np.uint8)]
    while levels[-1].shape != (1, 1):
        p = levels[-1].astype(np.int64)
        ph, pw = p.shape
        h, w = max(1, ph >> 1), max(1, pw >> 1)
        r0, r1 = np.minimum(2 * np.arange(h), ph - 1), np.minimum(2 * np.arange(h) + 1, ph - 1)
        c0, c1 = np.minimum(2 * np.arange(w), pw - 1), np.minimum(2 * np.arange(w) + 1, pw - 1)
        s = p[r0][:, c0] + p[r0][:, c1] + p[r1][:, c0] + p[r1][:, c1]
        levels.append(((s + 2) >> 2).astype(np.uint8))
    return levels
