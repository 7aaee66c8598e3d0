"""Restatement of the band sweep, written from the contract and not from the kernel.  It is the arbiter:
mvs_sweep_run_band must be bit-identical to band_volume(), mvs_sweep_band_resolve to resolve() and report().

Rules 1-3 a sample at a time: the sample is the oracle's orc_sweep_sample_fx (the C function behind oracle.sweep_sample_fx, bound once
here because a volume takes up to a million calls), the view matrix oracle.view_matrix, the frame oracle.pad_image, and the plane
z = np.float32(z0) + offsets[d], one float32 add.  Selection and refinement on the volume are oracle.argmin(..., sampler="fixed") and
oracle.refine_depth with the offsets as the plane table."""
import ctypes as C

import numpy as np

BACKGROUND_DEPTH = np.float32(1.0)
_fp, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def inside(z):
    """-1 < z < 1 (fusion rule 1; false for NaN)"""
    with np.errstate(invalid="ignore"):
        return (z > -1.0) & (z < 1.0)


def planes(prior, offsets):
    """-> (z [D, H, W] float32 = prior + offsets[d] in one add, live [D, H, W] bool: the pixel has a prior and the plane is inside)"""
    prior = np.asarray(prior, np.float32)
    offsets = np.asarray(offsets, np.float32)
    with np.errstate(invalid="ignore"):
        z = prior[None] + offsets[:, None, None]
    assert z.dtype == np.float32
    return z, inside(prior)[None] & inside(z)


def band_volume(oracle, main_cam, main_img, side_cams, side_imgs, prior, offsets, views=None):
    """the packed volume [D, H, W] uint32 of the band sweep over the side views `views` (default: all)"""
    main_img = np.asarray(main_img, np.uint8)
    H, W = main_img.shape
    views = range(len(side_imgs)) if views is None else views
    z, live = planes(prior, offsets)
    rows, cols = np.nonzero(live)[1:]
    xn = [oracle.lib.orc_pixel_xn(c, W) for c in range(W)]
    yn = [oracle.lib.orc_pixel_yn(r, H) for r in range(H)]
    xs, ys, zs = [xn[c] for c in cols], [yn[r] for r in rows], z[live].tolist()
    im255 = (255 * main_img.astype(np.int64))[rows, cols].tolist()
    cells = [0] * len(zs)
    sample = oracle.lib.orc_sweep_sample_fx
    sample.argtypes = [_fp, C.c_float, C.c_float, C.c_float, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    sample.restype = C.c_int
    dot = C.c_int(0)
    dot_ref = C.byref(dot)
    for v in views:
        q = np.ascontiguousarray(oracle.view_matrix(main_cam, side_cams[v], W, H), np.float32)
        pad = np.ascontiguousarray(oracle.pad_image(np.asarray(side_imgs[v], np.uint8)))
        qp, pp, pitch = q.ctypes.data_as(_fp), pad.ctypes.data_as(_u8p), pad.shape[1]
        for i in range(len(zs)):
            if sample(qp, xs[i], ys[i], zs[i], pp, pitch, W, H, dot_ref):
                cells[i] += (1 << 24) + abs(dot.value - im255[i])
    vol = np.zeros(live.shape, np.uint32)
    vol[live] = cells
    return vol


def resolve(prior, offset_map, index):
    """rule 5: prior + offset (one float32 add) where there is an index and the sum is inside (-1, 1), else the background depth"""
    prior, offset_map = np.asarray(prior, np.float32), np.asarray(offset_map, np.float32)
    with np.errstate(invalid="ignore"):
        z = prior + offset_map
    return np.where((np.asarray(index) >= 0) & inside(z), z, BACKGROUND_DEPTH).astype(np.float32)


def report(prior, offset_map, index, D):
    """[pixels with a prior, with an index, with index 0 or D - 1, emptied by the range test]"""
    index = np.asarray(index)
    have = index >= 0
    kept = resolve(prior, offset_map, index) != BACKGROUND_DEPTH     # (an absolute depth inside (-1, 1) never is the background depth)
    return [int(inside(np.asarray(prior, np.float32)).sum()), int(have.sum()), int((have & ((index == 0) | (index == D - 1))).sum()), int((have & ~kept).sum())]
