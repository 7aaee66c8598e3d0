"""Restatement of the occlusion-robust sweep (mvs_sweep_run_bestk), written from the contract and not from the
kernel.  It is the arbiter: the device's cells must be bit-identical to volume().

Per-view costs: the ZNCC cost is zncc_mirror.view_volume's (rules 1-4 of section 21); the absolute difference takes e and ok of every
pixel from the oracle's fixed-sampler sweep over that one view (a one-view packed cell is ok << 24 | e) and means e over the window's
members with zncc_mirror.box on int64 and an integer division.  The merge is np.sort over the view axis.  brute_cell does all of it at one
cell with loops and Python integers, the absolute difference's sample through the oracle's single-sample entry, and shares nothing with
the array path.  Selection and refinement on the volume are oracle.argmin / oracle.refine_depth(..., sampler="fixed")."""
import numpy as np

import zncc_mirror as zm

COST_ABSDIFF, COST_ZNCC, KEEP_ALL = 0, 1, 0
NONE = np.int64(1) << 40        # the cost of a view that does not count, in the sort: above every cost


def absdiff_view_volume(oracle, main_cam, main_img, side_cam, frame, D, z_lo, z_hi, r):
    """one view over the D planes of [z_lo, z_hi] -> (counted [D, H, W] bool: ok of the centre, c [D, H, W] uint32, 0 where not counted)"""
    assert 0 <= r <= 4
    one = oracle.sweep(main_cam, main_img, np.asarray(side_cam, np.float32)[None], [frame], D, z_lo, z_hi, want_volume=True, sampler="fixed")[3]
    ok, e = (one >> 24).astype(np.int64), (one & 0xffffff).astype(np.int64)
    assert ok.max(initial=0) <= 1 and (e[ok == 0] == 0).all() and e.max(initial=0) <= 65025
    N = np.stack([zm.box(m, r) for m in ok])
    S = np.stack([zm.box(x, r) for x in e])          # (e is 0 wherever ok is)
    assert S.max(initial=0) < 2 ** 23
    c = S // np.maximum(N, 1)
    return ok != 0, np.where(ok != 0, c, 0).astype(np.uint32)


def view_costs(oracle, cost, main_cam, main_img, side_cam, frame, D, z_lo, z_hi, r):
    """(counted, c) of one view, [D, H, W] each"""
    if cost == COST_ZNCC:
        return zm.view_volume(oracle, main_cam, main_img, side_cam, frame, oracle.plane_table(D, z_lo, z_hi), r)[1:]
    assert cost == COST_ABSDIFF
    return absdiff_view_volume(oracle, main_cam, main_img, side_cam, frame, D, z_lo, z_hi, r)


def merge(per_view, keep, shape=None):
    """the cell rule: per_view a sequence of (counted, c) -> the packed volume k << 24 | the sum of the k smallest c, k = min(keep, n)"""
    assert keep == KEEP_ALL or 1 <= keep <= 8
    if len(per_view) == 0:
        return np.zeros(shape, np.uint32)
    counted = np.stack([p[0] for p in per_view])
    c = np.where(counted, np.stack([p[1] for p in per_view]).astype(np.int64), NONE)
    c = np.sort(c, axis=0)
    n = counted.sum(0)
    k = n if keep == KEEP_ALL else np.minimum(keep, n)
    c = np.where(c == NONE, 0, c)
    total = (c if keep == KEEP_ALL else c[:keep]).sum(0)
    assert total.max(initial=0) < 2 ** 24 and k.max(initial=0) < 256
    return ((k.astype(np.int64) << 24) | total).astype(np.uint32)


def volume(oracle, cost, main_cam, main_img, side_cams, side_imgs, D, z_lo, z_hi, r, keep, views=None):
    """the packed volume [D, H, W] uint32 of mvs_sweep_run_bestk over the side views `views` (default: all)"""
    views = range(len(side_imgs)) if views is None else views
    per_view = [view_costs(oracle, cost, main_cam, main_img, side_cams[v], side_imgs[v], D, z_lo, z_hi, r) for v in views]
    return merge(per_view, keep, (D,) + np.asarray(main_img).shape)


def brute_view_cost(oracle, cost, main_cam, main_img, side_cam, frame, z, r, row, col):
    """the per-view cost at one cell with loops and scalars -> (counted, c)"""
    H, W = main_img.shape
    if cost == COST_ZNCC:
        B, ok = zm.warped(oracle, main_cam, side_cam, frame, z)
        return zm.brute_cell(main_img, B, ok, r, row, col)[1:]
    q = oracle.view_matrix(main_cam, side_cam, W, H)
    pad = oracle.pad_image(np.asarray(frame, np.uint8))
    members, centre = [], False
    for y in range(row - r, row + r + 1):
        for x in range(col - r, col + r + 1):
            if not (0 <= y < H and 0 <= x < W):
                continue
            ok, dot = oracle.sweep_sample_fx(q, oracle.lib.orc_pixel_xn(x, W), oracle.lib.orc_pixel_yn(y, H), float(z), pad)
            if ok:
                members.append(abs(int(dot) - 255 * int(main_img[y, x])))
                centre = centre or (y, x) == (row, col)
    if not centre:
        return False, 0
    return True, sum(members) // len(members)


def brute_cell(oracle, cost, main_cam, main_img, side_cams, side_imgs, z, r, keep, row, col, views=None):
    """the cell of plane depth z at (row, col) -> (n, per-view costs of the counted views in view order, the packed cell)"""
    views = range(len(side_imgs)) if views is None else views
    costs = []
    for v in views:
        counted, c = brute_view_cost(oracle, cost, main_cam, main_img, side_cams[v], side_imgs[v], z, r, row, col)
        if counted:
            costs.append(int(c))
    best = sorted(costs)
    if keep != KEEP_ALL:
        best = best[:keep]
    return len(costs), costs, (len(best) << 24) | sum(best)
