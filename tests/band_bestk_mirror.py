"""Restatement of the band sweep with windowed costs (mvs_sweep_run_band_bestk), written from the contract and
not from the kernel.  It is the arbiter: the device's cells must be bit-identical to volume().

Planes are band_mirror.planes (z = prior + offset in one float32 add, live where the pixel has a prior and the sum is inside (-1, 1)).
The ZNCC cost of a (plane, view) goes through oracle.warp_by_depth on the PER-PIXEL plane map, so every pixel -- every window member -- is
sampled at its own plane; a dead pixel is given depth 1.0, which that function reads as "no depth" (ok = 0).  Rules 2-4 are then
zncc_mirror.view_cost.  The absolute difference takes e and ok of every pixel from band_mirror.band_volume over that one view (a one-view
cell is ok << 24 | e) and means e over the window's members with zncc_mirror.box and an integer division.  The merge is
bestk_mirror.merge.  brute_cell does one cell with loops and the oracle's single-sample entry and shares nothing with the array path.
Selection and refinement on the volume are oracle.argmin / oracle.refine_depth(..., sampler="fixed") with the offsets as the plane table,
the absolute map band_mirror.resolve."""
import numpy as np

import band_mirror as bm
import bestk_mirror as km
import zncc_mirror as zm

COST_ABSDIFF, COST_ZNCC, KEEP_ALL = km.COST_ABSDIFF, km.COST_ZNCC, km.KEEP_ALL
NO_DEPTH = np.float32(1.0)


def warped(oracle, main_cam, side_cam, frame, z, live):
    """rule 2 for ZNCC on one plane map z [H, W] -> (B uint8, ok bool)"""
    frame = np.asarray(frame, np.uint8)
    with np.errstate(invalid="ignore"):
        depth = np.where(live, z, NO_DEPTH).astype(np.float32)
    assert not (depth[live] == NO_DEPTH).any()
    out = oracle.warp_by_depth(main_cam, depth, side_cam, frame, sampler="fixed")
    ok = out[..., 1] != 0
    assert not ok[~live].any()
    return out[..., 0], ok


def zncc_view_costs(oracle, main_cam, main_img, side_cam, frame, prior, offsets, r):
    assert 1 <= r <= 4
    z, live = bm.planes(prior, offsets)
    parts = []
    for d in range(len(z)):
        B, ok = warped(oracle, main_cam, side_cam, frame, z[d], live[d])
        parts.append(zm.view_cost(main_img, B, ok, r))
    return tuple(np.stack(a) for a in zip(*parts))


def absdiff_view_costs(oracle, main_cam, main_img, side_cam, frame, prior, offsets, r):
    assert 0 <= r <= 4
    one = bm.band_volume(oracle, main_cam, main_img, np.asarray(side_cam, np.float32)[None], [frame], prior, offsets)
    ok, e = (one >> 24).astype(np.int64), (one & 0xffffff).astype(np.int64)
    assert ok.max(initial=0) <= 1 and (e[ok == 0] == 0).all() and e.max(initial=0) <= 65025
    N = np.stack([zm.box(m, r) for m in ok])
    S = np.stack([zm.box(x, r) for x in e])
    assert S.max(initial=0) < 2 ** 23
    c = S // np.maximum(N, 1)
    return ok != 0, np.where(ok != 0, c, 0).astype(np.uint32)


def view_costs(oracle, cost, main_cam, main_img, side_cam, frame, prior, offsets, r):
    """(counted, c) of one view, [D, H, W] each"""
    if cost == COST_ZNCC:
        return zncc_view_costs(oracle, main_cam, main_img, side_cam, frame, prior, offsets, r)
    assert cost == COST_ABSDIFF
    return absdiff_view_costs(oracle, main_cam, main_img, side_cam, frame, prior, offsets, r)


def volume(oracle, cost, main_cam, main_img, side_cams, side_imgs, prior, offsets, r, keep, views=None):
    """the packed volume [D, H, W] uint32 of mvs_sweep_run_band_bestk over the side views `views` (default: all)"""
    views = range(len(side_imgs)) if views is None else views
    per_view = [view_costs(oracle, cost, main_cam, main_img, side_cams[v], side_imgs[v], prior, offsets, r) for v in views]
    return km.merge(per_view, keep, (len(offsets),) + np.asarray(main_img).shape)


def level(oracle, cost, main_cam, main_img, side_cams, side_imgs, prior, offsets, r, keep):
    """one band level -> (absolute depth, volume, (offset, cost, index)): fused selection, refinement, resolve"""
    vol = volume(oracle, cost, main_cam, main_img, side_cams, side_imgs, prior, offsets, r, keep)
    _, cmap, index = oracle.argmin(vol, offsets, sampler="fixed")
    offset = oracle.refine_depth(vol, offsets, index, sampler="fixed")
    return bm.resolve(prior, offset, index), vol, (offset, cmap, index)


def brute_view_cost(oracle, cost, main_cam, main_img, side_cam, frame, prior, offset, r, row, col):
    """the per-view cost at one cell with loops and scalars -> (members, counted, c)"""
    H, W = main_img.shape
    q = oracle.view_matrix(main_cam, side_cam, W, H)
    pad = oracle.pad_image(np.asarray(frame, np.uint8))
    B, ok = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    for y in range(row - r, row + r + 1):
        for x in range(col - r, col + r + 1):
            if not (0 <= y < H and 0 <= x < W):
                continue
            z0 = np.float32(prior[y, x])
            if not -1.0 < float(z0) < 1.0:           # no prior (false for NaN)
                continue
            z = z0 + np.float32(offset)
            assert type(z) is np.float32
            if not -1.0 < float(z) < 1.0:            # a dead plane
                continue
            good, dot = oracle.sweep_sample_fx(q, oracle.lib.orc_pixel_xn(x, W), oracle.lib.orc_pixel_yn(y, H), float(z), pad)
            if good:
                ok[y, x], B[y, x] = True, int(dot)
    members = int(ok.sum())
    if cost == COST_ZNCC:
        return (members,) + tuple(zm.brute_cell(main_img, (B + 127) // 255, ok, r, row, col)[1:])
    if not ok[row, col]:
        return members, False, 0
    e = [abs(int(B[y, x]) - 255 * int(main_img[y, x])) for y, x in zip(*np.nonzero(ok))]
    return members, True, sum(e) // len(e)


def brute_cell(oracle, cost, main_cam, main_img, side_cams, side_imgs, prior, offset, r, keep, row, col, views=None):
    """the cell of offset `offset` at (row, col) -> (n, per-view costs of the counted views in view order, the packed cell)"""
    views = range(len(side_imgs)) if views is None else views
    costs = []
    for v in views:
        _, counted, c = brute_view_cost(oracle, cost, main_cam, main_img, side_cams[v], side_imgs[v], prior, offset, r, row, col)
        if counted:
            costs.append(int(c))
    best = sorted(costs)
    if keep != KEEP_ALL:
        best = best[:keep]
    return len(costs), costs, (len(best) << 24) | sum(best)
