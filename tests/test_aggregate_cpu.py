"""CPU checks of the semi-global aggregation: the numpy mirror against a scalar triple-loop restatement of the
contract, what the aggregation buys on the oracle's volume of the synthetic scene, and the Python binding."""
import numpy as np
import pytest

import mvs_amd
import sgm_mirror
from mvs_amd import synth


def _scalar(vol, cs, z, paths, p1, p2, cap):
    """rules 1-4 one cell at a time, Python integers"""
    D, H, W = vol.shape
    mask = (1 << cs) - 1
    C = [[[0] * W for _ in range(H)] for _ in range(D)]
    seen = [[[False] * W for _ in range(H)] for _ in range(D)]
    for d in range(D):
        for y in range(H):
            for x in range(W):
                cell = int(vol[d, y, x])
                s, n = cell & mask, cell >> cs
                if n == 0:
                    C[d][y][x] = cap
                else:
                    seen[d][y][x] = True
                    C[d][y][x] = min((16 * s) // (255 * n) if cs == 24 else (16 * s) // n, cap)
    S = [[[0] * W for _ in range(H)] for _ in range(D)]
    for dy, dx in sgm_mirror.PATHS[:paths]:
        L = {}
        ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
        xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
        for y in ys:          # p - r is always visited before p in this order
            for x in xs:
                py, px = y - dy, x - dx
                for d in range(D):
                    if not (0 <= py < H and 0 <= px < W):
                        L[(y, x, d)] = C[d][y][x]
                        continue
                    m = min(L[(py, px, k)] for k in range(D))
                    terms = [L[(py, px, d)], m + p2]
                    if d > 0:
                        terms.append(L[(py, px, d - 1)] + p1)
                    if d < D - 1:
                        terms.append(L[(py, px, d + 1)] + p1)
                    L[(y, x, d)] = C[d][y][x] + min(terms) - m
                    assert L[(y, x, d)] <= cap + p2
        for (y, x, d), v in L.items():
            S[d][y][x] += v
    index = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), 1.0, np.float32)
    cost = np.full((H, W), np.inf, np.float32)
    for y in range(H):
        for x in range(W):
            best = None
            for d in range(D):
                if seen[d][y][x] and (best is None or S[d][y][x] < S[best][y][x]):
                    best = d
            if best is not None:
                index[y, x] = best
                depth[y, x] = z[best]
                cost[y, x] = np.float32(S[best][y][x]) / np.float32(16 * paths)
    return np.array(C), np.array(S), depth, cost, index


@pytest.mark.parametrize("cs", [24, 16])
@pytest.mark.parametrize("paths", [4, 8])
def test_mirror_equals_the_scalar_restatement(cs, paths):
    rng = np.random.Generator(np.random.PCG64(0xA66 + cs + paths))
    D, H, W = 4, 5, 6
    n = rng.integers(0, 4, (D, H, W))
    n[:, 2, 3] = 0                      # a pixel nobody sees
    n[1:, 0, 0] = 0                     # a pixel with one seen cell
    per = 255 * 255 if cs == 24 else 255
    s = (rng.integers(0, per + 1, (D, H, W)) * n) // rng.integers(1, 40, (D, H, W))   # mean costs from 0 up to past the cap
    assert (s < (1 << cs)).all()
    vol = ((n << cs) | s).astype(np.uint32)
    z = np.linspace(-0.5, 0.5, D).astype(np.float32)
    p1, p2, cap = 5, 40, 300
    C_ref, S_ref, depth_ref, cost_ref, index_ref = _scalar(vol, cs, z, paths, p1, p2, cap)
    assert (C_ref == cap).any() and (C_ref < cap).any() and (index_ref == -1).any() and (index_ref >= 0).any()
    C = sgm_mirror.cost16(vol, cs, cap)
    np.testing.assert_array_equal(C, C_ref)
    S = sgm_mirror.aggregate(C, paths, p1, p2)
    assert S.dtype == np.uint16
    np.testing.assert_array_equal(S, S_ref)
    depth, cost, index = sgm_mirror.select(S, sgm_mirror.seen_cells(vol, cs), z, paths)
    np.testing.assert_array_equal(index, index_ref)
    np.testing.assert_array_equal(depth, depth_ref)
    np.testing.assert_array_equal(cost, cost_ref)


def bad_share(index, gt, z):
    """share of pixels whose selected plane is more than one plane away from the plane nearest to the ground-truth depth"""
    nearest = np.abs(np.asarray(z, np.float64)[None, None, :] - gt.astype(np.float64)[..., None]).argmin(axis=-1)
    return float(np.mean(np.abs(index - nearest) > 1))


def test_aggregation_halves_the_bad_pixels_of_winner_take_all(oracle):
    """160 x 120, 32 planes over ground truth +- 0.002, 4 views at radius 0.3, fixed sampler; 8 paths, P1 16, P2 128, cap 4080.
    The mirror gives 0.0518 (winner-take-all) and 0.0028 (aggregated): DESIGN.md section 13."""
    W, H, D, V = 160, 120, 32, 4
    main_cam, main_img, side_cams, sides, gt = synth.make_views(W, H, V, radius=0.3)
    z_lo, z_hi = float(gt.min()) - 0.002, float(gt.max()) + 0.002
    _, _, i_wta, vol = oracle.sweep(main_cam, main_img, side_cams, sides, D, z_lo, z_hi, want_volume=True, nthreads=4, sampler="fixed")
    z = oracle.plane_table(D, z_lo, z_hi)
    S = sgm_mirror.aggregate(sgm_mirror.cost16(vol, 24, 4080), 8, 16, 128)
    _, _, i_agg = sgm_mirror.select(S, sgm_mirror.seen_cells(vol, 24), z, 8)
    wta, agg = bad_share(i_wta, gt, z), bad_share(i_agg, gt, z)
    print("bad pixels: winner-take-all %.4f, aggregated %.4f" % (wta, agg))
    assert wta > 0.01, "premise: winner-take-all has bad pixels to remove"
    assert agg <= 0.5 * wta


def test_constants_and_binding():
    assert mvs_amd.MVS_AGGREGATE_REFINE == 1
    lib = mvs_amd.load_library()
    for name in ("mvs_sweep_aggregate", "mvs_sweep_aggregated_device", "mvs_sweep_aggregate_fetch"):
        assert getattr(lib, name).argtypes is not None
    assert lib.mvs_sweep_aggregate(None, 8, 16, 128, 4080, 0) == -1          # MVS_EINVAL for a NULL context, no GPU needed
    assert lib.mvs_sweep_aggregate_fetch(None, None) == -1
    assert lib.mvs_sweep_aggregated_device(None, None) is None
    for name in ("sweep_aggregate", "sweep_aggregate_fetch", "sweep_aggregated_device"):
        assert callable(getattr(mvs_amd.Context, name))
