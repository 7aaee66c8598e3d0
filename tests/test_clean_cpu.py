"""CPU checks of the map cleaning: the numpy mirror (tests/clean_mirror.py) against a scalar restatement of the
contract, the premises of the crafted maps and volumes that tests/test_clean_gpu.py gives to the kernels (tests/clean_maps.py), what the
cleaning buys on the oracle's volume of the synthetic scene, and the Python binding."""
import collections
import ctypes

import numpy as np
import pytest

import clean_maps
import clean_mirror
import mvs_amd
import sgm_mirror
from mvs_amd import synth
from test_aggregate_cpu import bad_share


# ---- the mirror against one pixel at a time ---------------------------------------------------------------------------------------
def _scalar(index, vol, cs, S, min_views, u, min_size, max_diff):
    """the contract in Python integers -> (index after, report, sizes)"""
    D, H, W = vol.shape
    mask = (1 << cs) - 1
    report = [0, 0, 0, 0]
    mid = [[int(index[y, x]) for x in range(W)] for y in range(H)]
    for y in range(H):
        for x in range(W):
            i = int(index[y, x])
            if i < 0:
                continue
            report[0] += 1
            ci = int(vol[i, y, x])
            n_i, s_i = ci >> cs, ci & mask
            if n_i < min_views:
                report[1] += 1
                mid[y][x] = -1
                continue
            if u == 0:
                continue
            for d in range(D):
                cd = int(vol[d, y, x])
                n_d, s_d = cd >> cs, cd & mask
                if abs(d - i) < 2 or n_d == 0:
                    continue
                if S is not None:
                    rival = int(S[d, y, x]) * (100 - u) < int(S[i, y, x]) * 100
                else:
                    rival = s_d * n_i * (100 - u) < s_i * n_d * 100
                if rival:
                    report[2] += 1
                    mid[y][x] = -1
                    break
    sizes = [[0] * W for _ in range(H)]
    if min_size:
        seen = [[False] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                if mid[y][x] < 0 or seen[y][x]:
                    continue
                queue, members = collections.deque([(y, x)]), []
                seen[y][x] = True
                while queue:
                    cy, cx = queue.popleft()
                    members.append((cy, cx))
                    for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                        if 0 <= ny < H and 0 <= nx < W and not seen[ny][nx] and mid[ny][nx] >= 0 and abs(mid[ny][nx] - mid[cy][cx]) <= max_diff:
                            seen[ny][nx] = True
                            queue.append((ny, nx))
                for cy, cx in members:
                    sizes[cy][cx] = len(members)
    out = [row[:] for row in mid]
    for y in range(H):
        for x in range(W):
            if 0 < sizes[y][x] < min_size:
                report[3] += 1
                out[y][x] = -1
    return np.array(out, np.int32), report, np.array(sizes, np.int32)


def _random_case(cs, seed):
    """24 x 17 x 6: i.i.d. cells with counts 0..3, an index map of blocks and noise, and four crafted pixels (u = 10)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    W, H, D = 24, 17, 6
    per = clean_maps.PER[cs]
    n = rng.integers(0, 4, (D, H, W))
    s = (rng.integers(0, per + 1, (D, H, W)) * n) // rng.integers(1, 6, (D, H, W))
    index = (rng.integers(0, D, (H // 4 + 1, W // 4 + 1)).repeat(4, 0).repeat(4, 1)[:H, :W] + (rng.random((H, W)) < 0.15)) % D
    index[rng.random((H, W)) < 0.12] = -1
    S = rng.integers(0, 65536, (D, H, W))
    # the right half: winners with sum 0 and S 0, which nothing undercuts, seen by 1..3 views (mostly 2 or 3): components survive rules 1-2
    for y in range(H):
        for x in range(W // 2, W):
            if index[y, x] >= 0:
                n[index[y, x], y, x], s[index[y, x], y, x], S[index[y, x], y, x] = rng.choice([1, 2, 2, 3, 3, 3]), 0, 0

    def craft(y, x, i, n_i, s_i, S_i, others):
        index[y, x] = i
        n[:, y, x], s[:, y, x], S[:, y, x] = 0, 0, 0
        n[i, y, x], s[i, y, x], S[i, y, x] = n_i, s_i, S_i
        for d, (n_d, s_d, S_d) in others.items():
            n[d, y, x], s[d, y, x], S[d, y, x] = n_d, s_d, S_d

    craft(0, 0, 2, 2, 180, 900, {3: (1, 0, 0), 1: (3, 0, 0)})    # far better cells, but one plane away on either side: no rivals
    craft(0, 1, 2, 2, 180, 900, {4: (1, 99, 999)})               # two planes away: 99 * 2 * 90 < 180 * 1 * 100, 999 * 90 < 900 * 100
    craft(0, 2, 2, 2, 180, 900, {4: (1, 100, 1000)})             # equal products: no rival
    craft(0, 3, 2, 1, 90, 900, {0: (1, 0, 0)})                   # one view, and a rival two planes away: rule 1 takes it
    return index.astype(np.int32), clean_maps._pack(n, s, cs), S.astype(np.uint16)


RULES = {"rule 1": (2, 0, 0, 1), "rule 2": (0, 10, 0, 1), "rule 3": (0, 0, 4, 1), "rule 3, diff 0": (0, 0, 6, 0), "all": (2, 10, 4, 1), "none": (0, 0, 0, 1)}


@pytest.mark.parametrize("cs", [24, 16])
@pytest.mark.parametrize("aggregated", [False, True])
@pytest.mark.parametrize("rules", list(RULES))
def test_mirror_equals_the_scalar_restatement(cs, aggregated, rules):
    index, vol, S = _random_case(cs, 0xC1EA + cs)
    min_views, u, min_size, max_diff = RULES[rules]
    depth = np.linspace(-0.5, 0.5, index.size, dtype=np.float32).reshape(index.shape)
    cost = np.arange(index.size, dtype=np.float32).reshape(index.shape)
    i_ref, report_ref, sizes_ref = _scalar(index, vol, cs, S if aggregated else None, min_views, u, min_size, max_diff)
    d, c, i, report, sizes = clean_mirror.clean(depth, cost, index, vol, cs, S if aggregated else None, min_views, u, min_size, max_diff)
    np.testing.assert_array_equal(i, i_ref)
    assert report == report_ref
    if min_size:
        np.testing.assert_array_equal(sizes, sizes_ref)
        assert sizes.max() >= min_size > sizes[sizes > 0].min(), "premise: components on both sides of the threshold"
    else:
        assert sizes is None
    kept, gone = i >= 0, (index >= 0) & (i < 0)
    assert d[~gone].tobytes() == depth[~gone].tobytes() and c[~gone].tobytes() == cost[~gone].tobytes() and (i[~gone] == index[~gone]).all()
    assert gone.sum() == sum(report[1:]) and (d[gone] == np.float32(1.0)).all() and np.isposinf(c[gone]).all()
    if rules == "none":
        assert report == [int((index >= 0).sum()), 0, 0, 0] and (i == index).all()
    if rules == "rule 2":
        assert i[0, 0] == 2, "a rival one plane away counted"
        assert i[0, 1] == -1, "a rival two planes away did not count"
        assert i[0, 2] == 2, "equal products counted as a rival"
        assert i[0, 3] == -1 and report[1] == 0
    if rules == "all":
        # pixel (0, 3) fails both rules: with rule 2 alone it goes under rule 2, with both under rule 1 and only there
        _, _, _, alone, _ = clean_mirror.clean(depth, cost, index, vol, cs, S if aggregated else None, 0, u, 0, 1)
        both = clean_mirror.rule1(index, vol, cs, min_views) & clean_mirror.rule2(index, vol, cs, u, S if aggregated else None)
        assert both[0, 3] and both.sum() >= 1
        assert report[2] == alone[2] - int(both.sum()) and report[0] == alone[0]
    # a second pass with the same parameters rejects nothing
    again = clean_mirror.clean(d, c, i, vol, cs, S if aggregated else None, min_views, u, min_size, max_diff)
    assert again[3] == [int(kept.sum()), 0, 0, 0] and (again[2] == i).all()


# ---- the crafted maps hold what they are for ---------------------------------------------------------------------------------------
SHAPE, SMALL, LARGE = (203, 77), (21, 5), (640, 480)


def _simple_path(m):
    """every pixel with an index has one or two such 4-neighbours, and exactly two have one: a single open path if it is connected"""
    v = np.pad(m >= 0, 1)
    nb = (v[:-2, 1:-1].astype(int) + v[2:, 1:-1] + v[1:-1, :-2] + v[1:-1, 2:])[m >= 0]
    return set(np.unique(nb)) == {1, 2} and int((nb == 1).sum()) == 2


def test_constant_and_checkerboard():
    for W, H in (SHAPE, SMALL):
        assert (clean_mirror.component_sizes(clean_maps.constant(W, H), 0) == W * H).all()
    for max_diff in (0, 1, 3):
        m = clean_maps.checkerboard(*SHAPE, max_diff)
        assert set(np.unique(m)) == {0, max_diff + 1} and m.max() < clean_maps.D_MAPS
        assert (clean_mirror.component_sizes(m, max_diff) == 1).all()
        assert (clean_mirror.component_sizes(m, max_diff + 1) == m.size).all()


@pytest.mark.parametrize("gen", ["serpentine", "spiral"])
@pytest.mark.parametrize("shape", [SHAPE, LARGE])
def test_paths_are_single_components_of_known_length(gen, shape):
    m, length = getattr(clean_maps, gen)(*shape)
    W, H = shape
    assert m.shape == (H, W) and int((m >= 0).sum()) == length and _simple_path(m)
    assert length > (0.45 if gen == "spiral" else 0.5) * W * H and 0 <= m.max() < clean_maps.D_MAPS and len(np.unique(m)) == 9
    sizes = clean_mirror.component_sizes(m, 1)
    assert (sizes[m >= 0] == length).all() and (sizes[m < 0] == 0).all()
    assert clean_mirror.component_sizes(m, 0).max() == 3, "with max_diff 0 the path falls into its runs of three equal planes"
    ys, xs = np.nonzero(m >= 0)
    assert ys.min() == 0 and xs.min() == 0 and xs.max() == W - 1 and ys.max() >= H - 2   # the path visits every tile


def test_ramp():
    m = clean_maps.ramp(*SHAPE)
    W, H = SHAPE
    assert m.max() == 7 and (clean_mirror.component_sizes(m, 1) == W * H).all()
    sizes = clean_mirror.component_sizes(m, 0)
    assert (sizes[:, :182] == 26 * H).all() and (sizes[:, 182:] == (W - 182) * H).all()


def test_threshold_squares():
    m, want = clean_maps.threshold_squares(*SHAPE)
    sizes = clean_mirror.component_sizes(m, 1)
    assert sorted(want.values()) == [15] * 4 + [16] * 4 + [17] * 4
    for tile, corners in clean_maps.SQUARE_CORNERS.items():
        for cx, cy in corners:
            assert cx % tile == 0 and cy % tile == 0 and (cx % (2 * tile) or cy % (2 * tile) or tile == 64)
            assert (m[cy - 1:cy + 1, cx - 1:cx + 1] >= 0).all(), "the component has a pixel in each of the four tiles"
            assert (sizes[cy - 1:cy + 1, cx - 1:cx + 1] == want[(cx, cy)]).all()
    assert int((m >= 0).sum()) == sum(want.values())
    _, _, i, report, _ = clean_mirror.clean(np.zeros(m.shape, np.float32), np.zeros(m.shape, np.float32), m, speckle_min_size=16)
    assert report == [16 * 12, 0, 0, 15 * 4] and int((i >= 0).sum()) == (16 + 17) * 4


@pytest.mark.parametrize("name,seed,planes,weights", clean_maps.PERCOLATION)
def test_percolation_noise(name, seed, planes, weights):
    W, H = clean_maps.PERCOLATION_SHAPE
    m = clean_maps.percolation(W, H, seed, planes, weights)
    assert 0.58 < (m >= 0).mean() < 0.62 and set(np.unique(m)) == {-1, *planes}
    sizes = clean_mirror.component_sizes(m, 1)
    distinct = np.unique(sizes[sizes > 0])
    assert distinct[0] == 1 and len(distinct) >= 20
    largest = sizes == sizes.max()
    ys, xs = np.nonzero(largest)
    print("%s: %d distinct sizes, largest %d pixels, its box %d x %d" % (name, len(distinct), sizes.max(), np.ptp(xs) + 1, np.ptp(ys) + 1))
    assert np.ptp(xs) + 1 >= 193 and np.ptp(ys) + 1 >= 65


@pytest.mark.parametrize("cs", [24, 16])
def test_volume_for_selects_the_wanted_map(cs):
    m = clean_maps.percolation(70, 5, 3, (0, 2, 7))
    vol = clean_maps.volume_for(m, clean_maps.D_MAPS, cs)
    seen = sgm_mirror.seen_cells(vol, cs)
    s, n = sgm_mirror.split(vol, cs)
    # winner-take-all: the smallest mean cost among the seen cells, as exact rationals s / n (the wanted cell has 0, every other more)
    assert (seen.any(axis=0) == (m >= 0)).all()
    assert (np.where(seen, s, 1 << 40).argmin(axis=0)[m >= 0] == m[m >= 0]).all() and ((s == 0) & seen).sum() == (m >= 0).sum()
    assert (n[:, m >= 0].max() == 3) and (s <= clean_maps.PER[cs] * n).all()


@pytest.mark.parametrize("cs", [24, 16])
@pytest.mark.parametrize("W,H,D", [(70, 5, 11), (129, 6, 65)])
def test_rules_case_straddles_the_inequalities(W, H, D, cs):
    index, vol, S, kind = clean_maps.rules_case(W, H, D, cs, 0x12 + D)
    u = clean_maps.UNIQUENESS
    s, n = clean_mirror.split(vol, cs)
    assert (s <= clean_maps.PER[cs] * n).all(), "a sum no sweep can produce"
    own = clean_mirror._at(n, index)
    for count in range(4):
        assert ((own == count) & (kind >= 0)).any(), "no crafted winner with count %d" % count
    for flag, scores in ((False, None), (True, S)):
        r2 = clean_mirror.rule2(index, vol, cs, u, scores)
        for k, fires in ((0, False), (1, False), (2, False), (3, True), (4, True), (5, True), (6, False)):
            at = (kind == k) & ((own > 0) | flag)      # a winner nobody sees has sum 0: nothing lies below it; its S is as good as any
            assert at.any() and (r2[at] == fires).all(), "%s, aggregated %s: %s" % (clean_maps.KINDS[k], flag, r2[at])
        both = clean_mirror.rule1(index, vol, cs, 2) & r2
        assert both[kind == 7].all() and (kind == 7).any()
        assert r2[kind < 0].any() and not r2[kind < 0].all()
    # one unit: the equal pairs and the pairs below differ by 1 in s_d (and in S_d)
    for k_eq, k_below in ((2, 3),):
        for a in (s, S.astype(np.int64)):
            rival = np.where((n > 0) & (np.arange(D)[:, None, None] != index[None]), a, -1).max(axis=0)
            assert (rival[(kind == k_eq) & (own > 0)] % 10 == 0).all() and (rival[(kind == k_below) & (own > 0)] % 10 == 9).all()
    # the products of the largest sums need more than 32 bits with the fixed sampler's cells
    big = kind == 5
    products = clean_mirror._at(s, index)[big] * own[big] * 100
    assert big.any() and (products >= 2 ** 32).all() if cs == 24 else big.any()
    assert (S == 65535).any() and (S == 0).any()


# ---- what it buys -----------------------------------------------------------------------------------------------------------------
def _scene(oracle, W, H, D, V):
    main_cam, main_img, side_cams, sides, gt = synth.make_views(W, H, V, radius=0.3)
    z_lo, z_hi = float(gt.min()) - 0.002, float(gt.max()) + 0.002
    d_wta, c_wta, i_wta, vol = oracle.sweep(main_cam, main_img, side_cams, sides, D, z_lo, z_hi, want_volume=True, nthreads=4, sampler="fixed")
    z = oracle.plane_table(D, z_lo, z_hi)
    S = sgm_mirror.aggregate(sgm_mirror.cost16(vol, 24, 4080), 8, 16, 128)
    d_agg, c_agg, i_agg = sgm_mirror.select(S, sgm_mirror.seen_cells(vol, 24), z, 8)
    return gt, z, vol, S, (d_wta, c_wta, i_wta), (d_agg, c_agg, i_agg)


def _figures(gt, z, vol, S, maps):
    """bad share before, bad share among the kept pixels, share kept, report: parameters (2, 10, 100, 1)"""
    depth, cost, index = maps
    _, _, kept_index, report, _ = clean_mirror.clean(depth, cost, index, vol, 24, S, 2, 10, 100, 1)
    kept = kept_index >= 0
    assert (kept_index[kept] == index[kept]).all()
    return bad_share(index, gt, z), bad_share(index[kept][None], gt[kept][None], z), float(kept.mean()), report


@pytest.mark.parametrize("W,H,D,V", [(160, 120, 32, 4), (200, 150, 32, 2)])
def test_cleaning_removes_bad_pixels_and_keeps_the_rest(oracle, W, H, D, V):
    """fixed sampler, z range = ground truth +- 0.002, radius 0.3, parameters min_views 2, uniqueness 10, speckle 100 / 1.  The mirror gives
    160 x 120 x 32 x 4: winner-take-all bad 0.0518 -> 0.0213 among the 0.9432 kept, report [19200, 0, 643, 448];
                        aggregated (8, 16, 128, 4080) 0.0028 -> 0.0025 among 0.9983, [19200, 0, 31, 1];
    200 x 150 x 32 x 2: winner-take-all 0.1440 -> 0.0184 among 0.6535, [30000, 6586, 1861, 1948];
                        aggregated 0.0028 -> 0.0011 among 0.7811, [30000, 6541, 22, 3]   (DESIGN.md section 16)."""
    gt, z, vol, S, wta, agg = _scene(oracle, W, H, D, V)
    before, among, kept, report = _figures(gt, z, vol, None, wta)
    print("%d x %d x %d x %d winner-take-all: bad %.4f -> %.4f among the %.4f kept, report %s" % (W, H, D, V, before, among, kept, report))
    if V == 4:
        assert among <= 0.5 * before and kept >= 0.90
    else:
        assert among <= 0.25 * before and kept >= 0.60 and report[1] > 0.15 * W * H
    before, among, kept, report = _figures(gt, z, vol, S, agg)
    print("%d x %d x %d x %d aggregated: bad %.4f -> %.4f among the %.4f kept, report %s" % (W, H, D, V, before, among, kept, report))
    assert among <= before and kept >= 0.75


# ---- binding ------------------------------------------------------------------------------------------------------------------------
def test_constants_and_binding():
    assert mvs_amd.MVS_CLEAN_SCORES_AGGREGATED == 1
    lib = mvs_amd.load_library()
    want = {"mvs_sweep_clean": [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_uint], "mvs_sweep_clean_report": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)],
            "mvs_sweep_clean_sizes_device": [ctypes.c_void_p], "mvs_sweep_clean_sizes_fetch": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]}
    for name, argtypes in want.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name
    out = (ctypes.c_int * 4)()
    sizes = (ctypes.c_int32 * 4)()
    assert lib.mvs_sweep_clean(None, 2, 10, 100, 1, 0) == -1          # MVS_EINVAL for a NULL context, no GPU needed
    assert lib.mvs_sweep_clean_report(None, out) == -1
    assert lib.mvs_sweep_clean_sizes_fetch(None, sizes) == -1
    assert lib.mvs_sweep_clean_sizes_device(None) is None
    for name in ("sweep_clean", "sweep_clean_report", "sweep_clean_sizes"):
        assert callable(getattr(mvs_amd.Context, name))
