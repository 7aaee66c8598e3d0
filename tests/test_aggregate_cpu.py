"""CPU checks of the semi-global aggregation: the numpy mirror against a scalar triple-loop restatement of the
contract, the mirror's refinement against exact rational arithmetic, the premises of the crafted volumes that
tests/test_aggregate_edges_gpu.py gives to the kernels (tests/sgm_volumes.py), what the aggregation buys on the oracle's volume of the
synthetic scene, and the Python binding."""
import fractions

import numpy as np
import pytest

import mvs_amd
import sgm_mirror
import sgm_volumes
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


# ---- the crafted volumes do what they are for -----------------------------------------------------------------------------------
def _cases(gen):
    return [pytest.param(c, id=c.name) for c in sgm_volumes.CASES if c.gen == gen]


@pytest.mark.parametrize("case", _cases("ramp"))
def test_ramp_steps_cross_every_plane_edge(case):
    """the kernels hand L(p - r, d +- 1) over between lane slots (planes 63|64, 127|128, 191|192: the row kernel) and between waves
    (every 8th plane up to 128 planes, every 16th above: the column kernel).  At every edge b the step from plane b - 1 (code 2 at
    plane b) and the step from plane b (code 3 at plane b - 1) must win uniquely somewhere, along a horizontal path and along a
    vertical or diagonal one, over the case's offsets together."""
    cs = sgm_volumes.CS[case.sampler]
    edges = [b for b in range(1, case.D) if b % 8 == 0]
    for paths, p1, p2, cap in case.params:
        up = np.zeros((2, case.D), bool)      # [horizontal / other][plane]: code 2 seen
        down = np.zeros((2, case.D), bool)    # code 3 seen
        for off, (_, vol) in zip(case.args, sgm_volumes.volumes(case)):
            C = sgm_mirror.cost16(vol, cs, cap)
            np.testing.assert_array_equal(C, np.minimum(cap, sgm_volumes.ramp_costs(case.W, case.H, case.D, off)))
            for dy, dx in sgm_mirror.PATHS[:paths]:
                w = sgm_mirror.winners(C, dy, dx, p1, p2)
                up[int(dy != 0)] |= (w == 2).any(axis=(1, 2))
                down[int(dy != 0)] |= (w == 3).any(axis=(1, 2))
        for kind, name in enumerate(("horizontal", "vertical or diagonal")):
            missed = [b for b in edges if not (up[kind, b] and down[kind, b - 1])]
            assert not missed, "%s, %d paths: no %s path crosses the plane edges %s both ways" % (case.name, paths, name, missed)


@pytest.mark.parametrize("case", _cases("saturating"))
def test_saturating_reaches_the_16_bit_ceiling(case):
    cs = sgm_volumes.CS[case.sampler]
    (_, vol), = sgm_volumes.volumes(case)
    seen = sgm_mirror.seen_cells(vol, cs)
    assert seen[0].all() and 0.4 < seen[1:].mean() < 0.6
    for paths, p1, p2, cap in case.params:
        C = sgm_mirror.cost16(vol, cs, cap)
        assert (C[0] == 0).all() and (C[1:] == cap).all()
        assert (sgm_mirror.split(vol, cs)[0][1:][seen[1:]] * 16 >= cap * (255 if cs == 24 else 1) * sgm_mirror.split(vol, cs)[1][1:][seen[1:]]).all()
        S = sgm_mirror.aggregate(C, paths, p1, p2)
        assert int(S.max()) == paths * (cap + p2) and paths * (cap + p2) > 65535 - paths
        at_ceiling = S.max(axis=(1, 2)) == paths * (cap + p2)   # not the lowest planes: L(d) <= L(0) + d P1 keeps them down
        assert at_ceiling[-1] and at_ceiling.sum() >= case.D // 2


@pytest.mark.parametrize("case", _cases("division_edges"))
def test_division_edges_straddle_the_floor_boundaries(case):
    cs = sgm_volumes.CS[case.sampler]
    (_, vol), = sgm_volumes.volumes(case)
    s, n = sgm_mirror.split(vol, cs)
    assert set(np.unique(n)) == set(range(1, 256 if cs == 24 else 257))
    den = n * 255 if cs == 24 else n
    q = (16 * s) // den     # before the cap
    for count in np.unique(n):
        mine = n == count
        quotient = dict(zip(s[mine].tolist(), q[mine].tolist()))
        assert any(v - 1 in quotient and quotient[v - 1] != quotient[v] for v in quotient), "count %d: no pair of sums across a floor boundary" % count
        assert (255 * 255 * count if cs == 24 else 65535) in quotient, "count %d: the largest legal sum is missing" % count
    for paths, p1, p2, cap in case.params:
        assert p1 == 0 and p2 == 0
        C = sgm_mirror.cost16(vol, cs, cap)
        for value in (0, 1, cap - 1, cap):
            assert (C == value).any(), "no cell with C = %d" % value
        assert (q[C == cap] == cap).any() and (q[C == cap] > cap).any(), "the cap both met and exceeded"
        np.testing.assert_array_equal(sgm_mirror.aggregate(C, paths, 0, 0), paths * C)   # L = C: the cost kernel alone decides S


@pytest.mark.parametrize("case", _cases("noise"))
def test_noise_has_every_kind_of_winner_and_ties(case):
    """code 4 (the jump, m + P2), code 1 (the own plane) and code -1 (equal smallest terms) occur, the selection has a tie at the
    minimum, and the two special pixels exist.  With two planes the jump cannot win alone: m is the own plane or the other one, and
    P1 <= P2, so m + P2 never lies below both; D = 2 is exempt from code 4."""
    cs = sgm_volumes.CS[case.sampler]
    (_, vol), = sgm_volumes.volumes(case)
    seen = sgm_mirror.seen_cells(vol, cs)
    count = seen.sum(axis=0)
    assert count[sgm_volumes.nobody_sees(case.W, case.H)] == 0 and count[sgm_volumes.one_seen_cell(case.W, case.H)] == 1
    assert 0.05 < 1.0 - seen.mean() < 0.5
    for paths, p1, p2, cap in case.params:
        C = sgm_mirror.cost16(vol, cs, cap)
        assert (C == cap).any() and (C == 0).any()
        codes = set()
        for dy, dx in sgm_mirror.PATHS[:paths]:
            codes |= set(np.unique(sgm_mirror.winners(C, dy, dx, p1, p2)).tolist())
        assert {0, 1, -1} <= codes and (4 in codes or case.D == 2), "%s %s: winners %s" % (case.name, (paths, p1, p2, cap), sorted(codes))
        S = sgm_mirror.aggregate(C, paths, p1, p2)
        masked = np.where(seen, S.astype(np.int64), 1 << 40)
        ties = ((masked == masked.min(axis=0)).sum(axis=0) > 1) & seen.any(axis=0)
        assert ties.any(), "%s %s: no tie at the minimum of the selection" % (case.name, (paths, p1, p2, cap))


def test_ramp_and_saturating_cost_the_same_for_both_samplers():
    """CASES runs them with the fixed sampler only; the exact sampler's cells must give the same C"""
    W, H, D = 21, 6, 17    # 300 * 16 planes: past the cap
    for off in (0, 7):
        want = sgm_volumes.ramp_costs(W, H, D, off)
        assert want.min() == 0 and want.max() == sgm_volumes.CAP and (want[:, 0, 0] == np.minimum(sgm_volumes.CAP, 300 * np.abs(np.arange(D) - off))).all()
        for cs in (24, 16):
            np.testing.assert_array_equal(sgm_mirror.cost16(sgm_volumes.ramp(W, H, D, cs, off), cs, sgm_volumes.CAP), want)
    np.testing.assert_array_equal(sgm_mirror.cost16(sgm_volumes.saturating(W, H, D, 16), 16, 4080), sgm_mirror.cost16(sgm_volumes.saturating(W, H, D, 24), 24, 4080))
    np.testing.assert_array_equal(sgm_mirror.seen_cells(sgm_volumes.saturating(W, H, D, 16), 16), sgm_mirror.seen_cells(sgm_volumes.saturating(W, H, D, 24), 24))


def test_winners_on_a_volume_worked_by_hand():
    """one row, three planes, P1 2, P2 5: every code once"""
    C = np.array([[[0, 9, 9, 0]], [[4, 0, 9, 0]], [[9, 9, 0, 9]]])   # [D = 3, H = 1, W = 4]
    w = sgm_mirror.winners(C, 0, +1, 2, 5)
    # x = 1: L(x = 0) = (0, 4, 9), m = 0: plane 0 own 0; plane 1 min(4, 0 + 2, 9 + 2, 5) = 2 from d - 1; plane 2 min(9, 4 + 2, 5) = 5 jump
    assert w[:, 0, 0].tolist() == [0, 0, 0] and w[:, 0, 1].tolist() == [1, 2, 4]
    # x = 2: L(x = 1) = (9, 2, 14), m = 2: plane 0 min(9, 2 + 2, 7) = 4 from d + 1; plane 1 own 2; plane 2 min(14, 2 + 2, 7) = 4 from d - 1
    assert w[:, 0, 2].tolist() == [3, 1, 2]
    # x = 3: L(x = 2) = (11, 9, 2), m = 2: plane 0 min(11, 9 + 2, 7) = 7 jump; plane 1 min(9, 11 + 2, 2 + 2, 7) = 4 from d + 1; plane 2 own
    assert w[:, 0, 3].tolist() == [4, 3, 1]
    assert (sgm_mirror.winners(np.zeros((3, 1, 4), int), 0, -1, 0, 0)[:, 0, :3] == -1).all()   # equal terms: no unique winner


# ---- rule 5 in exact arithmetic -------------------------------------------------------------------------------------------------
def _rn32(x):
    """the float32 nearest to the rational x, ties to even, as a Fraction: the two neighbours on float32's grid at x, the choice by
    exact distance (normal range only; no float64 on the way)"""
    x = fractions.Fraction(x)
    if x == 0:
        return x
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if fractions.Fraction(2) ** e > a:
        e -= 1
    assert fractions.Fraction(2) ** e <= a < fractions.Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = fractions.Fraction(2) ** (e - 23)
    lo = (a / ulp).__floor__()
    below, above = a - lo * ulp, (lo + 1) * ulp - a
    k = lo if below < above or (below == above and lo % 2 == 0) else lo + 1
    return k * ulp if x > 0 else -(k * ulp)


def _f32(x):
    """Fraction that is a float32 value -> np.float32 (exact)"""
    v = np.float32(float(x))
    assert fractions.Fraction(float(v)) == x
    return v


def _fma_exact(a, b, c):
    F = fractions.Fraction
    return _f32(_rn32(F(float(a)) * F(float(b)) + F(float(c))))


def _refine_scalar(S, seen, z, index, taken):
    """rule 5 one pixel at a time: every float32 operation of refine_depth exactly, then rounded once.  `taken` counts the branches."""
    F = fractions.Fraction
    D, H, W = S.shape
    zq = [F(float(v)) for v in z]
    out = np.empty((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            i = int(index[y, x])
            if i < 0:
                taken["no index"] += 1
                out[y, x] = np.float32(1.0)   # MVS_BACKGROUND_DEPTH
                continue
            out[y, x] = z[i]
            if i == 0 or i == D - 1:
                taken["index 0" if i == 0 else "index D - 1"] += 1
                continue
            if not (seen[i - 1, y, x] and seen[i, y, x] and seen[i + 1, y, x]):
                taken["unseen neighbour"] += not (seen[i - 1, y, x] and seen[i + 1, y, x])
                continue
            ca, cb, cc = F(int(S[i - 1, y, x])), F(int(S[i, y, x])), F(int(S[i + 1, y, x]))   # u16: exact as float32
            den = _rn32(_rn32(ca - _rn32(2 * cb)) + cc)
            if den <= 0:
                taken["den <= 0"] += 1
                continue
            t = _rn32(_rn32(F(1, 2) * _rn32(ca - cc)) / den)
            if t > F(1, 2):
                taken["t clipped at +0.5"] += 1
                t = F(1, 2)
            elif t < -F(1, 2):
                taken["t clipped at -0.5"] += 1
                t = -F(1, 2)
            if t >= 0:
                taken["t >= 0"] += 1
                r = _rn32(t * _rn32(zq[i + 1] - zq[i]) + zq[i])
            else:
                taken["t < 0"] += 1
                r = _rn32(-t * _rn32(zq[i - 1] - zq[i]) + zq[i])
            out[y, x] = _f32(r)
    return out


def test_refine_mirror_equals_a_scalar_restatement():
    rng = np.random.Generator(np.random.PCG64(0x5EF1))
    D, H, W = 7, 24, 40
    S = rng.integers(0, 40, (D, H, W)).astype(np.uint16)
    S[:, :, W // 2:] = rng.integers(0, 65536, (D, H, W - W // 2))    # the right half: sums of full range
    seen = rng.random((D, H, W)) > 0.08
    z = np.sort(rng.uniform(-1.0, 1.0, D)).astype(np.float32)         # uneven spacing: the differences round
    index = rng.integers(-1, D, (H, W)).astype(np.int32)              # any plane, not only the best one: t leaves [-0.5, 0.5]
    taken = dict.fromkeys(("no index", "index 0", "index D - 1", "unseen neighbour", "den <= 0", "t clipped at +0.5", "t clipped at -0.5",
                           "t >= 0", "t < 0"), 0)
    want = _refine_scalar(S, seen, z, index, taken)
    print(taken)
    assert all(taken.values()), "a branch of rule 5 was not taken: %s" % taken
    got = sgm_mirror.refine(S, seen, z, index)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    # and on a selection of the mirror's own (t within [-0.5, 0.5] by construction)
    _, _, best = sgm_mirror.select(S, seen, z, 8)
    np.testing.assert_array_equal(sgm_mirror.refine(S, seen, z, best), _refine_scalar(S, seen, z, best, taken))


def test_fma32_equals_the_exact_fma():
    """sgm_mirror._fma32 against RN32 of the exact a b + c: random triples, triples whose exact sum is the midpoint of two float32
    neighbours (ties to even), and triples whose exact sum misses a midpoint by less than float64 resolves, so that the float64 sum
    lands on the midpoint and a second rounding from there goes the wrong way half of the time"""
    rng = np.random.Generator(np.random.PCG64(0xF3A))
    F = fractions.Fraction

    def check(a, b, c):
        a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
        got = sgm_mirror._fma32(a, b, c)
        want = np.array([_fma_exact(*abc) for abc in zip(a, b, c)], np.float32)
        np.testing.assert_array_equal(got, want)
        return want

    def signed(n, lo, hi):
        return (rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)

    n = 2000
    check(signed(n, 0.001, 100.0), signed(n, 0.001, 100.0), signed(n, 0.001, 100.0))
    a, b = signed(n, 0.5, 2.0), signed(n, 0.5, 2.0)
    check(a, b, (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.uniform(-1e-6, 1e-6, n))).astype(np.float32))   # cancellation

    def midpoints(n):
        M = 2 * rng.integers(1 << 23, 1 << 24, n) + 1     # odd, 25 bits: M 2^j is the midpoint of two float32 neighbours
        return M, rng.integers(-20, 20, n)

    def on_a_midpoint(a, b, c, M, j):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        return s == np.ldexp(M.astype(np.float64), j) * np.sign(s)

    # exact ties: a = A 2^ja and b = B 2^jb with odd A, B < 2^12, c = (M - A B) 2^j with j = ja + jb (even, below 2^25: a float32)
    M, j = midpoints(n)
    A, B = 2 * rng.integers(0, 1 << 11, n) + 1, 2 * rng.integers(0, 1 << 11, n) + 1
    ja = rng.integers(-10, 10, n)
    sign = rng.choice([-1.0, 1.0], n)
    a, b, c = (np.ldexp(A.astype(np.float64), ja) * sign).astype(np.float32), np.ldexp(B.astype(np.float64), j - ja).astype(np.float32), \
        (np.ldexp((M - A * B).astype(np.float64), j) * sign).astype(np.float32)
    assert on_a_midpoint(a, b, c, M, j).all()
    assert all(F(float(p)) * F(float(q)) + F(float(r)) == F(int(m)) * F(2) ** int(e) * int(sg) for p, q, r, m, e, sg in zip(a, b, c, M, j, sign))
    want = check(a, b, c)
    k = np.round(np.abs(want.astype(np.float64)) / np.ldexp(1.0, j + 1)).astype(np.int64)
    assert (k % 2 == 0).all() and ((2 * k == M + 1).any() and (2 * k == M - 1).any())   # to even, which is up for some and down for others

    # near misses: (1 + x)(1 - x + x^2) = 1 + x^3 with x = +-2^-k; a b 2^j + (M - 1) 2^j = M 2^j + x^3 2^j, and 2^-3k lies below half
    # a unit of float64 at M 2^j (2^(j - 29)) from k = 10 on.  1 - x + x^2 is a float32 up to k = 12 (x > 0) or k = 11 (x < 0).
    M, j = midpoints(n)
    k = rng.integers(10, 12, n)
    x = np.ldexp(rng.choice([-1.0, 1.0], n), -k)
    k12 = rng.random(n) < 0.2
    x[k12] = 2.0 ** -12
    sign = rng.choice([-1.0, 1.0], n)
    a, b, c = ((1.0 + x) * sign).astype(np.float32), np.ldexp(1.0 - x + x * x, j).astype(np.float32), (np.ldexp((M - 1).astype(np.float64), j) * sign).astype(np.float32)
    assert (a.astype(np.float64) == (1.0 + x) * sign).all() and (b.astype(np.float64) == np.ldexp(1.0 - x + x * x, j)).all()
    assert on_a_midpoint(a, b, c, M, j).all()
    assert all(F(float(p)) * F(float(q)) + F(float(r)) != F(int(m)) * F(2) ** int(e) * int(sg) for p, q, r, m, e, sg in zip(a, b, c, M, j, sign))
    want = check(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive != want).any() and (naive == want).any(), "premise: rounding the float64 sum again is wrong for some of these"
