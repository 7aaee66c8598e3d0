"""CPU checks of the depth selection and the sub-plane refinement on the crafted volumes of tests/select_volumes.py: the numpy mirror
(tests/select_mirror.py) against a scalar loop in Python integers and against the C oracle, the mirror's f32 refinement against exact
rational arithmetic within the bound its docstring derives, and the premise of every generator -- what share of its pixels a wrong
comparison would get wrong, which parabola situations occur -- so that a generator that goes soft fails without a GPU.  The counts are
printed (pytest -s).  tests/test_select_edges_gpu.py hands the same volumes to the kernels."""
import fractions

import numpy as np
import pytest

import select_mirror as mirror
import select_volumes as sv
import sgm_mirror as sgm

ALL = sv.CASES + sv.PARTIAL_CASES
U = 2.0 ** -24


def _ids(cases):
    return [pytest.param(c, id=c.name) for c in cases]


def _z(oracle, case):
    return oracle.plane_table(case.D, *case.z_range)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scalar_select(vol, cs, z):
    """one cell at a time, Python integers"""
    D, H, W = vol.shape
    mask = (1 << cs) - 1
    index, cost, depth = np.full((H, W), -1, np.int32), np.full((H, W), np.inf, np.float32), np.full((H, W), 1.0, np.float32)
    for y in range(H):
        for x in range(W):
            best = None
            for d in range(D):
                cell = int(vol[d, y, x])
                s, n = cell & mask, cell >> cs
                if n and (best is None or s * best[1] < best[0] * n):
                    best = (s, n, d)
            if best:
                index[y, x] = best[2]
                depth[y, x] = z[best[2]]
                cost[y, x] = np.float32(best[0]) / np.float32(best[1] if cs == 16 else 255 * best[1])
    return index, cost, depth


@pytest.mark.parametrize("case", _ids(ALL))
def test_mirror_equals_scalar_loop_and_oracle(oracle, case):
    vol, foreign = sv.volume(case)
    cs, z = sv.CS[case.sampler], _z(oracle, case)
    index, cost, depth = mirror.select(vol, cs, z)
    for got, want in zip((index, cost, depth), _scalar_select(vol, cs, z)):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    d_o, c_o, i_o = oracle.argmin(vol, z, sampler=case.sampler)
    np.testing.assert_array_equal(index, i_o)
    np.testing.assert_array_equal(_bits(cost), _bits(c_o))
    np.testing.assert_array_equal(_bits(depth), _bits(d_o))
    for idx in (index,) if foreign is None else (index, foreign):
        np.testing.assert_array_equal(_bits(mirror.refine(vol, cs, z, idx)), _bits(oracle.refine_depth(vol, z, idx, sampler=case.sampler)))


@pytest.mark.parametrize("case", _ids(sv.PARTIAL_CASES))
def test_partials_combine_to_the_selection(oracle, case):
    vol, _ = sv.volume(case)
    cs, z = sv.CS[case.sampler], _z(oracle, case)
    want = mirror.select(vol, cs, z)
    nobody = np.zeros((case.H, case.W, 2), np.uint32)
    nobody[..., 1] = mirror.NONE_RECORD[1]
    for split in sv.SPLITS:
        assert sum(split) == case.D
        first = np.concatenate(([0], np.cumsum(split)))
        recs = [mirror.select_partial(vol[a:b], cs, a) for a, b in zip(first[:-1], first[1:])]
        for parts in (recs, recs[:1] + [nobody] + recs[1:], [nobody] + recs):
            for got, w in zip(mirror.combine(parts, cs, z), want):
                np.testing.assert_array_equal(_bits(got), _bits(w))


def test_no_near_equal_pair_of_the_exact_layout_has_equal_f32_quotients():
    """select_volumes' first note: counts 256 and 257 are the only candidates, and no pair of their sums one rational step apart has it"""
    n1, n2 = 256, 257
    s1 = np.arange(0, 255 * n1 + 1, dtype=np.int64)
    found = 0
    for sign in (1, -1):                      # s1 n2 - s2 n1 = sign
        num = s1 * n2 - sign
        ok = (num % n1 == 0) & (num >= 0) & (num // n1 <= 255 * n2)
        a, b = s1[ok], num[ok] // n1
        found += int((a.astype(np.float32) / np.float32(n1) == b.astype(np.float32) / np.float32(n2)).sum())
    assert found == 0


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_sum_bits_of_an_unseen_cell_change_nothing(oracle, sampler):
    for gen in ("parabolas", "foreign_index", "extremes"):
        case = next(c for c in sv.cases_of(gen) if c.sampler == sampler and (c.W, c.D) == (132, 17))
        vol, foreign = sv.volume(case)
        cs, z = sv.CS[sampler], _z(oracle, case)
        dirty = sv.sum_bits_in_unseen_cells(vol, cs, 0xD1127)
        assert (dirty != vol).any() and ((dirty >> cs) == (vol >> cs)).all()
        want = mirror.select(vol, cs, z)
        for got, w in zip(mirror.select(dirty, cs, z), want):
            np.testing.assert_array_equal(_bits(got), _bits(w))
        index = want[0] if foreign is None else foreign
        np.testing.assert_array_equal(_bits(mirror.refine(dirty, cs, z, index)), _bits(mirror.refine(vol, cs, z, index)))
        np.testing.assert_array_equal(mirror.refine_exact(dirty, cs, z, index).z, mirror.refine_exact(vol, cs, z, index).z)
        np.testing.assert_array_equal(_bits(mirror.refine(dirty, cs, z, index)), _bits(oracle.refine_depth(dirty, z, index, sampler=sampler)))


# ---- what a wrong comparison would select ----------------------------------------------------------------------------------------
def _by_sums(vol, cs):
    s, n = sgm.split(vol, cs)
    return np.where((n != 0).any(axis=0), np.where(n != 0, s, 1 << 40).argmin(axis=0), -1)


def _by_f32_means(vol, cs, per_255):
    s, n = sgm.split(vol, cs)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = s.astype(np.float32) / (255 * n if per_255 else n).astype(np.float32)
    return np.where((n != 0).any(axis=0), np.where(n != 0, c, np.float32(np.inf)).argmin(axis=0), -1)


def _wrong_shares(vol, cs, index):
    return (float((_by_sums(vol, cs) != index).mean()), float((_by_f32_means(vol, cs, False) != index).mean()),
            float((_by_f32_means(vol, cs, True) != index).mean()))


def _full(case):
    return case.W >= 131


@pytest.mark.parametrize("case", _ids(sv.cases_of("mixed_counts", ALL)))
def test_premise_mixed_counts(oracle, case):
    vol, _ = sv.volume(case)
    cs = sv.CS[case.sampler]
    s, n = sgm.split(vol, cs)
    index = mirror.select(vol, cs, _z(oracle, case))[0]
    sums, means, means255 = _wrong_shares(vol, cs, index)
    print("%s: another plane by sums alone %.3f, by f32 means %.3f (s / 255 n: %.3f) of the pixels" % (case.name, sums, means, means255))
    if case.D >= 3:
        assert ((n == 0).any(axis=0)).all(), "every pixel has an unseen cell"
        assert all(len(set(n[:, y, x][n[:, y, x] != 0])) >= 2 for y in range(case.H) for x in range(case.W)), "two different counts"
    if case.D >= 7 and _full(case):
        assert sums >= 0.5            # D - 1 random cells: the smallest sum is the smallest mean in few pixels
    if case.D >= 2 and _full(case) and cs == 24:
        # a quarter of the pixels holds a near-equal pair, half of those with the cheaper cell at the higher plane, where equal
        # quotients keep the lower one: an eighth, less the pairs whose quotients straddle a rounding boundary
        assert means >= 1.0 / 16 and means255 >= 1.0 / 16


def _two_best(vol, cs, y, x):
    mask = (1 << cs) - 1
    cells = [(fractions.Fraction(int(c) & mask, int(c) >> cs), d, int(c) & mask, int(c) >> cs) for d, c in enumerate(vol[:, y, x]) if int(c) >> cs]
    return sorted(cells)[:2]


@pytest.mark.parametrize("case", _ids(c for c in sv.cases_of("near_equal") if c.D >= 2))
def test_premise_near_equal(oracle, case):
    vol, _ = sv.volume(case)
    cs = sv.CS[case.sampler]
    index = mirror.select(vol, cs, _z(oracle, case))[0]
    equal32 = lower = 0
    for y in range(case.H):
        for x in range(case.W):
            (c1, d1, s1, n1), (c2, d2, s2, n2) = _two_best(vol, cs, y, x)
            assert c2 - c1 == fractions.Fraction(1, n1 * n2) and c1 >= sv.PER[cs] // 2 and index[y, x] == d1
            equal32 += np.float32(s1) / np.float32(n1) == np.float32(s2) / np.float32(n2)
            lower += d1 < d2
    P = case.W * case.H
    sums, means, means255 = _wrong_shares(vol, cs, index)
    print("%s: %d pairs, f32 quotients equal in %d, cheaper cell at the lower plane in %d; another plane by sums %.3f, by f32 means %.3f (s / 255 n: %.3f)"
          % (case.name, P, equal32, lower, sums, means, means255))
    if _full(case):
        assert 0.35 * P <= lower <= 0.65 * P
        if cs == 24:   # 1 / (n1 n2) <= 2^-12 against an ulp of 2^-8: at most one pair in 16 straddles a rounding boundary
            assert equal32 >= 0.9 * P and means >= 0.3 and means255 >= 0.3


@pytest.mark.parametrize("case", _ids(c for c in sv.cases_of("ties", ALL) if c.D >= 2))
def test_premise_ties(oracle, case):
    vol, _ = sv.volume(case)
    cs, D = sv.CS[case.sampler], case.D
    s, n = sgm.split(vol, cs)
    win = mirror._winners(s, n)
    index = mirror.select(vol, cs, _z(oracle, case))[0]
    count = win.sum(axis=0)
    assert (count >= 2).all() and (index == win.argmax(axis=0)).all()
    tied_n = np.where(win, n, 0)
    different_counts = (np.where(win, n, 1 << 20).min(axis=0) != tied_n.max(axis=0))
    second = np.where(win & (np.arange(D)[:, None, None] > index[None]), np.arange(D)[:, None, None], D).min(axis=0)
    pairs = set(zip(index[second == index + 1].tolist(), second[second == index + 1].tolist()))
    print("%s: ties at %s planes; %d of %d pixels tie cells of different counts; %d boundaries (b - 1, b) hold the two lowest tied planes; %d ties at cost 0"
          % (case.name, sorted(set(count.ravel().tolist())), int(different_counts.sum()), count.size, len(pairs), int((s[win] == 0).sum())))
    if _full(case):
        assert set(count.ravel().tolist()) >= set(range(2, D + 1))
        assert pairs >= set((b - 1, b) for b in range(1, D)), "a tie across every plane boundary, part boundaries and multiples of 8 among them"
        assert 0.25 * count.size <= different_counts.sum() <= 0.75 * count.size
        assert (s[win] == 0).any() and (s[win] != 0).any()
    assert (_by_sums(vol, cs) != index).any() or D == 2


@pytest.mark.parametrize("case", _ids(sv.cases_of("extremes", ALL)))
def test_premise_extremes(oracle, case):
    vol, _ = sv.volume(case)
    cs, D = sv.CS[case.sampler], case.D
    s, n = sgm.split(vol, cs)
    index = mirror.select(vol, cs, _z(oracle, case))[0].ravel()
    s, n = s.reshape(D, -1), n.reshape(D, -1)
    nm, sm = sv.max_cell(cs)
    (an, as_), (bn, bs) = sv.straddle_cells(cs)
    if cs == 24:
        assert sm * nm == 2 ** 32 - 66716671 and as_ * bn < 2 ** 31 <= bs * an and as_ * bn < bs * an
    p = np.arange(index.size)
    k = p % 8
    seen = (n != 0).sum(axis=0)
    assert (index[k == 0] == 0).all() and (s[:, k == 0] == sm).all() and (n[:, k == 0] == nm).all()
    if D >= 2:
        assert (index[k == 1] == 0).all() and (index[k == 2] == 1).all()
        assert (n[0, k == 1] == an).all() and (n[1, k == 1] == bn).all() and (n[0, k == 2] == bn).all() and (n[1, k == 2] == an).all()
    assert (index[k == 3] == D - 1).all() and (index[k == 4] == 0).all()
    assert (index[k == 5] == D - 1).all() and (seen[k == 5] == 1).all()
    assert (index[k == 6] == -1).all() and (seen[k == 6] == 0).all()
    tail = np.array([sv.tail_plane(D, q) for q in p[k == 7] // 8])
    assert (index[k == 7] == tail).all() and (seen[k == 7] == 1).all()
    if D % 8:
        assert (tail >= 8 * (D // 8)).all() and (not _full(case) or set(tail.tolist()) == set(range(8 * (D // 8), D)))
    print("%s: best plane 0 in %d pixels, D - 1 in %d, none in %d; tail planes alone seen: %s; largest product %d"
          % (case.name, int((index == 0).sum()), int((index == D - 1).sum()), int((index < 0).sum()), sorted(set(tail.tolist())), sm * nm))


# ---- the refinement --------------------------------------------------------------------------------------------------------------
def _steps(z, index):
    """(|z[i + 1] - z[i]|, |z[i - 1] - z[i]|) in float64 for interior i (0 elsewhere)"""
    z64 = np.asarray(z, np.float64)
    D = len(z64)
    i = np.clip(index, 1, D - 2)
    inner = (index > 0) & (index < D - 1)
    return np.where(inner, np.abs(z64[i + 1] - z64[i]), 0.0), np.where(inner, np.abs(z64[i - 1] - z64[i]), 0.0)


def _check_refinement(case, vol, cs, z, index):
    """the f32 mirror against exact arithmetic -> (Exact, f32 den, compared mask, left-out mask)"""
    z32 = mirror.refine(vol, cs, z, index)
    ex = mirror.refine_exact(vol, cs, z, index)
    up, down = _steps(z, index)
    step = np.maximum(up, down)
    with np.errstate(divide="ignore", invalid="ignore"):
        err_t = np.where(ex.refined, mirror.REFINE_K * U * ex.m / ex.den, 0.0)
    compared = ex.refined & (ex.den >= 2.0 ** -10 * ex.m) & (np.abs(np.abs(ex.t) - 0.5) > err_t)
    diff = np.abs(z32.astype(np.float64) - ex.z)
    bound = step * err_t + U
    worst = float((diff[compared] / bound[compared]).max()) if compared.any() else 0.0
    assert (diff[compared] <= bound[compared]).all(), "%s: |f32 - exact| reaches %.3f of its bound" % (case.name, worst)
    # what holds everywhere
    plain = mirror.plain_depth(z, index)
    moved = z32.astype(np.float64) - plain.astype(np.float64)
    assert (np.abs(moved) <= 0.5 * step + U / 2).all()          # half a plane step, and the rounding of the last operation
    keeps = ~ex.parabola | (ex.den <= 0)
    np.testing.assert_array_equal(_bits(z32[keeps]), _bits(plain[keeps]))
    z64 = np.asarray(z, np.float64)
    i = np.clip(index, 1, len(z64) - 2)
    toward = np.where(ex.t > 0, np.sign(z64[i + 1] - z64[i]), np.where(ex.t < 0, np.sign(z64[i - 1] - z64[i]), 0.0))
    assert ((np.sign(moved) == toward) | (moved == 0))[ex.refined].all(), "a move away from the cheaper neighbour"
    ca, cb, cc, ok = mirror.neighbour_costs(vol, cs, index)
    den32 = np.where(ok, (ca - np.float32(2.0) * cb) + cc, np.float32(np.nan))
    return ex, den32, compared, ex.refined & ~compared, worst


def _count(mask):
    return int(np.count_nonzero(mask))


@pytest.mark.parametrize("case", _ids(sv.cases_of("parabolas")))
def test_premise_parabolas_and_refinement_bound(oracle, case):
    vol, _ = sv.volume(case)
    cs, D, z = sv.CS[case.sampler], case.D, _z(oracle, case)
    index = mirror.select(vol, cs, z)[0]
    if D < 3:
        np.testing.assert_array_equal(_bits(mirror.refine(vol, cs, z, index)), _bits(mirror.plain_depth(z, index)))
        return
    p = np.arange(case.W * case.H).reshape(case.H, case.W)
    assert (index == np.vectorize(lambda q: sv.parabola_plane(q, D))(p)).all(), "the crafted plane is the argmin"
    ex, den32, compared, left_out, worst = _check_refinement(case, vol, cs, z, index)
    assert (ex.den[ex.parabola] > 0).all() and (ex.t[ex.refined] > -0.5).all() and (ex.t[ex.refined] <= 0.5).all()   # an argmin's parabola
    name = np.vectorize(sv.parabola_class)(p)
    inside = (name == "vertex just inside -1/2") & (ex.t < -0.49)
    found = {
        "vertex 0": _count(ex.refined & (ex.t == 0)), "vertex +1/2": _count(ex.refined & (ex.t == 0.5)), "vertex just inside -1/2": _count(inside),
        "t > 0": _count(ex.t > 0), "t < 0": _count(ex.t < 0), "flat in f32, den* > 0": _count((den32 == 0) & (ex.den > 0)),
        "lower neighbour unseen": _count((name == "lower neighbour unseen") & ~ex.parabola & (index > 0) & (index < D - 1)),
        "upper neighbour unseen": _count((name == "upper neighbour unseen") & ~ex.parabola & (index > 0) & (index < D - 1)),
        "plane 0": _count(index == 0), "plane D - 1": _count(index == D - 1)}
    print("%s: %s; refined %d, compared %d (worst %.3f of the bound), left out %d" % (case.name, found, _count(ex.refined), _count(compared), worst, _count(left_out)))
    assert 4 * _count(left_out) <= _count(ex.refined), "more than a quarter of the refined pixels is left out of the comparison"
    if _full(case):
        need = [k for k in found if k != "flat in f32, den* > 0" or cs == 24]
        assert all(found[k] > 0 for k in need), found
        assert (name == "flat in f32")[(den32 == 0) & (ex.den > 0)].all()


@pytest.mark.parametrize("case", _ids(sv.cases_of("foreign_index")))
def test_premise_foreign_index_and_refinement_bound(oracle, case):
    vol, index = sv.volume(case)
    cs, D, z = sv.CS[case.sampler], case.D, _z(oracle, case)
    argmin = mirror.select(vol, cs, z)[0]
    if D < 3:
        np.testing.assert_array_equal(_bits(mirror.refine(vol, cs, z, index)), _bits(mirror.plain_depth(z, index)))
        return
    ex, den32, compared, left_out, worst = _check_refinement(case, vol, cs, z, index)
    found = {
        "exactly flat": _count(ex.parabola & (ex.den == 0)), "den < 0": _count(ex.parabola & (ex.den < -0.01 * ex.m)),
        "vertex beyond +-1 at den* >= m / 4": _count(ex.refined & (np.abs(ex.t) >= 1) & (4 * ex.den >= ex.m)), "vertex -1/2": _count(ex.refined & (ex.t == -0.5)),
        "den 0 in f32, den* < 0": _count((den32 == 0) & (ex.den < 0)), "no index over seen cells": _count((index < 0) & (argmin >= 0)),
        "plane 0": _count(index == 0), "plane D - 1": _count(index == D - 1)}
    print("%s: %s; index differs from the argmin in %.2f of the pixels; refined %d, compared %d (worst %.3f of the bound)"
          % (case.name, found, float((index != argmin).mean()), _count(ex.refined), _count(compared), worst))
    if _full(case):
        need = [k for k in found if k != "den 0 in f32, den* < 0" or cs == 24]
        assert all(found[k] > 0 for k in need), found
        assert (index != argmin).mean() > 0.5
