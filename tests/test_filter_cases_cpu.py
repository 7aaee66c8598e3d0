"""The crafted clouds of tests/filter_clouds.py on the CPU: the mirror (tests/filter_mirror.py) is the oracle bit for bit, every case's
premise holds, every observable defect the mirror can inject is caught by a case that names it, the kernel's summation shape gives the
oracle's normaliser, and the grid arithmetic -- as committed before the fix (the record of the defect) and as fixed -- is checked on
adversarial pairs.

Two of the mirror's defects cannot change keep or density on ANY cloud, and the file proves rather than pretends:
  trunc     truncation makes cell 0 twice as wide and mirrors the negative cells; x -> trunc(x / c) is still monotone with
            |x - y| <= c  =>  |trunc(x / c) - trunc(y / c)| <= 1, so the 27-cell walk still meets every accepted pair exactly once
  nan_last  densities start at 1 and stay >= 0, so a first NaN can only come from 0 * inf: normalizer = float(N / sum) = inf.
            sum = 0: every term fl((d_i + d_j) w) of sum is 0, and fl(d_j w) <= fl((d_i + d_j) w) by monotone rounding, so every score is
            0 and EVERY density becomes 0 * inf = NaN.
            sum > 0 cannot overflow N / sum: a weight is 0 or at least 2^-24 (1 - d2 / radius with the quotient a float <= 1).  In the
            first round all densities are 1 and sum >= 2 * 2^-24.  Later, if no density of the previous round was clamped, the densities
            are score_i * normalizer with the scores adding up to sum (each pair term once in either list), so they add up to about N
            and some paired point has d >= 1 / 2: sum >= 2^-25; if one was clamped it has d = 2 and a score > 0, hence a pair of
            weight >= 2^-24 (a pair of weight 0 adds nothing to a score): sum >= 2 * 2^-24.  Either way N / sum <= 2^25 N, far below
            the float range for any N an int holds.
            So NaN and non-NaN never mix; the loop stops on the NaN change, and with all keys equal the order is the index order
            whichever end NaN is ranked at.
test_unobservable_defects_change_nothing asserts both on every case."""
import functools

import numpy as np
import pytest

import filter_clouds as fc
import filter_mirror as fm

f32 = np.float32
MIRRORED = [c for c in fc.cases() if c.mirror]
UNOBSERVABLE = ("trunc", "nan_last")


def _same(a, b):
    """bit for bit, NaNs in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


@functools.lru_cache(maxsize=None)
def _run(name, defect=None, grid="oracle", sums="sequential"):
    c = fc.by_name(name)
    return fm.filter_points(c.points, c.alpha, defect=defect, grid=grid, sums=sums)


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    import orc
    c = fc.by_name(name)
    return orc.load().filter_points(c.points, c.alpha)


def _changed(name, defect, grid):
    base, bad = _run(name, None, grid), _run(name, defect, grid)
    return not (_same(base.keep, bad.keep) and _same(base.density, bad.density))


@pytest.mark.parametrize("case", MIRRORED, ids=lambda c: c.name)
def test_mirror_is_the_oracle(case):
    keep, dens = _oracle_run(case.name)
    for grid in ("oracle", "fixed"):                            # brute force, and the library's walk with the fixed cell arithmetic
        r = _run(case.name, None, grid)
        assert _same(r.keep, keep), grid
        assert _same(r.density, dens), grid
        assert not r.mixed_nan


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c.name)
def test_premise(case):
    keep, dens = _oracle_run(case.name)
    p = case.premise
    radius = fm.radius_of(case.alpha)
    p3 = fm.dehomog(case.points)
    if "density" in p:
        assert _same(dens, np.array(p["density"], f32))
    if "kept" in p:
        assert len(keep) == p["kept"]
    if "keep" in p:
        assert keep.tolist() == p["keep"]
    if "clamped" in p:
        assert int(np.count_nonzero(dens == f32(2.0))) == p["clamped"]
    if "distinct" in p:
        assert len(np.unique(dens)) == p["distinct"] < len(dens)    # tied densities
    if p.get("all_nan"):
        assert np.all(np.isnan(dens))
    if "zero_density" in p:
        assert np.all(dens[p["zero_density"]] == 0) and not np.all(np.isfinite(p3[p["zero_density"]]))
    if not case.mirror:
        return
    r = _run(case.name)
    for key in ("iterations", "pairs"):
        if key in p:
            assert getattr(r, key) == p[key], key
    if "chain_gt" in p:
        assert r.chain > p["chain_gt"] and len(case.points) <= 64     # one wavefront: one dependency level per round
    cells = fm.cells(p3, radius, "fixed")
    for i, c in p.get("cells", {}).items():
        assert tuple(cells[i]) == tuple(c), (i, cells[i])
    lo = fm.lower_lists(p3, radius)
    for i, j in p.get("split", []) + ([p["far_pair"]] if "far_pair" in p else []):
        assert j in lo[i][0]
    if "split" in p:
        assert np.all(lo[1][1] > 0)                                   # the missed pair has weight: the densities depend on it
    if "index_near" in p:
        assert abs(int(cells[0, 0]) - p["index_near"]) <= 64
    mask = fm.table_size(len(p3)) - 1
    for i, j in p.get("same_bucket", []):
        assert tuple(cells[i]) != tuple(cells[j]) and np.abs(cells[i] - cells[j]).max() > 2
        assert fm.cell_hash(cells[i], mask) == fm.cell_hash(cells[j], mask)
    if "shared_27" in p:
        i, j = p["shared_27"]
        around = [fm.cell_hash(cells[i] + d, mask) for d in fm.NEIGHBOUR_CELLS]
        assert j in lo[i][0] and np.abs(cells[i] - cells[j]).max() == 1 and around.count(fm.cell_hash(cells[j], mask)) >= 2
    if "centre" in p:                                                 # seam_26: one partner in each of the 26 cells around the centre's
        i = p["centre"]
        assert sorted(tuple(cells[j] - cells[i]) for j in lo[i][0]) == sorted(d for d in fm.NEIGHBOUR_CELLS if d != (0, 0, 0))


def test_iteration_counts_cover_both_parities_of_the_ping_pong():
    counts = [_run(c.name).iterations for c in MIRRORED if c.group == "B"]
    assert any(n % 2 == 1 and n > 1 for n in counts) and any(n % 2 == 0 and n < 200 for n in counts) and 1 in counts and 200 in counts, counts


def _variants(defect):
    return ["skip_cell:%d" % k for k in range(27)] if defect == "skip_cell" else [defect]


@pytest.mark.parametrize("case", [c for c in MIRRORED if c.defects], ids=lambda c: c.name)
def test_case_catches_the_defects_it_names(case):
    for defect in case.defects:
        if defect in UNOBSERVABLE:
            continue
        grid = "fixed" if defect in fm.GRID_DEFECTS else "oracle"
        assert any(_changed(case.name, v, grid) for v in _variants(defect)), defect


def test_every_observable_defect_is_caught_in_its_group():
    """a defect no case exposes is a failure of this file; skip_cell counts per cell: each of the 27 must be caught"""
    group_of = {"trunc": "A", "skip_cell": "A", "bucket_any": "A", "desc_lists": "B", "iter_plus": "B", "iter_minus": "B", "no_clamp": "B",
                "ties_desc": "C", "nan_last": "C"}
    assert set(group_of) == set(fm.DEFECTS)
    for defect in fm.DEFECTS:
        if defect in UNOBSERVABLE:
            continue
        grid = "fixed" if defect in fm.GRID_DEFECTS else "oracle"
        named = [c for c in MIRRORED if defect in c.defects and c.group == group_of[defect]]
        for v in _variants(defect):
            assert any(_changed(c.name, v, grid) for c in named), v


def test_unobservable_defects_change_nothing():
    """see the module docstring: asserted on every case, and the premise of the nan_last argument (no mix of NaN and numbers) with it"""
    for c in MIRRORED:
        assert not _run(c.name).mixed_nan
        assert not _changed(c.name, "nan_last", "oracle"), c.name
        assert not _changed(c.name, "trunc", "fixed"), c.name


@pytest.mark.parametrize("case", MIRRORED, ids=lambda c: c.name)
def test_kernel_summation_shape_gives_the_oracles_normaliser(case):
    """chunk_sums' tree against the oracle's sequential f64 sums: float(N / sum) is the same float in every iteration (and the stop test
    falls the same way, so count, density and keep are the same too)"""
    a, b = _run(case.name), _run(case.name, None, "oracle", "chunked")
    assert a.iterations == b.iterations
    assert _same(np.array(a.normalizers, f32), np.array(b.normalizers, f32))
    assert _same(a.density, b.density) and _same(a.keep, b.keep)


SPLIT = [c for c in fc.cases() if "split" in c.premise]


@pytest.mark.parametrize("case", SPLIT, ids=lambda c: c.name)
def test_committed_cell_arithmetic_misses_the_pair(case):
    """the record of the defect: with cell = sqrtf(radius), inv = 1.0f / cell and floorf(v * inv) the accepted pair sits two cells apart, the
    27-cell walk never meets it, and the densities are NaN where the oracle has [1, 1]"""
    p3, radius = fm.dehomog(case.points), fm.radius_of(case.alpha)
    c = fm.cells(p3, radius, "committed")
    assert np.abs(c[1] - c[0]).max() == 2
    assert np.abs(np.diff(fm.cells(p3, radius, "fixed"), axis=0)).max() <= 1
    bad = fm.filter_points(case.points, case.alpha, grid="committed")
    assert bad.pairs == 0 and np.all(np.isnan(bad.density))
    assert _same(_oracle_run(case.name)[1], np.array([1.0, 1.0], f32))


def test_committed_cell_arithmetic_changes_the_kept_set_of_the_path():
    """the same defect where the kept set shows it: the pair 3-4 of the path of consecutive floats is missed, the path falls into two
    components, and the selection is the one the MI355X returned with the library built that way (filterPoints on crafted clouds)"""
    case = fc.by_name("large_index_path12")
    bad = fm.filter_points(case.points, case.alpha, grid="committed")
    assert bad.pairs == 10 and bad.keep.tolist() == [5, 7, 8, 9, 10]
    assert _oracle_run(case.name)[0].tolist() == [3, 5, 6, 7, 8, 9]


def _adversarial_pairs(radius):
    """1-D pairs (x, y) the oracle accepts with x within 40 ulps of a cell boundary -- 0, 1 and 2^k, k = 12 .. 29, on both sides of the
    origin -- and y the farthest floats still in range on either side of x"""
    cell = np.sqrt(np.float64(radius))
    bounds = np.array([0.0, 1.0] + [2.0 ** k for k in range(12, 30)]) * cell
    bounds = np.concatenate([bounds, -bounds]).astype(f32)
    step = np.spacing(np.abs(bounds)).astype(f32)
    x = (bounds[:, None] + np.arange(-40, 41, dtype=f32)[None, :] * step[:, None]).astype(f32).ravel()
    x = np.concatenate([x, f32([-1e-30, 1e-30, -1e-38, 1e-38])])
    reach = np.sqrt(f32(radius))
    xs, ys = [], []
    for sign in (f32(1), f32(-1)):
        y0 = (x + sign * reach).astype(f32)
        for k in range(-3, 4):
            y = (y0 + f32(k) * np.spacing(np.abs(y0)).astype(f32)).astype(f32)
            d = (y - x).astype(f32)
            ok = (d * d).astype(f32) <= radius
            xs.append(x[ok])
            ys.append(y[ok])
    return np.concatenate(xs), np.concatenate(ys)


def test_fixed_cell_arithmetic_keeps_every_accepted_pair_within_one_cell():
    rng = np.random.default_rng(2024)
    radii = np.concatenate([np.exp(rng.uniform(np.log(1e-4), np.log(1.0), 2000)), [0.005, 0.0125, 0.05, 0.25, 0.104914196, 1e-4, 1.0,
                                                                                             1e-30, 1.2e-38, 1e-40, 3e-44, 1.4e-45, 1e6, 1e12]]).astype(f32)
    checked = missed_before = 0
    for radius in radii:
        x, y = _adversarial_pairs(radius)
        cx = fm.cells(np.stack([x, x, x], 1), radius, "fixed")[:, 0]
        cy = fm.cells(np.stack([y, y, y], 1), radius, "fixed")[:, 0]
        assert np.all(np.abs(cx) < 10 ** 9) and np.all(np.abs(cy) < 10 ** 9)     # inside the clamp
        gap = np.abs(cy - cx)
        assert gap.max() <= 1, (radius, x[gap.argmax()], y[gap.argmax()])
        checked += len(x)
        old = np.abs(fm.cells(np.stack([y, y, y], 1), radius, "committed")[:, 0] - fm.cells(np.stack([x, x, x], 1), radius, "committed")[:, 0])
        missed_before += int(np.count_nonzero(old > 1))
    assert checked > 2000 * 1000
    assert missed_before > 1000          # the same pairs under the committed arithmetic: the sweep is adversarial enough to have found the defect
