"""The crafted inputs of tests/poisson_cases.py reach what they claim -- on the oracle and the mirror alone, no GPU -- so that
tests/test_poisson_cases_gpu.py can never pass on a case that no longer reaches its edge."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_mirror as km  # noqa: E402
import meshing_oracle as mo  # noqa: E402
import poisson_cases as pc  # noqa: E402


def test_the_spacing_clouds_are_what_their_names_say():
    clouds = pc.spacing_clouds()
    assert [len(clouds["n%d" % n]) for n in (2, 3, 6, 7, 8)] == [2, 3, 6, 7, 8]
    for name, pts in clouds.items():
        assert pts.dtype == np.float32 and pts.shape[1] == 4 and np.isfinite(pts).all(), name
        per = mo.average_spacing_per_sample(pts)
        assert per.shape == (len(pts),) and abs(per.mean() - mo.average_spacing(pts)) == 0.0, name
    lattice = clouds["lattice"]
    assert len(lattice) == 125 and len(np.unique(mo.average_spacing_per_sample(lattice))) == 4     # corner, edge, face, inside: ties everywhere
    g = km.cell_grid(lattice)
    assert abs(float((np.float32(0.0) - g["ox"]) * g["inv"]) - 2.0) < 1e-6                          # its lowest samples: on a cell border, up to rounding
    assert len(clouds["duplicates"]) == 512 and np.all(mo.average_spacing_per_sample(clouds["duplicates"]) == 0.0)
    w = clouds["sphere-w"][:, 3]
    assert set(np.unique(w)) == {0.5, 2.0, -1.0, -4.0}
    xyz = clouds["sphere-w"][:, :3] / w[:, None]
    assert np.array_equal((xyz * w[:, None]).astype(np.float32), clouds["sphere-w"][:, :3])         # the quotient is exact
    out = clouds["sphere-outliers"]
    g = km.cell_grid(out)
    far = out[-8:, :3] / out[-8:, 3:4]
    lo = np.array([g["ox"], g["oy"], g["oz"]])
    hi = lo + g["cell"] * np.array([g["nx"], g["ny"], g["nz"]])
    beyond_lo, beyond_hi = far < lo, far > hi
    assert [tuple(r) for r in (beyond_hi.astype(int) - beyond_lo.astype(int))] == [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -1, -1)]
    inside = out[:-8, :3] / out[:-8, 3:4]
    assert np.mean(np.all((inside > lo) & (inside < hi), axis=1)) > 0.9


def test_the_isolated_row_exhausts_the_budget_of_the_search_as_it_was():
    """the parent rule (tests/knn_mirror.py): the passes R = 1 .. 32 around row 0 find nothing, the pass R = 64 spends the rest of the budget on
    empty rows and ends with no neighbour -- 0 where the exact value is 0.37 --, while 50 other rows get their exact values"""
    pts = pc.budget_cloud()
    assert pts.shape == (250000, 4) and np.all(pts[:, 3] == 1.0) and np.array_equal(pts[0, :3], np.array([0.6, 0.6, 0.02], np.float32))
    exact = mo.average_spacing_per_sample(pts)
    g, keys, q, ids = km.sort_by_cell(pts)
    assert min(g["nx"], g["ny"], g["nz"]) > 200          # the row is tens of cells from every other sample
    where = np.empty(len(ids), np.int64)
    where[ids] = np.arange(len(ids))
    value, info = km.parent_search(g, keys, q, int(where[pc.BUDGET_ROW]))
    assert info["R"] == 64 and info["budget"] <= 0 and info["found"] == 0 and value == 0.0
    assert 0.36 < exact[pc.BUDGET_ROW] < 0.38
    rows = np.random.default_rng(3).choice(np.arange(1, len(pts)), size=50, replace=False)
    for r in rows:
        value, info = km.parent_search(g, keys, q, int(where[r]))
        assert info["budget"] > 0 and info["found"] == 6 and abs(float(value) - exact[r]) <= 2e-6 * exact[r], (r, value, exact[r], info)


def test_the_splat_cloud_has_its_half_way_cases_and_the_exact_grid():
    pts, nrm = pc.splat_cloud()
    G, origin, h = mo.poisson_grid(pts, 4)
    assert G == pc.SPLAT_G and h == pc.SPLAT_H and np.array_equal(origin, pc.SPLAT_ORIGIN)
    xyz = pts[:, :3] / pts[:, 3:4]
    assert np.array_equal(xyz.min(0), np.zeros(3, np.float32)) and np.array_equal(xyz.max(0), np.full(3, 1.25, np.float32))
    assert {2.0, -1.0, 1.0} == set(np.unique(pts[:, 3]))
    assert mo.normal_scale_log2(nrm) == 0
    prod = pc.splat_products(pts, nrm, G, origin, h).astype(np.float64)
    half = prod[np.abs(prod - np.floor(prod)) == 0.5]
    k = np.floor(np.abs(half)).astype(np.int64)
    for sign in (1, -1):
        for parity in (0, 1):
            assert np.count_nonzero((np.sign(half) == sign) & (k % 2 == parity)) >= 8, (sign, parity)
    # rint rounds them to even; truncation, or rounding half away from zero, would give other integers
    assert np.any(np.rint(half) != np.trunc(half)) and np.any(np.rint(half) != np.sign(half) * np.floor(np.abs(half) + 0.5))
    g = (xyz - origin) / h
    t = g - np.floor(g)
    assert np.count_nonzero(np.all(t == 0.0, axis=1)) >= 4 and np.count_nonzero((t == 0.0).sum(1) == 1) >= 3 and np.count_nonzero(np.all(t == 0.5, axis=1)) >= 4
    a = np.abs(nrm)
    for value in (np.float32(1e4), np.nextafter(np.float32(1e4), np.float32(np.inf)), np.float32(np.inf)):
        assert np.any(nrm == value) and np.any(nrm == -value)
    assert np.isnan(nrm).any() and np.any((a > 0) & (a < np.finfo(np.float32).tiny)) and np.any(np.all(nrm == 0.0, axis=1))
    splat = mo.poisson_splat(pts, nrm, G, origin, h)
    assert np.abs(splat[:3]).max() > 1e4 * 65536 * 0.01 and splat[3].sum() > 0


def test_the_level_clouds_keep_their_middle_values_apart():
    """the oracle's chi at the samples: the value the lower median picks and the next one up differ by more than 100 x the tolerance of the
    level's comparison (1e-5 of chi's range), and so do all neighbours in the sorted order"""
    for n, (pts, nrm) in pc.level_clouds().items():
        assert len(pts) == n
        G, origin, h = mo.poisson_grid(pts, 4)
        assert G == pc.SPLAT_G and h == pc.SPLAT_H and np.array_equal(origin, pc.SPLAT_ORIGIN)
        chi = mo.poisson_chi(mo.poisson_splat(pts, nrm, G, origin, h), 1.0)
        vals = np.sort(mo.trilinear(chi, G, origin, h, pts[:, :3] / pts[:, 3:4]))
        tol = 1e-5 * (chi.max() - chi.min())
        assert np.diff(vals).min() > 100.0 * tol, (n, np.diff(vals) / tol)
        assert mo.poisson_level(chi, G, origin, h, pts[:, :3] / pts[:, 3:4]) == vals[(n - 1) // 2]


def test_the_fields_hold_the_patterns_they_are_there_for():
    fields = pc.fields()
    comp, count = mo.cell_components()
    for name, case in fields.items():
        assert case["chi"].dtype == np.float32 and np.isfinite(case["chi"]).all() and case["chi"].shape == (case["chi"].shape[0],) * 3, name
    for tag in ("iso0", "iso37"):
        cc = pc.corner_cases(fields["random-G9-" + tag]["chi"], fields["random-G9-" + tag]["iso"])
        assert set(range(1, 255)) <= set(np.unique(cc).tolist()), tag                                    # all 254 mixed corner patterns
        cc = pc.corner_cases(fields["checkerboard-G6-" + tag]["chi"], fields["checkerboard-G6-" + tag]["iso"])
        assert set(np.unique(cc).tolist()) <= {0b01101001, 0b10010110} and np.all(count[cc] == 4)       # four patches in every cell
        cc = pc.corner_cases(fields["slab-G12-" + tag]["chi"], fields["slab-G12-" + tag]["iso"])
        assert np.count_nonzero(count[cc] == 2) >= 10                                                   # two sheets through one cell
        for axis in "xyz":
            a, b = (pc.corner_cases(fields["ramp-%s%s-G8-%s" % (s, axis, tag)]["chi"], fields["ramp-%s%s-G8-%s" % (s, axis, tag)]["iso"]) for s in "+-")
            assert np.array_equal(a ^ b, np.where((a != 0) & (a != 255), 255, a ^ b)) and np.count_nonzero((a != 0) & (a != 255)) == 49
        ball = pc.corner_cases(fields["sphere-G12-" + tag]["chi"], fields["sphere-G12-" + tag]["iso"])
        mixed = (ball != 0) & (ball != 255)
        assert mixed.any() and not (mixed[[0, -1]].any() or mixed[:, [0, -1]].any() or mixed[:, :, [0, -1]].any())   # closed and interior
        off = pc.corner_cases(fields["sphere-off-centre-G12-" + tag]["chi"], fields["sphere-off-centre-G12-" + tag]["iso"])
        mixed = (off != 0) & (off != 255)
        assert mixed[0].any() and mixed[:, 0].any() and mixed[:, :, 0].any() and not (mixed[-1].any() or mixed[:, -1].any() or mixed[:, :, -1].any())
    assert {fields[n]["chi"].shape[0] for n in fields if n.startswith("random-G")} == {2, 3, 7, 9, 17}
    for tag, level in (("iso0", 0.0), ("iso37", pc.ISO_B)):
        case = fields["nodes-at-the-level-G7-" + tag]
        assert case["iso"] == np.float32(level) and np.count_nonzero(case["chi"] == case["iso"]) > 20
    z = fields["signed-zeros-G7"]["chi"]
    assert np.count_nonzero((z == 0) & np.signbit(z)) > 30 and np.count_nonzero((z == 0) & ~np.signbit(z)) > 30
    case = fields["nodes-next-to-a-tiny-level-G7"]
    tiny = case["iso"]
    assert 0 < tiny < np.finfo(np.float32).tiny
    steps = np.round((case["chi"].astype(np.float64) - float(tiny)) / 2.0 ** -149)
    assert all(np.count_nonzero(steps == s) > 10 for s in (-2, -1, 1, 2)) and not np.any(steps == 0)
    for name in ("constant-G5", "constant-at-the-level-G5", "below-the-level-G5", "sphere-mask-none-G12-iso0"):
        assert fields[name]["empty"]
        v, f = mo.surface_nets(fields[name]["chi"], fields[name]["iso"], fields[name]["origin"], fields[name]["h"], fields[name]["support"])
        assert len(v) == 0 and len(f) == 0
    one = fields["sphere-mask-one-node-G12-iso0"]
    assert one["support"].sum() == 1 and len(mo.surface_nets(one["chi"], one["iso"], one["origin"], one["h"], one["support"])[0]) == 1
    half = fields["sphere-mask-half-G12-iso0"]
    v, f = mo.surface_nets(half["chi"], half["iso"], half["origin"], half["h"], half["support"])
    v0, f0 = mo.surface_nets(half["chi"], half["iso"], half["origin"], half["h"])
    assert 0 < len(f) < len(f0) and 0 < len(v) < len(v0)


@pytest.mark.parametrize("name", pc.field_names())
def test_the_oracles_surface_nets_keep_what_the_gpu_test_asks_of_the_kernels(name):
    case = pc.fields()[name]
    v, f = mo.surface_nets(case["chi"], case["iso"], case["origin"], case["h"], case["support"])
    pc.check_mesh(case, v, f, mo.cell_components()[1])


def test_the_mask_cases_cover_their_seeds_and_radii():
    cases = pc.mask_cases()
    assert {R for _, R in cases.values()} == {1, 3, 16}
    for name, (w, R) in cases.items():
        assert w.shape == (16, 16, 16) and w.dtype == np.int64 and (w < 0).sum() == 1
        mask = mo.poisson_support(np.stack([w] * 4), R)
        seeds = np.argwhere(w > 0)
        assert len(seeds) == (0 if name.startswith("none") else 2 if name.startswith("two") else 1), name
        if name.startswith("two"):
            assert abs(seeds[0] - seeds[1]).max() == 2 * R + 1 and mask.sum() == 2 * (2 * R + 1) ** 3
        if R == 16 and len(seeds):
            assert mask.all()
        if not len(seeds):
            assert not mask.any()
