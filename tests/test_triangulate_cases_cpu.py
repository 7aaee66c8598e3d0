"""The crafted cases of tests/triangulate_cases.py on the CPU: the mirror (tests/triangulate_mirror.py) is the oracle on every case, every
case reaches what it declares (audited on the mirror's per-pixel diagnostics), together the cases reach every branch of
csrc/triangulate.hip that the random-flow tests of test_triangulate_gpu.py never take, and no comparison of normals can be passed by the
absolute tolerance of the GPU test."""
import functools

import numpy as np
import pytest

import triangulate_cases as tc
import triangulate_mirror as tm

RTOL = 1e-5       # the project's stated tolerance for quantities that pass through exp / pow (here: numpy's against libm's)


@functools.lru_cache(maxsize=None)
def _mirror(name):
    c = tc.by_name(name)
    return tm.triangulate_pixels(c["flows"], c["main"], c["sides"], c["depth"])


def _same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.mark.parametrize("name", tc.NAMES)
def test_mirror_is_the_oracle(name):
    got, ref = _mirror(name).rows, tc.reference(name)
    assert got.shape == ref.shape
    assert _same_bits(got[:, :4], ref[:, :4])
    g, r = got[:, 4:], ref[:, 4:]
    finite = np.isfinite(r)
    np.testing.assert_allclose(g[finite], r[finite], rtol=RTOL, atol=0)
    assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g[~finite], r[~finite], equal_nan=True)   # NaN, +inf, -inf: same class


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_reaches_what_it_declares(name):
    assert tc.audit(tc.by_name(name), _mirror(name)) == []


def test_every_family_has_a_clean_case():
    """no family is judged on its non-finite rows alone"""
    for fam in tc.FAMILIES:
        clean = [n for n in tc.NAMES if tc.by_name(n)["family"] == fam and tc.by_name(n)["clean"]]
        assert clean, fam
        for n in clean:
            ref = tc.reference(n)
            assert len(ref) and np.all(np.isfinite(ref)), n
    assert {tc.by_name(n)["family"] for n in tc.NAMES} == set(tc.FAMILIES)


def test_the_cases_reach_every_branch_the_random_inputs_miss():
    diags = {n: _mirror(n) for n in tc.NAMES}
    point = {n: d.status == tm.STATUS_POINT for n, d in diags.items()}
    # fewer than 3 valid neighbours: the fallback normal, and its neighbours 3 and more beside it
    assert sum(int((d.normal_branch == tm.BRANCH_FALLBACK).sum()) for d in diags.values()) >= 10
    # a partially dropped map (holes inside normal tiles and compaction chunks), and a fully dropped one
    d = diags["behind_partly"]
    assert (d.status == tm.STATUS_DROPPED).any() and point["behind_partly"].any()
    tiles = lambda m: {(r // tc.TILE_H, c // tc.TILE_W) for r, c in zip(*np.nonzero(m))}
    assert len(tiles(d.status == tm.STATUS_DROPPED) & tiles(point["behind_partly"])) >= 4       # tiles holding both kept and dropped pixels
    assert not point["behind_all"].any() and (diags["behind_all"].status == tm.STATUS_DROPPED).all()
    # det == 0
    assert any((d.det0 & point[n]).any() for n, d in diags.items())
    # V = 0: the values, not only the shape
    ref0 = tc.reference("views_0")
    assert len(ref0) > 15000 and np.all(np.isnan(ref0[:, :3])) and np.all(diags["views_0"].steps[point["views_0"]] == tm.MAX_STEPS)
    # the view counts at the ends of the three instantiations, and the one that skips pow()
    counts = {len(tc.by_name(n)["flows"]) for n in tc.NAMES}
    assert {0, 1, 4, 5, 8, 9, 32} <= counts
    # variance 0, tiny, huge and negative, at pixels that become points
    c = tc.by_name("variance_classes")
    var = np.stack([f[..., 2] for f in c["flows"]])[:, point["variance_classes"]]
    for v in (0.0, 1e-30, 1e30, -1.0):
        assert int((var == np.float32(v)).sum()) >= 100, v
    # every Newton step class around the hand-over, in each instantiation
    for n in ("views_4", "views_8", "views_32"):
        for s in (tc.TRI_SPLIT - 1, tc.TRI_SPLIT, tc.TRI_SPLIT + 1):
            assert (diags[n].steps[point[n]] == s).any(), (n, s)
    # goodSample false and true in one map
    d = diags["far_flows"]
    assert (d.good_sample[:, point["far_flows"]]).any() and (~d.good_sample[:, point["far_flows"]]).any()


@pytest.mark.parametrize("name", tc.NAMES)
def test_normals_are_far_above_the_absolute_tolerance(name):
    """the GPU comparison uses atol = 1e-9; it must not be what passes it.  Cases that declare exactly-zero normals are compared for
    equality on the GPU, not by tolerance."""
    ref = tc.reference(name)
    finite = np.isfinite(ref).all(1)
    if not finite.any() or tc.by_name(name)["expect"].get("zero_normals"):
        assert not finite.any() or np.all(ref[finite, 4:] == 0)
        return
    assert np.median(np.linalg.norm(ref[finite, 4:].astype(np.float64), axis=1)) > 1e-4


def test_cases_are_small_and_flows_have_a_reference():
    for n in tc.NAMES:
        c = tc.by_name(n)
        assert c["W"] * c["H"] <= 1024 * 521
        for f in c["flows"]:
            assert np.all(np.isfinite(f)) and np.abs(f[..., :2]).max() <= 1e6      # beyond: the oracle's (int) cast is undefined


@pytest.mark.parametrize("name", tc.NAMES)
def test_the_gpu_comparison_accepts_the_mirror(name):
    """compare_rows is what the GPU test applies to the library; the mirror, an independent computation of the same rows, passes it"""
    assert tc.compare_rows(_mirror(name).rows, tc.reference(name)) <= RTOL


def _pick(ref, pred):
    """(row, column) of the first component of columns 4-6 satisfying pred"""
    r, c = np.nonzero(pred(ref[:, 4:]))
    assert len(r), "no such component in this case"
    return r[0], 4 + c[0]


@pytest.mark.parametrize("name,pred,change", [
    ("views_32", np.isnan, lambda v: np.float32(np.inf)),                                # a NaN that became an infinity
    ("views_32", np.isnan, lambda v: np.float32(0.0)),                                   # a NaN that became a number
    ("islands", lambda a: np.isfinite(a) & (a != 0), lambda v: -v),                      # a flipped component
    ("islands", lambda a: np.isfinite(a) & (a != 0), lambda v: v * np.float32(1 + 3e-5)),  # a pdf off by three times the tolerance
    ("singular_with_good_view", lambda a: a == 0, lambda v: np.float32(1e-12)),          # an exact zero that is only small
], ids=["nan_to_inf", "nan_to_number", "sign_flip", "scale", "zero_to_tiny"])
def test_the_gpu_comparison_rejects_what_the_masked_one_let_through(name, pred, change):
    ref = tc.reference(name)
    bad = ref.copy()
    r, c = _pick(ref, pred)
    bad[r, c] = change(ref[r, c])
    with pytest.raises(AssertionError):
        tc.compare_rows(bad, ref)


def test_the_gpu_comparison_tells_the_infinities_apart():
    """no case has an infinite normal component in the reference (a diverged solve gives NaN); the class rule is exercised on rows made up
    from a real reference"""
    ref = tc.reference("islands").copy()
    ref[3, 5], ref[9, 4] = np.inf, -np.inf
    assert tc.compare_rows(ref.copy(), ref) == 0.0
    for r, c, v in ((3, 5, -np.inf), (3, 5, np.nan), (3, 5, 3.0e38), (9, 4, np.inf), (9, 4, np.nan)):
        bad = ref.copy()
        bad[r, c] = v
        with pytest.raises(AssertionError):
            tc.compare_rows(bad, ref)


def test_the_gpu_comparison_rejects_rotated_normals_and_shifted_rows():
    ref = tc.reference("behind_partly")
    bad = ref.copy()
    bad[7, 4:] = np.float32(np.linalg.norm(ref[7, 4:])) * np.array([0, 0, 1], np.float32)
    with pytest.raises(AssertionError):
        tc.compare_rows(bad, ref)
    with pytest.raises(AssertionError):
        tc.compare_rows(np.roll(ref, 1, axis=0), ref)                                    # a wrong compaction offset
    with pytest.raises(AssertionError):
        tc.compare_rows(ref[:-1], ref)


# which small case must catch which injectable defect of the mirror (triangulate_mirror.DEFECTS): the defect's rows fail the GPU comparison
CATCHES = {
    "gs_low_inclusive": ("far_flows_one_view", "far_flows"),
    "weights_unswapped": ("far_flows_one_view", "shape_128x48"),
    "det0_inverted": ("singular_with_good_view", "singular_whole_flows"),
    "no_drop": ("behind_partly", "behind_all"),
    "cap_49": ("islands", "variance_powers_of_two"),
    "window_short_cols": ("seam_neighbours", "shape_65x3"),
    "window_short_rows": ("seam_neighbours", "shape_19x23"),
    "n_gt_3": ("islands", "seam_neighbours", "shape_2x2"),
    "fallback_dehomog": ("islands", "seam_neighbours", "chunks_1024x521"),
    "no_flip": ("islands", "behind_partly"),
    "no_root": ("islands", "shape_2x2"),
}


def test_every_injectable_defect_is_named():
    assert set(CATCHES) == set(tm.DEFECTS)


@pytest.mark.parametrize("defect,name", [(d, n) for d, names in CATCHES.items() for n in names])
def test_case_catches_the_defect(defect, name):
    """a kernel with this defect would fail the GPU test of this case"""
    c = tc.by_name(name)
    rows = tm.triangulate_pixels(c["flows"], c["main"], c["sides"], c["depth"], defect=defect).rows
    with pytest.raises(AssertionError):
        tc.compare_rows(rows, tc.reference(name))
