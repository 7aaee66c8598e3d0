"""The device stages of csrc/poisson.hip on the crafted inputs of tests/poisson_cases.py (tests/test_poisson_cases_cpu.py shows that they
reach what they claim): the spacing search per sample against the k-d tree, the surface nets on chosen fields against the oracle and
against what must hold whatever an oracle says, the support mask against the oracle and a brute-force distance, the fixed-point splat
integer for integer at exact half-way cases, and the level as the LOWER median."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshing_common as mc  # noqa: E402
import meshing_oracle as mo  # noqa: E402
import poisson_cases as pc  # noqa: E402

# a spacing is sqrt(dx^2 + dy^2 + dz^2) summed over six neighbours and divided: about a dozen float32 operations of at most 2.5 ulp each
# (the k-d tree works in float64 on the same float32 quotients); 1e-12 absolute for the zeros
SPACING_RTOL, SPACING_ATOL = 2e-6, 1e-12


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401  (the HIP runtime, first)
    return ctypes.CDLL(os.path.join(mc.LIBDIR, "libmvs_hip.so"))


@pytest.fixture(scope="module")
def patch_count(hip):
    table = (ctypes.c_uint32 * 256)()
    assert hip.mvs_test_cell_patch_table(table) == 0
    return np.array(table, np.int64) >> 24


# ---- spacing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.spacing_clouds()))
def test_spacing_per_sample_equals_the_kd_tree(hip, name):
    pts = pc.spacing_clouds()[name]
    exact = mo.average_spacing_per_sample(pts)
    got = mc.spacing_per_sample(hip, pts).astype(np.float64)
    err = np.abs(got - exact)
    worst = int(np.argmax(err - SPACING_RTOL * exact))
    print(name, "worst sample", worst, "device", got[worst], "exact", exact[worst], "relative", err[worst] / max(exact[worst], 1e-300))
    assert np.all(err <= SPACING_RTOL * exact + SPACING_ATOL), (name, worst, got[worst], exact[worst])
    if name == "duplicates":
        assert np.all(got == 0.0)


def test_spacing_of_a_sample_that_spends_its_budget_on_empty_cells(hip):
    """pc.budget_cloud(): around row 0 the search walks empty cell rows until its budget is gone.  Whatever it then reports comes from true
    distances to six distinct other samples -- never below the exact value, never 0 --; every other sample gets its exact value; and the
    public entry point reports the mean of exactly these values"""
    pts = pc.budget_cloud()
    exact = mo.average_spacing_per_sample(pts)
    got = mc.spacing_per_sample(hip, pts)
    g64 = got.astype(np.float64)
    row = pc.BUDGET_ROW
    print("isolated row: device", g64[row], "exact", exact[row])
    assert np.all(g64 >= exact * (1.0 - SPACING_RTOL) - SPACING_ATOL)
    assert g64[row] > 0.0
    others = np.arange(len(pts)) != row
    assert np.all(np.abs(g64 - exact)[others] <= SPACING_RTOL * exact[others] + SPACING_ATOL)
    nrm = np.zeros((len(pts), 3), np.float32)
    nrm[:, 2] = 1.0
    r = mc.poisson(hip, pts, nrm, 5, 1.0, keep=False)
    assert np.float32(r["spacing"]) == np.float32(np.cumsum(g64)[-1] / len(pts))          # summed in float64 in sample order, rounded once
    assert np.array_equal(mc.spacing_per_sample(hip, pts), got)         # and the same bytes again


def test_the_public_average_is_the_mean_of_the_per_sample_values(hip):
    for name in ("sphere-w", "sphere-outliers", "lattice"):
        pts = pc.spacing_clouds()[name]
        got = mc.spacing_per_sample(hip, pts).astype(np.float64)
        nrm = np.ones((len(pts), 3), np.float32)
        r = mc.poisson(hip, pts, nrm, 5, 1.0, keep=False)
        assert np.float32(r["spacing"]) == np.float32(np.cumsum(got)[-1] / len(pts)), name      # summed in float64 in sample order, rounded once


def test_spacing_hook_refuses_what_the_entry_point_refuses(hip):
    pts = pc.spacing_clouds()["n8"]
    out = np.zeros(8, np.float32)
    p, o = pts.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    assert hip.mvs_test_average_spacing(None, 8, o) == -1 and hip.mvs_test_average_spacing(p, 1, o) == -1 and hip.mvs_test_average_spacing(p, 8, None) == -1
    same = np.tile(pts[:1], (8, 1))
    assert hip.mvs_test_average_spacing(same.ctypes.data_as(ctypes.c_void_p), 8, o) == -1        # no extent
    bad = pts.copy()
    bad[3, 1] = np.nan
    assert hip.mvs_test_average_spacing(bad.ctypes.data_as(ctypes.c_void_p), 8, o) == -1


# ---- surface nets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.field_names())
def test_surface_nets_on_a_chosen_field(hip, patch_count, name):
    case = pc.fields()[name]
    chi, iso, origin, h = case["chi"], case["iso"], case["origin"], case["h"]
    G = chi.shape[0]
    v, f = mc.surface_nets(hip, chi, iso, origin, h, case["support"])
    rv, rf = mo.surface_nets(chi, iso, origin, h, None if case["support"] is None else case["support"].astype(bool))
    assert len(v) == len(rv) and len(f) == len(rf), (name, len(v), len(rv), len(f), len(rf))
    assert np.array_equal(f, rf), name
    if len(v):
        err = float(np.abs(v - rv).max())
        print(name, "vertices", len(v), "faces", len(f), "largest vertex difference", err)
        assert err <= 2e-6 * float(np.abs(origin).max() + G * h), name
    pc.check_mesh(case, v, f, patch_count)


def test_surface_nets_hook_refuses_bad_arguments(hip):
    case = pc.fields()["random-G3-iso0"]
    s = ctypes.c_void_p()
    chi, origin = case["chi"].ctypes.data_as(ctypes.c_void_p), case["origin"].ctypes.data_as(ctypes.c_void_p)
    h, iso = ctypes.c_float(0.05), ctypes.c_float(0.0)
    assert hip.mvs_test_surface_nets(None, 3, origin, h, iso, None, ctypes.byref(s)) == -1
    assert hip.mvs_test_surface_nets(chi, 1, origin, h, iso, None, ctypes.byref(s)) == -1
    assert hip.mvs_test_surface_nets(chi, 3, None, h, iso, None, ctypes.byref(s)) == -1
    assert hip.mvs_test_surface_nets(chi, 3, origin, ctypes.c_float(0.0), iso, None, ctypes.byref(s)) == -1
    assert hip.mvs_test_surface_nets(chi, 3, origin, h, iso, None, None) == -1


# ---- support mask ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.mask_cases()))
def test_support_mask_equals_the_oracle_and_a_brute_force_distance(hip, name):
    w, R = pc.mask_cases()[name]
    got = mc.support_mask(hip, w, R)
    assert np.array_equal(got, mo.poisson_support(np.stack([w] * 4), R)), name
    G = w.shape[0]
    seeds = np.argwhere(w > 0)
    k, j, i = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    brute = np.zeros(w.shape, bool)
    for sk, sj, si in seeds:
        brute |= np.maximum(np.maximum(abs(k - sk), abs(j - sj)), abs(i - si)) <= R          # Chebyshev distance, no wrap
    assert np.array_equal(got, brute), name


# ---- splat and level -------------------------------------------------------------------------------------------------------------
def test_splat_rounds_half_way_cases_to_even_and_drops_what_is_no_estimate(hip):
    pts, nrm = pc.splat_cloud()
    r = mc.poisson(hip, pts, nrm, 4, 1.0)
    assert r["G"] == pc.SPLAT_G and np.float32(r["h"]) == pc.SPLAT_H and np.array_equal(r["origin"], pc.SPLAT_ORIGIN) and r["normal_scale_log2"] == 0
    splat = mo.poisson_splat(pts, nrm, pc.SPLAT_G, pc.SPLAT_ORIGIN, pc.SPLAT_H)
    diff = np.argwhere(splat != r["splat"])
    assert len(diff) == 0, (len(diff), diff[:5], splat[tuple(diff[0])], r["splat"][tuple(diff[0])])


@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_level_is_the_lower_median_of_the_returned_field(hip, n):
    pts, nrm = pc.level_clouds()[n]
    r = mc.poisson(hip, pts, nrm, 4, 1.0)
    assert r["G"] == pc.SPLAT_G and np.float32(r["h"]) == pc.SPLAT_H and np.array_equal(r["origin"], pc.SPLAT_ORIGIN)
    assert np.array_equal(r["splat"], mo.poisson_splat(pts, nrm, pc.SPLAT_G, pc.SPLAT_ORIGIN, pc.SPLAT_H))
    chi = r["chi"].astype(np.float64)
    vals = np.sort(mo.trilinear(chi, r["G"], r["origin"], r["h"], pts[:, :3] / pts[:, 3:4]))
    lower, upper = vals[(n - 1) // 2], vals[(n - 1) // 2 + 1]
    tol = 1e-5 * (chi.max() - chi.min())
    print(n, "level", r["iso"], "sorted samples", vals, "tolerance", tol)
    assert abs(r["iso"] - lower) <= tol
    assert abs(r["iso"] - lower) < abs(r["iso"] - upper)
    if (n - 1) // 2 > 0:
        assert abs(r["iso"] - lower) < abs(r["iso"] - vals[(n - 1) // 2 - 1])
