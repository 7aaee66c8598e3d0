"""The crafted cameras of tests/sweep_cameras.py on the CPU: every case is what it is there for (its premise over the mirror's numbers), the
oracle's view matrix has the designed dyadic entries, and oracle/sweep_oracle.c equals tests/sweep_mirror.py -- a restatement of DESIGN.md
section 2 that calls nothing of the oracle -- on volume, depth, cost and index of both samplers, by exact equality."""
import numpy as np
import pytest

import sweep_cameras as sc
import sweep_mirror as sm

NAMES = sorted(sc.CASES)


def test_weight_table_equals_the_formula(oracle):
    table = sm.weight_table()
    assert (table.astype(np.int64).sum(axis=2) == 255).all()
    np.testing.assert_array_equal(oracle.fx_weight_table(), table)


def test_rne_decides_ties_on_exact_numbers():
    """u = RNE(s 256 r + 4): halves go to the even integer, and a product a hair off the half goes where it belongs"""
    s = np.array([0.001953125, 0.005859375, 0.509765625, 0.498046875, np.nextafter(np.float32(0.509765625), np.float32(1)), 3.0e38, np.nan], np.float32)
    u, tie = sm.rne_u(s, np.ones_like(s))
    assert list(u[:5]) == [4, 6, 134, 132, 135] and list(tie[:5]) == [True, True, True, True, False]   # 0.5 -> 0, 1.5 -> 2, 130.5 -> 130, 127.5 -> 128
    assert u[5] > 1 << 30 and u[6] == -1


def test_plane_table_equals_the_oracle(oracle):
    for D in (1, 16, 17, 33):
        np.testing.assert_array_equal(oracle.plane_table(D, -1.0, 1.0), sm.plane_table(D))


def test_exact_u_is_the_number_the_mirror_rounds():
    """affine dyadic cameras: the float32 projection is exact, so the Fraction form and the array form see the same real number"""
    c = sc.CASES["shear_tie"]
    m = sc.mirror_of("shear_tie", "fixed")
    for col, row, d in ((0, 0, 0), (63, 7, 15), (17, 3, 8), (0, 7, 7)):
        u = sm.exact_u(m["q"][0], col, row, m["z"][d], c.W, c.H)
        assert u.denominator == 2
        lo, hi = int(u - sm.Fraction(1, 2)), int(u + sm.Fraction(1, 2))
        assert int(m["views"][0]["ux"][d, row, col]) == (lo if lo % 2 == 0 else hi)


@pytest.mark.parametrize("name", NAMES)
def test_view_matrix_has_the_designed_entries(oracle, name):
    c = sc.CASES[name]
    for cam, q in zip(c.side_cams, c.q()):
        np.testing.assert_array_equal(oracle.view_matrix(c.main_cam, cam, c.W, c.H), q)


@pytest.mark.parametrize("name", [n for n in NAMES if sc.CASES[n].premise])
def test_case_is_what_it_is_there_for(name):
    c = sc.CASES[name]
    c.premise(c, sc.mirror_of(name, "fixed"))


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_mirror(oracle, name, sampler):
    c = sc.CASES[name]
    m = sc.mirror_of(name, sampler)
    main, sides = c.frames()
    depth, cost, index, vol = oracle.sweep(c.main_cam, main, c.side_cams, sides, c.D, want_volume=True, nthreads=4, sampler=sampler)
    np.testing.assert_array_equal(vol, m["volume"])
    np.testing.assert_array_equal(index, m["index"])
    np.testing.assert_array_equal(depth, m["depth"])
    np.testing.assert_array_equal(cost, m["cost"])
