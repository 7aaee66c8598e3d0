"""csrc/triangulate.hip against the oracle on the crafted cases of tests/triangulate_cases.py, with no row left out of the comparison
(triangulate_cases.compare_rows): positions bit for bit, pdf-scaled normals within the stated rtol = 1e-5 of the device exp / pow,
non-finite components by class, directions to 1e-6, exact zeros exact.  What each case reaches is audited on the CPU
(test_triangulate_cases_cpu.py)."""
import numpy as np
import pytest

import mvs_amd
import triangulate_cases as tc

pytestmark = pytest.mark.gpu


def _run(ctx, name):
    c = tc.by_name(name)
    return ctx.triangulate(c["flows"], c["main"], c["sides"], c["depth"])


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_matches_the_oracle(name):
    c = tc.by_name(name)
    with mvs_amd.Context(c["W"], c["H"]) as ctx:
        got = _run(ctx, name)
    ref = tc.reference(name)
    if "points" in c["expect"]:
        assert len(ref) == c["expect"]["points"]
    worst = tc.compare_rows(got, ref)
    print("\n%s: %d rows, largest relative difference in columns 4-6: %.3g" % (name, len(ref), worst))


@pytest.mark.parametrize("name", ["views_4", "views_8", "views_32", "far_flows", "behind_partly", "chunks_1024x521"])
def test_same_case_twice_gives_the_same_bytes(name):
    """the order in which unconverged pixels enter the second Newton pass's queue differs from run to run and must not show"""
    c = tc.by_name(name)
    with mvs_amd.Context(c["W"], c["H"]) as ctx:
        a = _run(ctx, name)
        b = _run(ctx, name)
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_nothing_survives_a_call_on_the_same_context():
    """dense, then sparse, then empty, then sparse again on ONE 150 x 40 context: nothing of the valid flags, the staged (x, y, z, valid)
    records or the queue length of a call may reach the next"""
    with mvs_amd.Context(150, 40) as ctx:
        for name in ("behind_partly", "islands", "behind_all", "islands", "singular_only_view", "seam_neighbours"):
            got = _run(ctx, name)
            tc.compare_rows(got, tc.reference(name))
    assert len(tc.reference("behind_all")) == 0 and len(tc.reference("islands")) == tc.by_name("islands")["expect"]["points"]


def test_33_views_are_refused_and_the_context_stays_usable():
    c = tc.by_name("views_32")
    W, H = c["W"], c["H"]
    flows = list(c["flows"]) + [c["flows"][0]]
    sides = np.concatenate([c["sides"], c["sides"][:1]])
    small = tc.by_name("views_4")
    with mvs_amd.Context(W, H) as ctx:
        with pytest.raises(mvs_amd.MvsError, match=r"error -1\b.*at most 32 side views"):     # MVS_EINVAL
            ctx.triangulate(flows, c["main"], sides, c["depth"])
        tc.compare_rows(_run(ctx, "views_4"), tc.reference("views_4"))
        with pytest.raises(mvs_amd.MvsError, match=r"error -1\b"):
            ctx.triangulate(flows, c["main"], sides, c["depth"])
        tc.compare_rows(_run(ctx, "views_32"), tc.reference("views_32"))
    assert small["W"] == W and small["H"] == H
