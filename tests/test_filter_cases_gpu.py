"""The crafted clouds of tests/filter_clouds.py on the GPU: mvs_filter_points' kept set AND the densities it ranked by
(mvs_filter_density_fetch) equal the oracle exactly -- NaNs in the same places -- on every case, on both orderings of the neighbour
lists, through the host fallback of the greedy pass, and on a context that has run other clouds and another stage in between.
tests/test_filter_cases_cpu.py proves on the CPU what each case is there for."""
import numpy as np
import pytest

import filter_clouds as fc
import mvs_amd

pytestmark = pytest.mark.gpu

ESTATE = -3
HOOKS = ("MVS_FILTER_SORTED_LISTS", "MVS_FILTER_MAX_ROUNDS", "MVS_FILTER_TIMING")
_ref = {}


def _oracle(oracle, case):
    if case.name not in _ref:
        keep, dens = oracle.filter_points(case.points, case.alpha)
        keep.setflags(write=False)
        dens.setflags(write=False)
        _ref[case.name] = (keep, dens)
    return _ref[case.name]


def _context(monkeypatch, sorted_lists=None, **env):
    """hooks are read when the context is created (the master switch is set by conftest)"""
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    if sorted_lists is not None:
        monkeypatch.setenv("MVS_FILTER_SORTED_LISTS", sorted_lists)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return mvs_amd.Context(70, 50)


def _assert_exact(got_keep, got_dens, ref, what):
    keep, dens = ref
    np.testing.assert_array_equal(got_keep, keep, err_msg=what)
    assert got_dens.dtype == np.float32 and got_dens.shape == dens.shape, what
    nan = np.isnan(dens)
    np.testing.assert_array_equal(np.isnan(got_dens), nan, err_msg=what)
    np.testing.assert_array_equal(got_dens[~nan].view(np.uint32), dens[~nan].view(np.uint32), err_msg=what)


@pytest.mark.parametrize("sorted_lists", [None, "0", "1"], ids=["auto", "insertion", "global_sort"])
@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c.name)
def test_case_equals_the_oracle(oracle, monkeypatch, case, sorted_lists):
    ref = _oracle(oracle, case)
    with _context(monkeypatch, sorted_lists) as ctx:
        keep = ctx.filter_points(case.points, case.alpha)
        dens = ctx.filter_density()
        _assert_exact(keep, dens, ref, case.name)
        _assert_exact(ctx.filter_points(case.points, case.alpha), ctx.filter_density(), ref, case.name + " (second call)")


@pytest.mark.parametrize("sorted_lists", [None, "0", "1"], ids=["auto", "insertion", "global_sort"])
def test_chain_is_finished_on_the_host(oracle, monkeypatch, capfd, sorted_lists):
    """the chain case's dependency chain is longer than 8 rounds and all of it sits in one wavefront (a round decides one level of it):
    with MVS_FILTER_MAX_ROUNDS=8 the host walk must have run, and the result is still the oracle's"""
    case = fc.by_name("chain")
    with _context(monkeypatch, sorted_lists, MVS_FILTER_MAX_ROUNDS="8", MVS_FILTER_TIMING="1") as ctx:
        capfd.readouterr()
        keep = ctx.filter_points(case.points, case.alpha)
        err = capfd.readouterr().err
        assert "finished on the host after 8 rounds" in err, err[-1500:]
        _assert_exact(keep, ctx.filter_density(), _oracle(oracle, case), "chain through the host walk")


def _by_size(reverse):
    return sorted(fc.cases(), key=lambda c: (len(c.points), c.name), reverse=reverse)


@pytest.mark.parametrize("largest_first", [True, False], ids=["largest_first", "largest_last"])
def test_one_context_for_every_case_with_a_flow_call_in_between(oracle, monkeypatch, largest_first):
    """buffers grow, shrink in use and are shared with other stages (the filter's work arrays sit in the flow stage's arena): every result
    on the reused context equals that of a fresh one -- the oracle's, by test_case_equals_the_oracle -- and the densities outlive a
    Farneback flow call, which rewrites that arena"""
    rng = np.random.default_rng(5)
    prev = rng.integers(0, 256, (50, 70), dtype=np.uint8)
    nxt = np.roll(prev, 1, axis=1)
    with _context(monkeypatch) as ctx, _context(monkeypatch) as other:
        flow_ref = other.flow(prev, nxt, True)
        for case in _by_size(largest_first):
            ref = _oracle(oracle, case)
            keep = ctx.filter_points(case.points, case.alpha)
            _assert_exact(keep, ctx.filter_density(), ref, case.name)
            np.testing.assert_array_equal(ctx.flow(prev, nxt, True), flow_ref)
            _assert_exact(keep, ctx.filter_density(), ref, case.name + " (after a flow call)")


def test_density_fetch_states(monkeypatch):
    case = fc.by_name("path4")
    buf = np.empty(8, np.float32)
    ptr = buf.ctypes.data_as(mvs_amd._fp)
    with _context(monkeypatch) as ctx:
        fetch, count = ctx.lib.mvs_filter_density_fetch, ctx.lib.mvs_filter_density_count
        assert fetch(ctx.h, ptr) == ESTATE and count(ctx.h) == 0    # before any filter call
        ctx.filter_points(case.points, case.alpha)
        assert fetch(ctx.h, ptr) == 0 and count(ctx.h) == 4 and count(None) == 0
        assert fetch(ctx.h, None) == -1 and fetch(ctx.h, ptr) == 0   # a refused fetch changes nothing
        with pytest.raises(mvs_amd.MvsError):
            ctx.filter_points(case.points, 0.0)                 # a failed call
        assert fetch(ctx.h, ptr) == ESTATE and count(ctx.h) == 0
        with pytest.raises(mvs_amd.MvsError):
            ctx.filter_density()
        keep = np.empty(4, np.int32)                            # the C function called directly: the wrapper takes N from the library
        kept = mvs_amd.C.c_int(0)
        pts = np.ascontiguousarray(case.points[:3])
        assert ctx.lib.mvs_filter_points(ctx.h, pts.ctypes.data_as(mvs_amd._fp), 3, 1.0, keep.ctypes.data_as(mvs_amd._i32p), mvs_amd.C.byref(kept)) == 0
        assert count(ctx.h) == 3 and ctx.filter_density().shape == (3,)
        assert len(ctx.filter_points(np.zeros((0, 4), np.float32), 1.0)) == 0   # N = 0
        assert fetch(ctx.h, ptr) == ESTATE
