"""mvs_sweep_aggregate on crafted volumes at the edges of its kernels (csrc/aggregate.hip): the volumes of tests/sgm_volumes.py go in through
mvs_sweep_use_volume + mvs_sweep_set_planes, no sweep runs, and S and the depth / cost / index maps are compared bit for bit with the
numpy mirror (tests/sgm_mirror.py), with and without the refinement.  tests/test_aggregate_cpu.py shows without a GPU what every volume
is for; the state tests below cover what the kernels inherit from earlier calls on the same context."""
import numpy as np
import pytest
import torch

import mvs_amd
import sgm_mirror as sgm
import sgm_volumes
from mvs_amd import synth
from test_aggregate_gpu import _compare

pytestmark = pytest.mark.gpu

EINVAL = -1


def inject(ctx, vol, D):
    """make `vol` (uint32 [>= D, H, W]) the context's volume of D planes; the caller keeps the returned tensor alive as long as the context uses it"""
    t = torch.from_numpy(vol.view(np.int32).copy()).cuda()   # a copy: the volumes of sgm_volumes are read-only
    torch.cuda.synchronize()
    ctx.sweep_use_volume(t.data_ptr(), t.numel() * 4)
    ctx.sweep_set_planes(D)
    return t


def _untouched(t, vol):
    return torch.equal(t.cpu(), torch.from_numpy(vol.view(np.int32).copy()))


def _run(ctx, key, vol, sampler, oracle, params, D=None):
    """inject, then compare both ways of the selection for every parameter set; the volume stays what it was"""
    D = vol.shape[0] if D is None else D
    t = inject(ctx, vol, D)
    z = oracle.plane_table(D, -1.0, 1.0)
    out = None
    for paths, p1, p2, cap in params:
        for refine in (False, True):
            out = _compare(ctx, key, vol[:D], sampler, z, paths, p1, p2, cap, refine=refine)
    assert _untouched(t, vol), "the aggregation wrote into the volume"
    return t, out


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in sgm_volumes.CASES])
def test_crafted_volume(oracle, case):
    with mvs_amd.Context(case.W, case.H, 0, sampler=case.sampler) as ctx:
        for key, vol in sgm_volumes.volumes(case):
            t, (S, depth, cost, index) = _run(ctx, key, vol, case.sampler, oracle, case.params)
            if case.gen == "division_edges":   # P1 = P2 = 0: L = C, the cost kernel alone
                paths, _, _, cap = case.params[-1]
                np.testing.assert_array_equal(S, paths * sgm.cost16(vol, sgm_volumes.CS[case.sampler], cap))
            if case.gen == "saturating":
                paths, _, p2, cap = case.params[-1]
                assert int(S.max()) == paths * (cap + p2)
                assert (index == 0).all()
            if case.gen == "noise":
                assert index[sgm_volumes.nobody_sees(case.W, case.H)] == -1 and index[sgm_volumes.one_seen_cell(case.W, case.H)] == 0
            del t


def test_poisoned_allocations(oracle, monkeypatch):
    """nobody zeroes S: the row launch stores and the column launches add, so 0xFF bytes in a fresh S (and C) must not show"""
    monkeypatch.setenv("MVS_POISON_ALLOC", "1")
    W, H, D = 129, 6, 65
    vol = sgm_volumes.noise(W, H, D, 24, 0xA110C)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        _run(ctx, "poison", vol, "fixed", oracle, ((4, 16, 128, 4080), (8, 16, 128, 4080)))


def test_shrinking_and_growing_on_one_context(oracle):
    """fewer planes, fewer paths and back: nothing of the larger call's S, C or maps shows in the smaller one"""
    W, H = 129, 6
    big, small = sgm_volumes.noise(W, H, 65, 24, 0xB16), sgm_volumes.noise(W, H, 9, 24, 0x5A11)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        keep = [_run(ctx, "shrink65", big, "fixed", oracle, (sgm_volumes.STD,))[0]]
        keep.append(_run(ctx, "shrink9", small, "fixed", oracle, ((4, 16, 128, 4080),))[0])
        assert ctx.sweep_aggregate_fetch().shape == (9, H, W)
        ptr, nbytes = ctx.sweep_aggregated_device()
        assert ptr and nbytes == 9 * H * W * 2
        keep.append(_run(ctx, "shrink65", big, "fixed", oracle, (sgm_volumes.STD,))[0])
        assert ctx.sweep_aggregate_fetch().shape == (65, H, W)
        # a smaller part of the same volume: D shrinks, the storage does not
        keep.append(_run(ctx, "shrink65-first17", big, "fixed", oracle, (sgm_volumes.STD,), D=17)[0])


def test_the_callers_volume(oracle):
    W, H, D = 70, 5, 11
    views = synth.make_views(W, H, 2, radius=0.3)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        lib = ctx.lib
        # the context's own volume first, from a sweep
        ctx.sweep_set(views[0], views[1], views[2], views[3], D)
        ctx.sweep_run(0, 2, mvs_amd.MVS_SWEEP_VOLUME)
        own = ctx.sweep_fetch(want_volume=True)[3]
        assert sgm.seen_cells(own, 24).any()
        z = oracle.plane_table(D, -1.0, 1.0)
        _compare(ctx, "own", own, "fixed", z, 8, 16, 128, 4080)
        # storage of D + 3 planes, D of them in use: the rest is not read (it would change S) and not written
        vol = sgm_volumes.noise(W, H, D + 3, 24, 0xCA11)
        t, _ = _run(ctx, "callers", vol, "fixed", oracle, (sgm_volumes.STD,), D=D)
        assert (own != vol[:D]).any()
        # one cell short
        short = t.reshape(-1)[:D * H * W - 1]
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert lib.mvs_sweep_aggregate(ctx.h, 8, 16, 128, 4080, 0) == EINVAL
        assert b"bytes" in lib.mvs_last_error(ctx.h)
        ctx.sweep_use_volume(t.data_ptr(), D * H * W * 4)    # exactly enough
        _compare(ctx, "callers", vol[:D], "fixed", z, 8, 16, 128, 4080)
        assert _untouched(t, vol)
        # and back to its own
        ctx.sweep_use_volume(0, 0)
        _compare(ctx, "own", own, "fixed", z, 8, 16, 128, 4080, refine=True)
        np.testing.assert_array_equal(ctx.sweep_fetch(want_volume=True)[3], own)


def test_stream_order_after_a_sweep(oracle):
    """mvs_sweep_aggregate right behind mvs_sweep_run, nothing that synchronises in between: the aggregation reads the volume the sweep
    is still writing unless the stream orders them"""
    W, H, D = 150, 70, 37
    main_cam, main_img, side_cams, sides = synth.make_views(W, H, 3, radius=0.8)[:4]
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, len(sides), mvs_amd.MVS_SWEEP_VOLUME)
        ctx.sweep_aggregate(8, 16, 128, 4080)
        S = ctx.sweep_aggregate_fetch()
        depth, cost, index, _ = ctx.sweep_fetch()
        vol = ctx.sweep_fetch(want_volume=True)[3]
    seen = sgm.seen_cells(vol, 24)
    assert 0.01 < 1.0 - seen.mean() < 0.5
    S_ref = sgm.aggregate(sgm.cost16(vol, 24, 4080), 8, 16, 128)
    np.testing.assert_array_equal(S, S_ref)
    d_ref, c_ref, i_ref = sgm.select(S_ref, seen, oracle.plane_table(D, -1.0, 1.0), 8)
    np.testing.assert_array_equal(index, i_ref)
    np.testing.assert_array_equal(cost, c_ref)
    np.testing.assert_array_equal(depth, d_ref)
