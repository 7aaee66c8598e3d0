"""The deferred chunk epilogue of the rectified-view kernel (csrc/sweep_rect.hip): a chunk's cost volume stores and depth selection run
one turn late -- behind the barrier and the copy issue of the next chunk's first region -- and the workgroup's last chunk is finished
behind the region loop.  sweep_fx_rect against the general kernel (MVS_SWEEP_NO_RECT) and the oracle, every cell of volume, depth, best
cost and index, all three variants (volume + fused, fused only, volume only), on the smallest shapes at which a deferred epilogue can go
wrong and that tests/test_rect_turn_gpu.py does not pin.  Every frame is 200 x 52: a ragged last tile column (8 of 64 columns) and a
ragged last tile row (4 of 8 rows), so the checked-rows and the col_ok forms of the epilogue are deferred ones too.

  * one view, four chunks in one workgroup: every turn ends a chunk, so every turn but the first runs a deferred epilogue in front of
    its sampling, and the last chunk is finished behind the loop;
  * exactly one chunk per workgroup (forced split 4 of 4 chunks): no turn ever runs an epilogue, only the lines behind the loop store;
  * a ragged last chunk (40 planes: chunks of 16, 16 and 8) in one workgroup, and in two (shares of 2 chunks and 1);
  * the switch from the plain to the cross-multiplied depth comparison while chunks are deferred: a ring whose plan has both clean
    regions and border planes.  On a ring the shift against the main view falls with the plane index, so a plane that is partly out
    of frame lies in a tile's FIRST chunks (test_plain_switch_case_has_full_and_border_chunks shows it from the oracle's counts): a
    workgroup whose first chunk is all FULL leaves the plain comparison later only through a failed certificate (they fall on any
    plane; the planner's share of them is printed), or not at all.  The frame has workgroups that never leave it and workgroups
    that leave it in their first chunk, so that every later chunk's deferred epilogue is the cross-multiplied one;
  * launches back to back on one context, each with other flags, under a forced split: no pending epilogue, accumulator or count may
    leak from one launch into the next, and the partial bests of the split must still merge.
"""
import numpy as np
import pytest

import mvs_amd
from mvs_amd import synth
from test_rect_turn_gpu import BOTH, FUSED, NO_RECT, VOL, _plan, _same

pytestmark = pytest.mark.gpu

W, H = 200, 52

CASES = {
    # name: (D, V, radius, forced plane split)
    "one_view_every_turn_ends_a_chunk": (64, 1, 0.1, 1),
    "one_chunk_per_workgroup": (64, 3, 0.1, 4),
    "ragged_last_chunk": (40, 2, 0.1, 1),
    "ragged_last_chunk_shares_2_and_1": (40, 2, 0.1, 2),
    "plain_switch_under_deferral": (64, 3, 0.15, 1),
}

_reference = {}


def _views(name):
    D, V, radius, split = CASES[name]
    return synth.make_views(W, H, V, radius=radius, freq_scale=0.5)


def _oracle_of(oracle, name):
    """the oracle's (depth, cost, index, volume) of a case: computed once, shared, never written to"""
    if name not in _reference:
        D, V, radius, split = CASES[name]
        main_cam, main_img, side_cams, sides, _ = _views(name)
        ref = oracle.sweep(main_cam, main_img, side_cams, sides, D, want_volume=True, nthreads=8, sampler="fixed")
        for a in ref:
            a.setflags(write=False)
        _reference[name] = ref
    return _reference[name]


def _equals_oracle(got, ref, what):
    for g, r, name in zip(got, ref, ("depth", "cost", "index", "volume")):
        if g is None:
            continue
        bad = np.count_nonzero(g != r)
        assert bad == 0, "%s against the oracle, %s: %d of %d differ" % (what, name, bad, r.size)


@pytest.mark.parametrize("name", sorted(CASES))
def test_deferred_epilogue_equals_general_and_oracle(oracle, monkeypatch, capfd, name):
    monkeypatch.setenv("MVS_RECT_VERBOSE", "1")
    D, V, radius, split = CASES[name]
    main_cam, main_img, side_cams, sides, _ = _views(name)
    extra = split << 16
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH | NO_RECT)
        gen = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_run(0, V, BOTH | extra)
        assert ctx.plan_shape() == 4, "the ring geometry should take the rectified kernel"
        both = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_run(0, V, FUSED | extra)
        fused = ctx.sweep_fetch(want_volume=False)[:3]
        ctx.sweep_run(0, V, VOL | extra)
        vol = ctx.sweep_fetch(want_volume=True)[3]
    plan = _plan(capfd.readouterr().err)
    print(name, plan)
    if name == "plain_switch_under_deferral":
        border = plan["left"] + plan["right"] + plan["top"] + plan["bottom"]
        print("failed certificates: %.3f %% of the planes" % plan["flagged"])
        assert plan["clean"] > 0.0 and border > 0.0, "the case is not what it is there for: %s" % plan
    ref = _oracle_of(oracle, name)
    _same(both, gen, "volume + fused")
    _same(fused, gen[:3], "fused only")
    _same((None, None, None, vol), gen, "volume only")
    _equals_oracle(both, ref, "volume + fused")
    _equals_oracle(fused, ref[:3], "fused only")
    _equals_oracle((None, None, None, vol), ref, "volume only")


def test_plain_switch_case_has_full_and_border_chunks(oracle):
    """what the oracle's counts say about the plain-switch case (a cell's count is its top byte): some tile is FULL -- every cell counts
    every view -- on all its planes, some tile only from a later chunk on, and no tile is FULL in its first chunk and not in a later one"""
    name = "plain_switch_under_deferral"
    D, V, radius, split = CASES[name]
    full = (_oracle_of(oracle, name)[3] >> 24) == V
    always, later, first_only = 0, 0, 0
    for y in range(0, H, 8):
        for x in range(0, W, 64):
            chunks = [bool(full[c:c + 16, y:y + 8, x:x + 64].all()) for c in range(0, D, 16)]
            always += all(chunks)
            later += (not chunks[0]) and chunks[-1]
            first_only += chunks[0] and not all(chunks)
    assert always > 0 and later > 0 and first_only == 0, (always, later, first_only)


def test_launches_back_to_back_with_other_flags(oracle):
    """volume + fused, then volume only, then fused only, then volume + fused again on one context, two workgroups per tile"""
    name = "one_chunk_per_workgroup"
    D, V, radius, split = CASES[name]
    main_cam, main_img, side_cams, sides, _ = _views(name)
    ref = _oracle_of(oracle, name)
    extra = 2 << 16
    with mvs_amd.Context(W, H, sampler="fixed") as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, BOTH | NO_RECT)
        gen = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_run(0, V, BOTH | extra)
        assert ctx.plan_shape() == 4
        first = ctx.sweep_fetch(want_volume=True)
        ctx.sweep_run(0, V, VOL | extra)
        vol = ctx.sweep_fetch(want_volume=True)[3]
        ctx.sweep_run(0, V, FUSED | extra)
        fused = ctx.sweep_fetch(want_volume=False)[:3]
        ctx.sweep_run(0, V, BOTH | extra)
        again = ctx.sweep_fetch(want_volume=True)
    for got, what in ((first, "volume + fused"), ((None, None, None, vol), "volume only"), (fused, "fused only"), (again, "volume + fused again")):
        _same(got, gen, what)
        _equals_oracle(got, ref, what)
