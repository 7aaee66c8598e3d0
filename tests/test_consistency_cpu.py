"""The geometric term of the propagation on the CPU: the crafted case's premise (every clause of rule 5 fails
somewhere and holds somewhere, inside one tile), the mirror (tests/consistency_mirror.py) against the scalar restatement on every pixel,
the identities that need no device (no neighbours = the photometric stage; weight 0 = the same maps with a support map; the third, a
setter between init and run, is a statement about the context and lives in tests/test_consistency_gpu.py), rule 7's bound at the largest
admitted parameters, and two comparisons on section 22's occluder scene.

Figures of one run (the mirror; bad = more than 1.5 steps of a 48-plane table off; whole image / edge pixels, %), printed by the tests:
start 2.39 / 6.25, photometric 2.61 / 6.88, analytic neighbours at weight 10: 1.37 / 3.39, estimated neighbours at weight 10: 2.31 / 5.74."""
import numpy as np
import pytest

import consistency_cases as cc
import consistency_mirror as cm
import gated_cases as gc
import propagate_mirror as pm

f32 = np.float32
ZNCC, ABSDIFF, KEEP_ALL = cc.ZNCC, cc.ABSDIFF, cc.KEEP_ALL


def test_every_clause_fails_and_holds_somewhere():
    frame, tile, per = cc.clause_counts()
    print(dict(zip(cm.CLAUSES, frame.tolist())), dict(zip(cm.CLAUSES, tile.tolist())))
    assert (frame > 0).all() and (tile > 0).all(), (frame, tile)
    # each clause's own neighbour: it fails there and the neighbour answers elsewhere (slot 3 faces away: never)
    for j, clause in ((1, cm.FAR), (2, cm.OUTSIDE), (4, cm.BACK_BEHIND), (5, cm.INVALID)):
        assert per[j][clause] > 0 and per[j][cm.ANSWERS] > 0, (j, per[j])
    assert per[3][cm.BEHIND] == per[3].sum() and per[0][cm.FAR] == 0
    assert (per[6] == per[0]).all() and (per[7] == per[2]).all()               # the slots listed twice
    # the start map has pixels without a hypothesis on both sides of the seams
    c = cc.crafted()
    assert not pm.inside(c.start[15, 31]) and not pm.inside(c.start[16, 32]) and not pm.inside(c.start[18, 69])


@pytest.mark.parametrize("offset", (0.0, 0.11, -0.3))
def test_the_mirror_equals_the_scalar_restatement(offset):
    c = cc.crafted()
    term = c.term()
    z = (c.start + f32(offset)).astype(f32)
    rows, cols = np.nonzero(pm.inside(z))
    g, answers, clause, _ = term.evaluate(rows, cols, z[rows, cols], c.H, c.W)
    main = (term.M, term.Mi)
    seen = set()
    for i, (row, col) in enumerate(zip(rows, cols)):
        bg, ba, detail = cm.brute_term(main, term.neighbours, cc.WEIGHT, cc.MAX_PX, c.W, c.H, int(row), int(col), z[row, col])
        assert (bg, ba, [d[0] for d in detail]) == (int(g[i]), int(answers[i]), clause[i].tolist()), (row, col)
        seen.update(d[0] for d in detail)
    assert offset != 0.0 or seen == set(range(6))


def test_no_neighbours_is_the_photometric_stage(oracle):
    c = cc.crafted()
    for cost, r, keep in ((ZNCC, 1, 2), (ABSDIFF, 2, KEEP_ALL)):
        plain = pm.State(cc.scene(oracle), c.start, cost, r, keep)
        off = cc.shots(cost, r, keep, slots=())
        for k in range(3):
            if k:
                plain.run(1, cc.DZ, cc.DG, 2, cc.SEED)
            for a, b in zip(cc.pc.snapshot(plain)[:5], off[k][:5]):
                assert a.tobytes() == b.tobytes()
            assert tuple(plain.report()) == off[k][5] and not off[k][6].any()


def test_weight_zero_changes_the_support_map_only():
    for cost, r, keep in ((ZNCC, 1, 2), (ABSDIFF, 2, KEEP_ALL)):
        off, zero, on = cc.shots(cost, r, keep, slots=()), cc.shots(cost, r, keep, weight=0.0), cc.shots(cost, r, keep)
        for k in range(3):
            for a, b in zip(zero[k][:5], off[k][:5]):
                assert a.tobytes() == b.tobytes()
            assert zero[k][5] == off[k][5] and zero[k][6].any() and zero[k][6].max() <= len(cc.SLOTS)
        assert (on[2][3] != off[2][3]).any() and (on[2][0] != off[2][0]).any(), "the crafted weight changes cells and depths"


def test_support_counts_the_held_hypotheses_neighbours():
    c = cc.crafted()
    shot = cc.shots(ZNCC, 1, 2)[2]
    z, support = shot[0], shot[6]
    assert (support[~pm.inside(z)] == 0).all()
    term = c.term()
    for row, col in ((0, 0), (3, 11), (9, 21), (15, 30), (16, 33), (18, 68), (7, 45)):
        assert support[row, col] == cm.brute_term((term.M, term.Mi), term.neighbours, cc.WEIGHT, cc.MAX_PX, c.W, c.H, row, col, z[row, col])[1]


def test_rule_7s_bound_at_the_largest_admitted_parameters(oracle):
    max_px = f32(3.0)
    weight = f32(cm.MAX_PENALTY / (3.0 * 255.0))
    while cm.admitted(np.nextafter(weight, f32(np.inf)), max_px):
        weight = np.nextafter(weight, f32(np.inf))
    while not cm.admitted(weight, max_px):
        weight = np.nextafter(weight, f32(0.0))
    cap = int(np.floor(max_px * cm.w255(weight)))
    assert cap <= cm.MAX_PENALTY < int(np.floor(max_px * cm.w255(np.nextafter(weight, f32(np.inf))))) and cap > cm.MAX_PENALTY - 16
    assert 8 * (65025 + cap) < 1 << 24 <= 16 * (65025 + cap)
    for bad in ((-1.0, 1.0), (np.nan, 1.0), (np.inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.inf), (1.0, np.nan)):
        assert not cm.admitted(*bad)
    # every neighbour at the cap, eight kept views at ZNCC's top of the scale: the sums still fit (State._eval asserts it per cell)
    c = cc.crafted()
    state = cm.State(cc.scene(oracle), c.start, ZNCC, 1, 8, term=c.term(slots=(3,) * 8, weight=weight, max_px=max_px))
    k, s = state.cells >> 24, state.cells & 0xffffff
    assert (k <= 3).all() and (s[k > 0] >= k[k > 0].astype(np.int64) * cap).all() and not state.support().any()


# ---- the occluder scene -----------------------------------------------------------------------------------------------------------------
def _shares(oracle, z):
    return gc.bad_shares(oracle, "occluder", z, 48)


def test_accurate_neighbours_repair_the_edge_pixels(oracle):
    start, photo = _shares(oracle, gc.propagation_start("occluder")), _shares(oracle, gc.propagated("occluder", 255, False))
    z, support = cc.consistent("occluder", "analytic", 10.0)
    got = _shares(oracle, z)
    print("start %.2f / %.2f, photometric %.2f / %.2f, analytic neighbours at weight 10: %.2f / %.2f" % (start + photo + got))
    assert got[1] < start[1] and got[1] < photo[1]
    assert support.max() <= 4 and support.any()


def test_estimated_neighbours_help_a_little(oracle):
    photo = _shares(oracle, gc.propagated("occluder", 255, False))
    got = _shares(oracle, cc.consistent("occluder", "estimated", 10.0)[0])
    print("photometric %.2f / %.2f, estimated neighbours at weight 10: %.2f / %.2f" % (photo + got))
    assert got[1] < photo[1]
