"""The guide-gated windows' contract without a GPU: what the crafted guide of tests/gated_cases.py holds, asserted on
the mirror (tests/gated_mirror.py); the mirror against a loop at hand-picked cells; the identities (tau 255 and a constant guide are the
ungated sweep, gate 255 is the ungated propagation, two runs are one); and the figures of section 26's tables, which are deterministic
integer and one-rounding arithmetic on committed scene code and must reproduce to the printed digits."""
import numpy as np
import pytest

import bestk_cases as bk
import bestk_mirror as bm
import gated_cases as gc
import gated_mirror as gm
import propagate_cases as pc
import propagate_mirror as pm
from mvs_amd import Context, load_library

# the device-side counterparts of the mirror: a tree without the feature fails here
DEVICE_ENTRIES = (Context.sweep_run_bestk_gated, Context.propagate_set_gate, load_library().mvs_sweep_run_bestk_gated, load_library().mvs_propagate_set_gate)

ABSDIFF, ZNCC, KEEP_ALL, TAU = gc.ABSDIFF, gc.ZNCC, gc.KEEP_ALL, gc.TAU


def _stacked(cost, r, tau, guide="crafted"):
    per_view = [gc.crafted_view(cost, r, tau, guide, v) for v in range(bk.Crafted.V)]
    return np.stack([p[0] for p in per_view]), np.stack([p[1] for p in per_view]).astype(np.int64)


def test_the_crafted_guide_is_what_it_says():
    g, c = gc.crafted_guide(), gc.crafted()
    assert g.shape == (c.H, c.W) and set(np.unique(g)) == set(gc.LEVELS) | {gc.LONE}
    d = np.abs(np.diff(np.asarray(gc.LEVELS)))
    assert set(d) == {TAU, TAU + 1}                                  # members sit on the <=, and one beyond it
    h = np.abs(np.diff(g.astype(int), axis=1))
    assert (h == TAU).any() and (h == TAU + 1).any()
    # borders on the tile seams, inside tiles and at the frame's edge
    assert (g[:, 31] != g[:, 32]).all() and (g[:, 63] != g[:, 64]).all() and (g[15] != g[16]).all()
    assert (g[:, 68] != g[:, 69]).all() and (g[17] != g[18]).all() and (g[:, 4] != g[:, 5]).any() and (g[8] != g[9]).all()
    assert (c.main_img[2:9, 5:14] == 77).all()                        # the blocks (2..8, 5..13) coincide with the main image's constant block


@pytest.mark.parametrize("r", (1, 2, 4))
def test_crafted_case_holds_what_it_is_for(r):
    c = gc.crafted()
    gate, every = gc.crafted_gate("crafted", TAU, r), gc.crafted_gate("crafted", 255, r)
    out = 1.0 - gate.sum() / every.sum()                             # (pixel, member) pairs inside the frame that the gate takes out
    alone = gate.sum(0) == 1
    print("r = %d: %.1f %% of the (pixel, member) pairs gated out at tau %d, %d pixels whose window is the centre alone" % (r, 100 * out, TAU, alone.sum()))
    assert 0.20 <= out <= 0.80
    assert alone.sum() >= 1 and all(alone[p] for p in gc.LONE_AT)
    # views dropped only because the gate left the main image or the warped frame without variance: ok(p), counted without the gate
    counted, _ = _stacked(ZNCC, r, TAU)
    ungated, _ = _stacked(ZNCC, r, 255)
    starved = ungated & ~counted
    print("r = %d: %.2f %% of the (view, plane, pixel) cells lose their view to va = 0 or vb = 0 under the gate" % (r, 100 * starved.mean()))
    assert (counted <= ungated).all() and starved.mean() >= 0.01
    for cost in (ABSDIFF, ZNCC):
        counted, _ = _stacked(cost, r, TAU)
        # every view range the device tests run holds cells with fewer counted views than a keep they run (8) and with more (1).  The main
        # camera's views 3 and 4 are in frame everywhere, so under the absolute difference a range that holds them has n >= 1 or 2 by
        # construction: as in section 22's test, each of n = 0, 0 < n < 2 and n > 2 must hold 1 % of the cells of one of the ranges
        shares = {}
        for first, count in gc.RANGES:
            n = counted[first:first + count].sum(0)
            print("%s r = %d, views [%d, %d): %s %% of the cells with n = 0 .. %d" % (
                gc.NAMES[cost], r, first, first + count, " ".join("%.1f" % (100 * (n == i).mean()) for i in range(count + 1)), count))
            assert ((n > 0) & (n < 8)).any() and (n > 1).any(), (cost, r, first, count)
            for name, share in (("n = 0", (n == 0).mean()), ("0 < n < keep", ((n > 0) & (n < 2)).mean()), ("n > keep", (n > 2).mean())):
                shares[name] = max(shares.get(name, 0.0), float(share))
        assert all(v >= 0.01 for v in shares.values()), (cost, shares)
        assert counted.sum(0).max() == bk.Crafted.V and c.D == counted.shape[1]


@pytest.mark.parametrize("cost,r", gc.COST_RADII)
def test_mirror_against_a_loop(oracle, cost, r):
    c, guide = gc.crafted(), gc.crafted_guide()
    z = c.planes(oracle)
    counted, costs = _stacked(cost, r, TAU)
    others = np.where(counted[[1, 2, 4]], costs[[1, 2, 4]], 1 << 30).min(0)
    tie = tuple(np.argwhere(counted[0] & counted[3] & (costs[0] > 0) & (costs[0] < others))[0])    # views 0 and 5 tie behind the identity view
    # the frame's corners, both sides of a guide border inside a tile and on the seams, two centre-only windows, the tie
    cells = [(0, 0, 0), (3, 0, c.W - 1), (5, c.H - 1, 0), (c.D - 1, c.H - 1, c.W - 1), (2, 8, 13), (2, 9, 14), (4, 15, 31), (4, 16, 32), (1, 12, 32), (6, 5, 27), tie]
    for d, row, col in cells:
        for keep in (1, 2, 8, KEEP_ALL):
            per_view, cell = gm.brute_cell(oracle, cost, *c.views(), z[d], r, keep, TAU, guide, row, col)
            assert [p[1] for p in per_view] == [bool(x) for x in counted[:, d, row, col]], (d, row, col)
            assert [p[2] for p in per_view] == [int(x) for x in costs[:, d, row, col]], (d, row, col)
            assert cell == int(gc.crafted_volume(cost, r, keep, TAU)[d, row, col]), (d, row, col, keep)
    for d, row, col in ((1, 12, 32), (6, 5, 27)):                     # centre alone: one member at the most, ZNCC has no variance
        per_view = gm.brute_cell(oracle, cost, *c.views(), z[d], r, 2, TAU, guide, row, col)[0]
        assert max(p[0] for p in per_view) == 1 and (cost == ABSDIFF or not any(p[1] for p in per_view))
    d, row, col = tie
    assert int(gc.crafted_volume(cost, r, 2, TAU)[tie]) == (2 << 24) + costs[0, d, row, col] and costs[5, d, row, col] == costs[0, d, row, col]
    # the main image as the guide, tau 0, and a view range
    for d, row, col in cells[:6]:
        assert gm.brute_cell(oracle, cost, *c.views(), z[d], r, 2, 0, None, row, col)[1] == int(gc.crafted_volume(cost, r, 2, 0, "main")[d, row, col])
        assert gm.brute_cell(oracle, cost, *c.views(), z[d], r, 2, TAU, guide, row, col, views=range(1, 4))[1] == int(gc.crafted_volume(cost, r, 2, TAU, "crafted", (1, 2, 3))[d, row, col])


@pytest.mark.parametrize("cost,r", gc.COST_RADII)
def test_identity_tau_255_and_a_constant_guide_are_the_ungated_sweep(oracle, cost, r):
    for keep in gc.KEEPS:
        ungated = bk.crafted_volume(cost, r, keep)
        np.testing.assert_array_equal(gc.crafted_volume(cost, r, keep, 255, "crafted"), ungated)
        np.testing.assert_array_equal(gc.crafted_volume(cost, r, keep, 255, "main"), ungated)
        np.testing.assert_array_equal(gc.crafted_volume(cost, r, keep, 0, "constant"), ungated)
        np.testing.assert_array_equal(gc.crafted_volume(cost, r, keep, TAU, "constant", (1, 2, 3)), bk.crafted_volume(cost, r, keep, (1, 2, 3)))
    assert (gc.crafted_volume(cost, r, KEEP_ALL, TAU) != bk.crafted_volume(cost, r, KEEP_ALL)).mean() >= 0.2     # and the crafted gate is none of them
    c = gc.crafted()
    np.testing.assert_array_equal(gm.volume(oracle, cost, *c.views(), c.D, c.Z_LO, c.Z_HI, r, 2, 255), bm.volume(oracle, cost, *c.views(), c.D, c.Z_LO, c.Z_HI, r, 2))


@pytest.mark.parametrize("cost,r", ((ABSDIFF, 1), (ZNCC, 2), (ZNCC, 4)))
def test_propagation_gate_255_is_the_ungated_propagation(oracle, cost, r):
    c = pc.crafted()
    keep, slopes, nrandom = pc.VARIANTS[1]
    ungated = pc.crafted_states(cost, r, keep, slopes, nrandom)[1]
    for guide in (None, gc.crafted_guide()):
        state = pm.State(gm.Scene(oracle, *c.views(), tau=255, guide=guide), c.prior, cost, r, keep, slopes=slopes, max_step=pc.MAX_STEP)
        for shot in ungated:
            for a, b in zip(pc.snapshot(state)[:5], shot[:5]):
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
            assert tuple(state.report()) == shot[5]
            state.run(1, pc.DZ, pc.DG, nrandom, pc.SEED)


@pytest.mark.parametrize("cost,r", ((ABSDIFF, 1), (ZNCC, 2)))
def test_gated_propagation_two_runs_are_one_and_matches_a_loop(oracle, cost, r):
    c, guide = pc.crafted(), gc.crafted_guide()
    keep, slopes, nrandom = 2, True, 2
    scene = gm.Scene(oracle, *c.views(), tau=TAU, guide=guide)
    twice = pm.State(scene, c.prior, cost, r, keep, slopes=slopes, max_step=pc.MAX_STEP)
    init = pc.snapshot(twice)
    twice.run(1, pc.DZ, pc.DG, nrandom, pc.SEED).run(1, pc.DZ, pc.DG, nrandom, pc.SEED)
    once = pm.State(scene, c.prior, cost, r, keep, slopes=slopes, max_step=pc.MAX_STEP).run(2, pc.DZ, pc.DG, nrandom, pc.SEED)
    for a, b in zip(pc.snapshot(twice)[:5], pc.snapshot(once)[:5]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert twice.report() == once.report()
    ungated = pc.crafted_states(cost, r, keep, slopes, nrandom)[1][0]
    assert (init[3] != ungated[3]).mean() >= 0.1                     # the gate changes the cells
    z, gx, gy, cells = init[:4]
    for row, col in ((0, 0), (c.H - 1, c.W - 1), (8, 13), (9, 14), (15, 31), (16, 32), (12, 32), (10, 40)):
        if not pm.inside(z[row, col]):
            assert cells[row, col] == 0
            continue
        assert gm.brute_prop_cell(oracle, cost, *c.views(), z[row, col], gx[row, col], gy[row, col], r, keep, TAU, guide, row, col)[1] == int(cells[row, col]), (row, col)


# section 26's tables, bad % of the image / of the edge pixels, winner-take-all, r = 2: {(scene, cost, D): {keep: {tau: (image, edge)}}}
SWEEP_TABLE = {
    ("occluder", ZNCC, 48): {KEEP_ALL: {255: (5.33, 22.14), 60: (5.03, 20.60), 30: (2.88, 10.57), 15: (1.89, 4.85)},
                             2: {255: (2.34, 6.16), 60: (2.03, 4.91), 30: (1.71, 3.60), 15: (1.98, 4.35)}},
    ("occluder", ABSDIFF, 64): {KEEP_ALL: {255: (1.48, 5.12), 60: (1.17, 4.35), 30: (0.97, 3.45), 15: (1.27, 3.81)},
                                2: {255: (1.00, 1.85), 60: (0.79, 1.37), 30: (0.74, 1.34), 15: (0.78, 1.37)}},
    ("contrast", ZNCC, 48): {KEEP_ALL: {255: (6.00, 26.04), 60: (2.89, 13.69), 30: (2.88, 13.63), 15: (2.02, 9.58)},
                             2: {255: (2.08, 7.71), 60: (0.04, 0.00), 30: (0.04, 0.00), 15: (0.04, 0.00)}},
    ("contrast", ABSDIFF, 64): {KEEP_ALL: {255: (13.84, 50.15), 60: (13.79, 50.00), 30: (13.79, 50.03), 15: (13.73, 49.70)},
                                2: {255: (2.79, 5.89), 60: (0.31, 0.00), 30: (0.31, 0.00), 15: (0.31, 0.00)}},
}


@pytest.mark.parametrize("name,cost,D", sorted(SWEEP_TABLE))
def test_sweep_figures_of_section_26(oracle, name, cost, D):
    s = gc.scene(name)
    if name == "contrast":
        means = s.main_img[s.front].mean(), s.main_img[~s.front].mean()
        print("contrast scene: the main image's means are %.1f on the rectangle and %.1f off it" % means)
        assert round(means[0]) == 200 and round(means[1]) == 61
    got = {}
    for keep, row in SWEEP_TABLE[name, cost, D].items():
        for tau in row:
            got[keep, tau] = gc.wta_shares(oracle, name, gc.scene_volume(name, cost, 2, D, keep, tau), D)
            print("%s, %s, %d planes, keep %s, tau %3d: %5.2f / %5.2f (section 26: %5.2f / %5.2f)" % (
                (name, gc.NAMES[cost], D, "all" if keep == KEEP_ALL else keep, tau) + got[keep, tau] + row[tau]))
    # tau 255 is today's sweep
    for keep in SWEEP_TABLE[name, cost, D]:
        if name == "occluder":
            np.testing.assert_array_equal(gc.scene_volume(name, cost, 2, D, keep, 255), bk.occluder_volume(cost, 2, D, keep))
    for (keep, tau), shares in got.items():
        if tau != 15:                                                # the tau-15 row is printed, not asserted
            assert tuple(round(x, 2) for x in shares) == SWEEP_TABLE[name, cost, D][keep][tau], (keep, tau, shares)
    if name == "contrast":
        assert got[2, 30][1] <= 0.5 * got[2, 255][1]                 # measured: 0.00 against 7.71 (ZNCC) and against 5.89 (absolute difference)
    elif cost == ZNCC:
        assert got[KEEP_ALL, 30][1] < got[KEEP_ALL, 255][1]         # measured: 10.57 against 22.14


# section 26's propagation table: {scene: (start, ungated no random, ungated random, tau 30 no random, tau 30 random)}
PROP_TABLE = {"occluder": ((2.39, 6.25), (2.61, 6.88), (4.19, 9.70), (1.85, 4.02), (2.97, 5.60)),
              "contrast": ((2.03, 7.20), (2.14, 7.56), (3.76, 9.49), (0.06, 0.00), (0.02, 0.00))}


@pytest.mark.parametrize("name", sorted(PROP_TABLE))
def test_propagation_figures_of_section_26(oracle, name):
    """ZNCC r = 2, keep 2, from the UNGATED 16-plane refined map, 3 iterations; bad: more than 1.5 steps of a 48-plane table off"""
    rows = [("the start", gc.propagation_start(name)), ("ungated, no random", gc.propagated(name, 255, False)), ("ungated, random", gc.propagated(name, 255, True)),
            ("tau 30, no random", gc.propagated(name, 30, False)), ("tau 30, random", gc.propagated(name, 30, True))]
    got = [gc.bad_shares(oracle, name, z, 48) for _, z in rows]
    for (label, _), shares, doc in zip(rows, got, PROP_TABLE[name]):
        print("%s: %-20s %5.2f / %5.2f (section 26: %5.2f / %5.2f)" % ((name, label) + shares + doc))
    z15 = gc.propagated(name, 15, False)
    print("%s: %-20s %5.2f / %5.2f (printed, not asserted)" % ((name, "tau 15, no random") + gc.bad_shares(oracle, name, z15, 48)))
    for shares, doc in zip(got, PROP_TABLE[name]):
        assert tuple(round(x, 2) for x in shares) == doc
    if name == "contrast":
        assert got[3][1] <= 0.5 * got[0][1]                          # measured: 0.00 against 7.20
    else:
        assert got[3][1] < got[0][1]                                 # measured: 4.02 against 6.25
