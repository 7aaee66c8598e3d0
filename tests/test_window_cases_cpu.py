"""The crafted cases of tests/window_cameras.py on the CPU: every case is what it is there for (its premise), no s.w it inverts is outside
what the kernels' reciprocal guarantees, and the oracle entries that the windowed mirrors (zncc_mirror, bestk_mirror, band_mirror,
band_bestk_mirror, gated_mirror, propagate_mirror) take their samples from -- oracle.warp_by_depth(..., sampler="fixed") on constant and on
per-pixel plane maps, oracle.sweep_sample_fx, oracle.sweep and oracle.argmin -- equal tests/sweep_mirror.py on these cases, by exact
equality.  With that the windowed mirrors are independent of oracle/sweep_oracle.c on these cases by transitivity; three of them are
held against the volumes of window_cameras directly, and the brute_cell of each against the array path at the cells the premises name."""
import numpy as np
import pytest

import band_bestk_mirror as bbm
import band_mirror as bm
import bestk_mirror as km
import propagate_mirror as pm
import sweep_mirror as sm
import window_cameras as wc
import zncc_mirror as zm

ABSDIFF, ZNCC, KEEP_ALL = wc.ABSDIFF, wc.ZNCC, wc.KEEP_ALL
F = np.float32


def _distinct_views(c):
    seen = set()
    for v in range(c.V):
        key = (c.cams[v].tobytes(), np.asarray(c.sides[v]).tobytes())
        if key not in seen:
            seen.add(key)
            yield v


@pytest.mark.parametrize("name", [n for n in wc.NAMES if wc.CASES[n].premise])
def test_case_is_what_it_is_there_for(name):
    c = wc.CASES[name]
    c.premise(c)


@pytest.mark.parametrize("name", wc.NAMES)
def test_no_reciprocal_outside_the_newton_steps_guarantee(name):
    """the all-ones condition of sweep_mirror.reciprocal (cap 0), on the plane table and on the band's per-pixel maps"""
    c = wc.CASES[name]
    zs = [c.z()] + ([np.where(c.planes()[1], c.planes()[0], F(0))] if c.prior is not None else [])
    for v in _distinct_views(c):
        for z in zs:
            sw = sm.project(c.q()[v], z, c.W, c.H)[2]
            assert not sm._all_ones(np.where(sw > 0, sw, F(1)).astype(F)).any()
            sm.reciprocal(sw)


@pytest.mark.parametrize("name", wc.NAMES)
def test_view_matrix_has_the_designed_entries(oracle, name):
    c = wc.CASES[name]
    for v in _distinct_views(c):
        np.testing.assert_array_equal(oracle.view_matrix(c.main_cam, c.side_cams[v], c.W, c.H), c.q()[v])


@pytest.mark.parametrize("name", wc.NAMES)
def test_warp_by_depth_equals_the_mirrors_samples(oracle, name):
    """rule 1 of section 21 on constant plane maps: B == (dot + 127) // 255 and ok == valid"""
    c = wc.CASES[name]
    z = c.z()
    assert not (z == F(1.0)).any()
    for v in _distinct_views(c):
        s = wc.samples(name)[v]
        for d in range(c.D):
            out = oracle.warp_by_depth(c.main_cam, np.full((c.H, c.W), z[d], F), c.side_cams[v], np.asarray(c.sides[v], np.uint8), sampler="fixed")
            np.testing.assert_array_equal(out[..., 1] != 0, s["valid"][d], err_msg="%s view %d plane %d: ok" % (name, v, d))
            np.testing.assert_array_equal(np.where(s["valid"][d], out[..., 0], 0), (s["dot"][d] + 127) // 255, err_msg="%s view %d plane %d: B" % (name, v, d))


@pytest.mark.parametrize("name", wc.BANDS)
def test_warp_by_depth_equals_the_mirrors_samples_on_per_pixel_maps(oracle, name):
    """the same on the band cases' maps prior + offset_d, a dead plane given as depth 1.0 (band_bestk_mirror.warped)"""
    c = wc.CASES[name]
    z, live = c.planes()
    for v in range(c.V):
        s = wc.samples(name, band=True)[v]
        for d in range(c.D):
            B, ok = bbm.warped(oracle, c.main_cam, c.side_cams[v], c.sides[v], z[d], live[d])
            np.testing.assert_array_equal(ok, s["valid"][d])
            np.testing.assert_array_equal(np.where(ok, B, 0), (s["dot"][d] + 127) // 255)


@pytest.mark.parametrize("name", [n for n in wc.NAMES if (wc.CASES[n].W, wc.CASES[n].H) == (64, 8)])
def test_sweep_sample_fx_equals_the_mirrors_samples_on_the_border(oracle, name):
    """(ok, dot) of the oracle's single-sample entry on the border rows and columns"""
    c = wc.CASES[name]
    z = c.z()
    border = [(r, col) for r in range(c.H) for col in range(c.W) if r in (0, c.H - 1) or col in (0, c.W - 1)]
    xn = [oracle.lib.orc_pixel_xn(col, c.W) for col in range(c.W)]
    yn = [oracle.lib.orc_pixel_yn(r, c.H) for r in range(c.H)]
    for v in _distinct_views(c):
        s = wc.samples(name)[v]
        q, pad = oracle.view_matrix(c.main_cam, c.side_cams[v], c.W, c.H), oracle.pad_image(np.asarray(c.sides[v], np.uint8))
        for d in range(c.D):
            for r, col in border:
                ok, dot = oracle.sweep_sample_fx(q, xn[col], yn[r], float(z[d]), pad)
                assert bool(ok) == bool(s["valid"][d, r, col]) and (not ok or int(dot) == int(s["dot"][d, r, col])), (name, v, d, r, col)


@pytest.mark.parametrize("name", wc.BANDS)
def test_sweep_sample_fx_equals_the_mirrors_samples_on_the_bands_seams(oracle, name):
    """the same at each pixel's own plane, on the rows and columns beside the seams of both tilings and on the frame's border"""
    c = wc.CASES[name]
    z, live = c.planes()
    rows, cols = (0, 7, 8, 15, 16, 23, 24, c.H - 1), (0, 31, 32, c.W - 1)
    pix = [(r, col) for r in range(c.H) for col in range(c.W) if r in rows or col in cols]
    for v in range(c.V):
        s = wc.samples(name, band=True)[v]
        q, pad = oracle.view_matrix(c.main_cam, c.side_cams[v], c.W, c.H), oracle.pad_image(c.sides[v])
        for d in (0, 7, 15):
            for r, col in pix:
                if live[d, r, col]:
                    ok, dot = oracle.sweep_sample_fx(q, oracle.lib.orc_pixel_xn(col, c.W), oracle.lib.orc_pixel_yn(r, c.H), float(z[d, r, col]), pad)
                    assert bool(ok) == bool(s["valid"][d, r, col]) and (not ok or int(dot) == int(s["dot"][d, r, col])), (v, d, r, col)


@pytest.mark.parametrize("name", wc.NAMES)
def test_oracle_sweep_and_selection_equal_the_mirror(oracle, name):
    """oracle.sweep's one-view cells (the absolute difference's e and ok in bestk_mirror and gated_mirror) and oracle.argmin"""
    c = wc.CASES[name]
    for v in _distinct_views(c):
        s = wc.samples(name)[v]
        one = oracle.sweep(c.main_cam, c.main, c.side_cams[v][None], [c.sides[v]], c.D, -1.0, 1.0, want_volume=True, sampler="fixed")[3]
        want = np.where(s["valid"], (1 << 24) + np.abs(s["dot"] - 255 * c.main.astype(np.int64)[None]), 0)
        np.testing.assert_array_equal(one, want.astype(np.uint32))
    r = 2
    for vol in (wc.bestk_volume(name, ABSDIFF, r, 2 if c.V > 1 else KEEP_ALL), wc.zncc_volume(name, r)):
        for got, want in zip(oracle.argmin(vol, c.z(), sampler="fixed"), wc.maps(vol, c.z())):
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["ladder_int_left", "ladder_tie_bottom", "horizon", "front_x", "few_views"])
def test_the_windowed_mirrors_equal_the_volumes_here(oracle, name):
    c = wc.CASES[name]
    for r in (1, 4):
        np.testing.assert_array_equal(zm.volume(oracle, c.main_cam, c.main, c.side_cams, c.sides, c.z(), r), wc.zncc_volume(name, r))
    for cost, r, keep in ((ABSDIFF, 0, KEEP_ALL), (ABSDIFF, 3, 2), (ZNCC, 2, 2)):
        np.testing.assert_array_equal(km.volume(oracle, cost, c.main_cam, c.main, c.side_cams, c.sides, c.D, -1.0, 1.0, r, keep), wc.bestk_volume(name, cost, r, keep))


@pytest.mark.parametrize("name", wc.BANDS)
def test_the_band_mirrors_equal_the_volumes_here(oracle, name):
    c = wc.CASES[name]
    np.testing.assert_array_equal(bm.band_volume(oracle, c.main_cam, c.main, c.side_cams, c.sides, c.prior, c.z()), wc.band_volume(name))
    for cost, r, keep in ((ABSDIFF, 1, 2), (ZNCC, 4, KEEP_ALL)):
        np.testing.assert_array_equal(bbm.volume(oracle, cost, c.main_cam, c.main, c.side_cams, c.sides, c.prior, c.z(), r, keep),
                                      wc.bestk_volume(name, cost, r, keep, band=True))


def test_propagate_mirrors_sampler_equals_the_mirrors_samples(oracle):
    """propagate_mirror.Scene.sample (its own float32 restatement) on whole plane maps of the three cases it runs on"""
    for name in wc.PROPAGATED:
        c = wc.CASES[name]
        scene = pm.Scene(oracle, *c.views())
        rows, cols = np.indices((c.H, c.W))
        s = wc.samples(name)[0]
        for d in range(c.D):
            ok, dot = scene.sample(0, rows, cols, np.full((c.H, c.W), c.z()[d], F))
            np.testing.assert_array_equal(ok, s["valid"][d])
            np.testing.assert_array_equal(dot, s["dot"][d])


# ---- one cell at a time --------------------------------------------------------------------------------------------------------------
def _named_cells():
    """(case, plane, row, col): the bound plane's border pixels and their neighbours, seam pixels of front_x, a cell of near_saturated"""
    out = []
    for name, edge in (("ladder_int_left", "left"), ("ladder_tie_right", "right"), ("ladder_int_top", "top")):
        c = wc.CASES[name]
        kb, nx, line = wc.bound_planes(c, edge)
        rows, cols = np.nonzero(line)
        for i in (0, len(rows) // 2, len(rows) - 1):
            out += [(name, kb, int(rows[i]), int(cols[i])), (name, nx, int(rows[i]), int(cols[i]))]
        out += [(name, kb, 1, 1), (name, kb, c.H - 2, c.W - 2)]
    out += [("front_x", 20, row, col) for row in (0, 15, 16) for col in (31, 32, 33, 34)]
    out += [("front_y", 20, row, col) for row in (14, 15, 16) for col in (0, 31, 32)]
    out += [("horizon", 3, 4, col) for col in (15, 16, 17, 20)]
    out += [("near_saturated", 0, 10, 10), ("near_saturated", 5, 0, 63), ("ncc_extremes", 0, 16, 32), ("few_views", 8, 0, 0), ("few_views", 7, 3, 0), ("few_views", 9, 0, 5)]
    return out


@pytest.mark.parametrize("r", [1, 2, 4])
def test_brute_cells_equal_the_array_path(oracle, r):
    for name, d, row, col in _named_cells():
        c = wc.CASES[name]
        what = "%s plane %d (%d, %d) r = %d" % (name, d, row, col, r)
        per_view = []
        for v in range(c.V):
            s = wc.samples(name)[v]
            N, counted, cost = zm.brute_cell(c.main, (s["dot"][d] + 127) // 255, s["valid"][d], r, row, col)
            assert N == zm.box(s["valid"][d].astype(np.int64), r)[row, col], what
            got = wc.view_costs(name, ZNCC, r)[v]
            assert (bool(got[0][d, row, col]), int(got[1][d, row, col])) == (counted, cost), what
            per_view.append(cost if counted else None)
        for cost in (ABSDIFF, ZNCC):
            for keep in (1, 2, KEEP_ALL):
                n, costs, cell = km.brute_cell(oracle, cost, c.main_cam, c.main, c.side_cams, c.sides, c.z()[d], r, keep, row, col)
                assert cell == int(wc.bestk_volume(name, cost, r, keep)[d, row, col]), what
                if cost == ZNCC:
                    assert costs == [x for x in per_view if x is not None], what


@pytest.mark.parametrize("cost,r", [(ABSDIFF, 0), (ABSDIFF, 2), (ZNCC, 1), (ZNCC, 4)])
@pytest.mark.parametrize("name", wc.BANDS)
def test_the_bands_brute_cells_equal_the_array_path(oracle, name, cost, r):
    """cells beside the dead pixels on the seams and on the frame's border lines: every window member at its own plane"""
    c = wc.CASES[name]
    offsets = c.z()
    cells = ((7, 31), (8, 31), (15, 32), (16, 30), (16, 33), (23, 33), (3, 32), (5, 31), (1, 1), (30, 62), (12, 17), (0, 1), (3, 0), (4, 63), (c.H - 1, 40))
    for d in (0, 8, 15):
        for row, col in cells:
            for keep in (2, KEEP_ALL):
                if row < c.H:
                    cell = bbm.brute_cell(oracle, cost, c.main_cam, c.main, c.side_cams, c.sides, c.prior, offsets[d], r, keep, row, col)[2]
                    assert cell == int(wc.bestk_volume(name, cost, r, keep, band=True)[d, row, col]), (d, row, col, keep)
