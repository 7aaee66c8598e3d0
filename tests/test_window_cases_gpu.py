"""The windowed sweeps, the band sweeps and the propagation on the crafted cases of tests/window_cameras.py: every kernel that carries a copy
of the fixed sampler -- zncc.hip, bestk.hip (the table and band sweeps), bestk_gated.hip and propagate.hip through zncc_sample /
absdiff_sample, band.hip through absdiff_sample -- equals the mirrors built on tests/sweep_mirror.py's samples on volume, depth, cost and index (the band
sweeps also on the resolved map and the report, the propagation on z, gx, gy, cells, cost map and report), by exact equality: no cell
budget.  Between two runs a run over zero views empties volume and maps, so no run can pass on what its predecessor left.  One context
per frame size serves every case of that size."""
import numpy as np
import pytest

import band_mirror as bm
import mvs_amd
import propagate_cases as pc
import propagate_mirror as pm
import window_cameras as wc
from test_band_gpu import _device, _same_cells, _same_floats, _same_maps
from test_propagate_gpu import _same_state

pytestmark = pytest.mark.gpu

VOL, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOL | FUSED
ABSDIFF, ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL
COST_RADII = [(cost, r) for cost in (ABSDIFF, ZNCC) for r in wc.RADII[cost]]
F = np.float32
# the cases held against gated_mirror (the identity at tau = 255 runs on every case): a ladder of each kind and axis, s.w == 0, both fronts
GATED = ["ladder_int_left", "ladder_int_bottom", "ladder_tie_right", "ladder_tie_top", "horizon", "front_x", "front_y", "few_views", "shear_tie"]


def test_the_bindings_constants_are_the_mirrors():
    assert (ABSDIFF, ZNCC, KEEP_ALL) == (wc.ABSDIFF, wc.ZNCC, wc.KEEP_ALL)


@pytest.fixture(scope="module")
def contexts():
    have = {}

    def staged(c):
        if (c.W, c.H) not in have:
            have[c.W, c.H] = mvs_amd.Context(c.W, c.H, 0, sampler="fixed")
        ctx = have[c.W, c.H]
        ctx.sweep_set(*c.views(), c.D)
        np.testing.assert_array_equal(ctx.sweep_view_matrices(), c.q())
        return ctx

    yield staged
    for ctx in have.values():
        ctx.close()


def _empty(ctx):
    ctx.sweep_run(0, 0, BOTH)


def _volume_and_maps(ctx, run, vol, z, what):
    _empty(ctx)
    run(BOTH)
    got = ctx.sweep_fetch(want_volume=True)
    _same_cells(got[3], vol, what + ", volume + fused")
    _same_maps(got[:3], wc.maps(vol, z), what + ", volume + fused")


def _three_ways(ctx, run, vol, z, what):
    _volume_and_maps(ctx, run, vol, z, what)
    want = wc.maps(vol, z)
    _empty(ctx)
    run(FUSED)
    _same_maps(ctx.sweep_fetch()[:3], want, what + ", fused alone")
    _empty(ctx)
    run(VOL)
    ctx.sweep_argmin()
    got = ctx.sweep_fetch(want_volume=True)
    _same_cells(got[3], vol, what + ", volume + mvs_sweep_argmin")
    _same_maps(got[:3], want, what + ", volume + mvs_sweep_argmin")


# ---- zncc.hip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.PLAIN + ["max_views_zncc"])
def test_zncc_equals_the_mirror(contexts, name):
    c = wc.CASES[name]
    ctx = contexts(c)
    for r in wc.RADII[ZNCC]:
        _three_ways(ctx, lambda flags: ctx.sweep_run_zncc(r, 0, c.V, flags), wc.zncc_volume(name, r), c.z(), "%s, zncc r = %d" % (name, r))


# ---- bestk.hip -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.PLAIN)
def test_bestk_equals_the_mirror(contexts, name):
    c = wc.CASES[name]
    ctx = contexts(c)
    keeps = wc.FEW_KEEPS if name == "few_views" else (2, KEEP_ALL)
    for cost, r in COST_RADII:
        for keep in keeps:
            check = _three_ways if keep == 2 else _volume_and_maps
            check(ctx, lambda flags: ctx.sweep_run_bestk(cost, r, keep, 0, c.V, flags), wc.bestk_volume(name, cost, r, keep), c.z(),
                  "%s, %s r = %d keep = %d" % (name, wc.COST_NAMES[cost], r, keep))
    if name == "few_views":      # without the repeated view: the count takes 0 .. 3
        for cost, r in ((ABSDIFF, 0), (ZNCC, 2)):
            for keep in wc.FEW_KEEPS:
                _volume_and_maps(ctx, lambda flags: ctx.sweep_run_bestk(cost, r, keep, 0, 3, flags), wc.bestk_volume(name, cost, r, keep, nviews=3), c.z(),
                                 "%s, views [0, 3), %s r = %d keep = %d" % (name, wc.COST_NAMES[cost], r, keep))


@pytest.mark.parametrize("name,cost", [("max_views_zncc", ZNCC), ("max_views_absdiff", ABSDIFF)])
def test_bestk_on_255_views(contexts, name, cost):
    c = wc.CASES[name]
    ctx = contexts(c)
    for r in wc.RADII[cost]:
        for keep in (8, KEEP_ALL):
            vol = wc.bestk_volume(name, cost, r, keep)
            assert (vol == ((0xFFFD0200 if cost == ZNCC else 0xFFFD02FF) if keep == KEEP_ALL else (8 << 24) | 8 * (65024 if cost == ZNCC else 65025))).all()
            _three_ways(ctx, lambda flags: ctx.sweep_run_bestk(cost, r, keep, 0, c.V, flags), vol, c.z(), "%s, r = %d keep = %d" % (name, r, keep))


# ---- bestk_gated.hip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.PLAIN + ["max_views_zncc", "max_views_absdiff"])
def test_gated_at_tau_255_is_the_ungated_kernel(contexts, name):
    c = wc.CASES[name]
    ctx = contexts(c)
    guide = _device(c.guide())
    for cost in {"max_views_zncc": (ZNCC,), "max_views_absdiff": (ABSDIFF,)}.get(name, (ABSDIFF, ZNCC)):
        for r in (1, 2, 3, 4):
            for keep in ((8, KEEP_ALL) if c.V == 255 else (2, KEEP_ALL)):
                what = "%s, %s r = %d keep = %d, tau = 255" % (name, wc.COST_NAMES[cost], r, keep)
                _empty(ctx)
                ctx.sweep_run_bestk(cost, r, keep, 0, c.V, BOTH)
                ref = ctx.sweep_fetch(want_volume=True)
                _same_cells(ref[3], wc.bestk_volume(name, cost, r, keep), what + ": the ungated kernel")
                _empty(ctx)
                ctx.sweep_run_bestk_gated(cost, r, keep, 255, guide.data_ptr(), 0, c.V, BOTH)
                got = ctx.sweep_fetch(want_volume=True)
                _same_cells(got[3], ref[3], what)
                _same_maps(got[:3], ref[:3], what)


@pytest.mark.parametrize("tau", [0, 30])
@pytest.mark.parametrize("name", GATED)
def test_gated_equals_the_mirror(contexts, name, tau):
    c = wc.CASES[name]
    ctx = contexts(c)
    guide = _device(c.guide())
    for cost, r, keep in ((ABSDIFF, 1, 2), (ABSDIFF, 3, KEEP_ALL), (ZNCC, 2, KEEP_ALL), (ZNCC, 4, 2)):
        vol = wc.gated_volume(name, cost, r, keep, tau)
        assert (vol != wc.bestk_volume(name, cost, r, keep)).any(), "the gate changes cells"
        _three_ways(ctx, lambda flags: ctx.sweep_run_bestk_gated(cost, r, keep, tau, guide.data_ptr(), 0, c.V, flags), vol, c.z(),
                    "%s, %s r = %d keep = %d, tau = %d" % (name, wc.COST_NAMES[cost], r, keep, tau))


# ---- band.hip, the band entry of bestk.hip -------------------------------------------------------------------------------------------
def _band_maps(ctx, c, vol, what):
    """the maps hold offsets; then the resolved map and the report"""
    want = wc.maps(vol, c.z())
    _same_maps(ctx.sweep_fetch()[:3], want, what)
    _same_floats(ctx.sweep_band_resolve(), bm.resolve(c.prior, want[0], want[2]), what + ", resolved")
    assert ctx.sweep_band_report() == bm.report(c.prior, want[0], want[2], c.D), what


def _band_three_ways(ctx, c, run, vol, what):
    _empty(ctx)
    run(BOTH)
    _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, what + ", volume + fused")
    _band_maps(ctx, c, vol, what + ", volume + fused")
    _empty(ctx)
    run(FUSED)
    _band_maps(ctx, c, vol, what + ", fused alone")
    _empty(ctx)
    run(VOL)
    ctx.sweep_argmin()
    _same_cells(ctx.sweep_fetch(want_volume=True)[3], vol, what + ", volume + mvs_sweep_argmin")
    _band_maps(ctx, c, vol, what + ", volume + mvs_sweep_argmin")


@pytest.mark.parametrize("name", wc.BANDS)
def test_band_equals_the_mirror_and_the_gather(contexts, name):
    c = wc.CASES[name]
    ctx = contexts(c)
    prior = _device(c.prior)
    vol = wc.band_volume(name)
    _band_three_ways(ctx, c, lambda flags: ctx.sweep_run_band(prior.data_ptr(), 0, c.V, flags), vol, name)
    # prior + offset_d is plane d + s of the table: the band's cells are the plain sweep's, gathered -- on the device too
    _empty(ctx)
    ctx.sweep_run(0, c.V, VOL)
    plain = ctx.sweep_fetch(want_volume=True)[3]
    _same_cells(plain, wc.sweep_volume(name), "the plain sweep")
    idx = np.arange(c.D)[:, None, None] + c.smap[None]
    rows, cols = np.indices((c.H, c.W))
    have = bm.inside(c.prior)[None] & (idx >= 0) & (idx < c.D)
    _same_cells(np.where(have, plain[np.clip(idx, 0, c.D - 1), rows[None], cols[None]], 0).astype(np.uint32), vol, "the gather identity")
    for first in range(c.V):          # a view at a time (band_shift: front_x's, horizon's and shear_tie's camera)
        ctx.sweep_run_band(prior.data_ptr(), first, 1, VOL)
        s = wc.samples(name, band=True)[first]
        one = np.where(s["valid"], (1 << 24) + np.abs(s["dot"] - 255 * c.main.astype(np.int64)[None]), 0).astype(np.uint32)
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], one, "%s, view %d" % (name, first))


@pytest.mark.parametrize("cost,r", [(ABSDIFF, 0), (ABSDIFF, 1), (ABSDIFF, 4), (ZNCC, 1), (ZNCC, 2), (ZNCC, 4)])
@pytest.mark.parametrize("name", wc.BANDS)
def test_band_bestk_equals_the_mirror(contexts, name, cost, r):
    c = wc.CASES[name]
    ctx = contexts(c)
    prior = _device(c.prior)
    for keep in (2, KEEP_ALL):
        vol = wc.bestk_volume(name, cost, r, keep, band=True)
        _band_three_ways(ctx, c, lambda flags: ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, keep, 0, c.V, flags), vol,
                         "%s, %s r = %d keep = %d" % (name, wc.COST_NAMES[cost], r, keep))
    if (cost, r) == (ABSDIFF, 0):
        _same_cells(wc.bestk_volume(name, cost, r, KEEP_ALL, band=True), wc.band_volume(name), "radius 0, every view: the band sweep")
    for first in range(c.V):
        ctx.sweep_run_band_bestk(prior.data_ptr(), cost, r, KEEP_ALL, first, 1, VOL)
        counted, cc = wc.view_costs(name, cost, r, band=True)[first]
        _same_cells(ctx.sweep_fetch(want_volume=True)[3], np.where(counted, np.uint32(1 << 24) + cc, 0).astype(np.uint32), "%s, view %d" % (name, first))


# ---- propagate.hip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost,r,keep", [(ABSDIFF, 1, 2), (ZNCC, 2, KEEP_ALL), (ZNCC, 4, 1), (ABSDIFF, 0, KEEP_ALL)])
@pytest.mark.parametrize("name", wc.PROPAGATED)
def test_init_on_a_plane_is_that_plane_of_the_bestk_volume(contexts, name, cost, r, keep):
    """no mirror needed: a hypothesis (z_d, 0, 0) at every pixel samples every window member at z_d"""
    c = wc.CASES[name]
    ctx = contexts(c)
    ctx.sweep_run_bestk(cost, r, keep, 0, c.V, VOL)
    vol = ctx.sweep_fetch(want_volume=True)[3]
    _same_cells(vol, wc.bestk_volume(name, cost, r, keep), name)
    for d, zd in enumerate(c.z()):
        start = _device(np.full((c.H, c.W), zd, F))
        ctx.propagate_init(start.data_ptr(), cost, r, keep)
        z, gx, gy, cells = ctx.propagate_fetch()
        _same_cells(cells, vol[d], "%s, %s r = %d keep = %d, plane %d" % (name, wc.COST_NAMES[cost], r, keep, d))
        assert (z == zd).all() and not gx.any() and not gy.any()


@pytest.mark.parametrize("cost,r,keep", [(ABSDIFF, 1, 2), (ZNCC, 2, KEEP_ALL), (ZNCC, 4, KEEP_ALL)])
@pytest.mark.parametrize("name", wc.PROPAGATED)
def test_propagation_equals_the_mirror(oracle, contexts, name, cost, r, keep):
    c = wc.CASES[name]
    ctx = contexts(c)
    start = c.start_map()
    dz, dg, seed, max_step = 1.0 / 16, 1.0 / 64, 0x5EED, 0.25
    state = pm.State(pm.Scene(oracle, *c.views()), start, cost, r, keep, slopes=True, max_step=max_step)
    what = "%s, %s r = %d" % (name, wc.COST_NAMES[cost], r)
    assert (~pm.inside(state.z)).sum() >= 6 and state.gx.any() and state.gy.any() and (state.cells != 0).any(), what
    for g in (state.gx, state.gy):
        assert (g * 16 == np.round(g * 16)).all(), "the seeded slopes are multiples of 1/16: exact"
    ctx.propagate_init(_device(start).data_ptr(), cost, r, keep, slopes=True, max_step=max_step)
    _same_state(ctx, pc.snapshot(state), what + ", init")
    for nrandom in (0, 2):
        state.run(1, dz, dg, nrandom, seed)
        ctx.propagate_run(1, dz, dg, nrandom, seed)
        _same_state(ctx, pc.snapshot(state), what + ", then an iteration with nrandom = %d" % nrandom)
    assert sum(state.report()[1:4]) > 0, what + ": some candidate won"
