"""mvs_sweep_clean on the GPU (csrc/clean.hip) against the numpy mirror of DESIGN.md section 16 (tests/clean_mirror.py): the depth / cost /
index maps, the report and the size map, bit for bit.  Crafted index maps (tests/clean_maps.py; tests/test_clean_cpu.py shows what each
holds) reach the context through a volume whose winner-take-all selection they are -- inject() + sweep_argmin, no sweep runs -- and
the cells rules 1-2 read come from a second injected volume; the real path runs behind a sweep on the synthetic scene."""
import numpy as np
import pytest
import torch

import clean_maps
import clean_mirror
import mvs_amd
import sgm_mirror
from mvs_amd import synth
from test_aggregate_edges_gpu import inject

pytestmark = pytest.mark.gpu

CS = {"fixed": 24, "exact": 16}
EINVAL, ESTATE = -1, -3
D8 = clean_maps.D_MAPS


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _maps(ctx):
    return tuple(a.copy() for a in ctx.sweep_fetch()[:3])


def _same_maps(got, want, what=""):
    for g, w, name in zip(got, want, ("depth", "cost", "index")):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s %s" % (name, what))


def _select(ctx, index, cs):
    """make `index` the context's selection: the volume of clean_maps.volume_for, winner-take-all -> (volume tensor, volume, maps)"""
    vol = clean_maps.volume_for(index, D8, cs)
    t = inject(ctx, vol, D8)
    ctx.sweep_argmin()
    maps = _maps(ctx)
    np.testing.assert_array_equal(maps[2], index)
    return t, vol, maps


def _clean_and_compare(ctx, before, vol, cs, S=None, min_views=0, uniqueness=0, speckle_min_size=0, speckle_max_diff=1, what=""):
    """one mvs_sweep_clean on the context's maps (= `before`) against the mirror -> (maps after, report, sizes)"""
    ctx.sweep_clean(min_views, uniqueness, speckle_min_size, speckle_max_diff, aggregated=S is not None)
    got = _maps(ctx)
    report = ctx.sweep_clean_report()
    d, c, i, report_ref, sizes_ref = clean_mirror.clean(*before, vol, cs, S, min_views, uniqueness, speckle_min_size, speckle_max_diff)
    if speckle_min_size:
        sizes = ctx.sweep_clean_sizes()
        assert sizes.dtype == np.int32 and ctx.lib.mvs_sweep_clean_sizes_device(ctx.h)
        wrong = np.argwhere(sizes != sizes_ref)
        assert len(wrong) == 0, "%s: %d sizes differ; first at (y, x) = %s: %d, mirror %d" % (what, len(wrong), wrong[0], sizes[tuple(wrong[0])], sizes_ref[tuple(wrong[0])])
    else:
        sizes = None
        assert ctx.lib.mvs_sweep_clean_sizes_device(ctx.h) is None
        assert ctx.lib.mvs_sweep_clean_sizes_fetch(ctx.h, np.empty(before[2].shape, np.int32).ctypes.data_as(mvs_amd._i32p)) == ESTATE
    assert report == report_ref, what
    _same_maps(got, (d, c, i), what)
    untouched = i >= 0
    for g, b in zip(got, before):
        assert _bits(g)[untouched].tobytes() == _bits(b)[untouched].tobytes()
    return got, report, sizes


# ---- rule 3 on crafted index maps ---------------------------------------------------------------------------------------------------
def _speckle_runs(ctx, index, cs, runs):
    """every (min_size, max_diff, kept pixels expected or None) of `runs` on the map, the selection restored in between"""
    t, vol, before = _select(ctx, index, cs)
    out = []
    for k, (min_size, max_diff, kept) in enumerate(runs):
        if k:
            ctx.sweep_argmin()
        got, report, sizes = _clean_and_compare(ctx, before, None, cs, None, 0, 0, min_size, max_diff, what="min_size %d, max_diff %d" % (min_size, max_diff))
        if kept is not None:
            assert int((got[2] >= 0).sum()) == kept and report == [int((index >= 0).sum()), 0, 0, int((index >= 0).sum()) - kept]
        out.append(sizes)
    del t
    return out


@pytest.mark.parametrize("W,H", [(203, 77), (21, 5)])
def test_constant_map(W, H):
    with mvs_amd.Context(W, H, 0) as ctx:
        sizes = _speckle_runs(ctx, clean_maps.constant(W, H), 24, ((W * H, 1, W * H), (W * H + 1, 1, 0), (1, 0, W * H)))
        assert all((s == W * H).all() for s in sizes)


def test_checkerboard():
    W, H = 203, 77
    with mvs_amd.Context(W, H, 0) as ctx:
        sizes = _speckle_runs(ctx, clean_maps.checkerboard(W, H, 1), 24, ((2, 1, 0), (1, 1, W * H), (W * H, 2, W * H), (W * H + 1, 2, 0)))
        assert (sizes[0] == 1).all() and (sizes[2] == W * H).all()


@pytest.mark.parametrize("gen", ["serpentine", "spiral"])
@pytest.mark.parametrize("W,H", [(203, 77), (640, 480)])
def test_one_pixel_wide_paths(gen, W, H):
    index, length = getattr(clean_maps, gen)(W, H)
    with mvs_amd.Context(W, H, 0, sampler="exact" if gen == "spiral" else "fixed") as ctx:
        sizes = _speckle_runs(ctx, index, 16 if gen == "spiral" else 24, ((length, 1, length), (length + 1, 1, 0), (4, 0, 0)))
        assert (sizes[0][index >= 0] == length).all() and sizes[2].max() == 3


def test_ramp():
    W, H = 203, 77
    with mvs_amd.Context(W, H, 0) as ctx:
        sizes = _speckle_runs(ctx, clean_maps.ramp(W, H), 24, ((W * H, 1, W * H), (26 * H, 0, 182 * H), (26 * H + 1, 0, 0)))
        assert (sizes[0] == W * H).all() and (sizes[1][:, :182] == 26 * H).all() and (sizes[1][:, 182:] == 21 * H).all()


def test_threshold_squares():
    W, H = 203, 77
    index, want = clean_maps.threshold_squares(W, H)
    with mvs_amd.Context(W, H, 0) as ctx:
        t, vol, before = _select(ctx, index, 24)
        got, report, sizes = _clean_and_compare(ctx, before, None, 24, speckle_min_size=16, speckle_max_diff=1)
        for (cx, cy), size in want.items():
            assert sizes[cy, cx] == size and (got[2][cy, cx] >= 0) == (size >= 16), (cx, cy, size)
        assert report == [16 * 12, 0, 0, 15 * 4]


@pytest.mark.parametrize("name,seed,planes,weights", clean_maps.PERCOLATION)
def test_percolation_noise(name, seed, planes, weights):
    W, H = clean_maps.PERCOLATION_SHAPE
    index = clean_maps.percolation(W, H, seed, planes, weights)
    with mvs_amd.Context(W, H, 0) as ctx:
        sizes = _speckle_runs(ctx, index, 24, ((50, 1, None), (2, 1, None), (100000, 1, 0)))
        assert len(np.unique(sizes[0])) >= 20


# ---- rules 1 and 2 on crafted cells -------------------------------------------------------------------------------------------------
def _overwrite_sums(ctx, S):
    """put `S` where the last mvs_sweep_aggregate left its sums (the device buffer the library hands out)"""
    ptr, nbytes = ctx.sweep_aggregated_device()
    assert nbytes == S.size * 2
    ctx.synchronize()
    alias = torch.as_tensor(mvs_amd._DeviceArray(ptr, S.shape, "<i2"), device="cuda")
    alias.copy_(torch.from_numpy(S.view(np.int16).copy()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("W,H,D", [(70, 5, 11), (129, 6, 65)])
def test_rules_1_and_2_on_crafted_cells(W, H, D, sampler):
    cs = CS[sampler]
    index, cells, S, kind = clean_maps.rules_case(W, H, D, cs, 0x12 + D)
    selecting = clean_maps.volume_for(index, D, cs)
    with mvs_amd.Context(W, H, 0, sampler=sampler) as ctx:
        t_cells = inject(ctx, cells, D)
        ctx.sweep_aggregate(4, 0, 0, 1)          # any sums of D planes: the crafted ones replace them
        _overwrite_sums(ctx, S)
        t_sel = inject(ctx, selecting, D)
        ctx.sweep_argmin()
        before = _maps(ctx)
        np.testing.assert_array_equal(before[2], index)
        fired = np.zeros(3, int)
        for min_views in (0, 1, 2, 3):
            for u in (0, clean_maps.UNIQUENESS, 35, 99):
                for flag in (False, True):
                    ctx.sweep_use_volume(t_sel.data_ptr(), t_sel.numel() * 4)
                    ctx.sweep_argmin()
                    ctx.sweep_use_volume(t_cells.data_ptr(), t_cells.numel() * 4)
                    _, report, _ = _clean_and_compare(ctx, before, cells, cs, S if flag else None, min_views, u, what="min_views %d, u %d, flag %s" % (min_views, u, flag))
                    fired += np.array(report[1:]) > 0
        assert fired[0] and fired[1] and not fired[2]
        assert torch.equal(t_cells.cpu(), torch.from_numpy(cells.view(np.int32).copy())), "the cleaning wrote into the volume"
        np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)


# ---- the real path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_behind_a_sweep(oracle, sampler):
    """sweep -> aggregate(refine) -> clean with nothing that synchronises in between, then the same on refined winner-take-all maps"""
    W, H, D, V = 160, 120, 32, 4
    cs = CS[sampler]
    main_cam, main_img, side_cams, sides, gt = synth.make_views(W, H, V, radius=0.3)
    z_lo, z_hi = float(gt.min()) - 0.002, float(gt.max()) + 0.002
    params = dict(min_views=2, uniqueness=10, speckle_min_size=100, speckle_max_diff=1)
    with mvs_amd.Context(W, H, 0, sampler=sampler) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D, z_lo, z_hi)
        ctx.sweep_run(0, V, mvs_amd.MVS_SWEEP_VOLUME)
        ctx.sweep_aggregate(8, 16, 128, 4080, refine=True)
        ctx.sweep_clean(aggregated=True, **params)
        cleaned, report, sizes = _maps(ctx), ctx.sweep_clean_report(), ctx.sweep_clean_sizes()
        vol, S = ctx.sweep_fetch(want_volume=True)[3], ctx.sweep_aggregate_fetch()
        ctx.sweep_aggregate(8, 16, 128, 4080, refine=True)      # the uncleaned maps again
        before = _maps(ctx)
        assert (before[0] != oracle.plane_table(D, z_lo, z_hi)[np.clip(before[2], 0, None)])[before[2] >= 0].mean() > 0.1, "premise: refined depths"
        d, c, i, report_ref, sizes_ref = clean_mirror.clean(*before, vol, cs, S, 2, 10, 100, 1)
        print("%s, aggregated: report %s" % (sampler, report))
        assert report == report_ref and sum(report[1:]) > 0
        np.testing.assert_array_equal(sizes, sizes_ref)
        _same_maps(cleaned, (d, c, i))
        kept = cleaned[2] >= 0
        assert _bits(cleaned[0])[kept].tobytes() == _bits(before[0])[kept].tobytes()
        # winner-take-all, refined
        ctx.sweep_argmin()
        wta = _maps(ctx)
        ctx.sweep_refine_depth()
        before = _maps(ctx)
        assert (before[0] != wta[0]).mean() > 0.1
        cleaned, report, _ = _clean_and_compare(ctx, before, vol, cs, None, **params)
        print("%s, winner-take-all: report %s" % (sampler, report))
        assert report[2] > 0 and report[3] > 0
        kept = cleaned[2] >= 0
        assert _bits(cleaned[0])[kept].tobytes() == _bits(before[0])[kept].tobytes()
        # nothing but the maps changed
        ctx.sweep_argmin()
        _same_maps(_maps(ctx), wta)
        np.testing.assert_array_equal(ctx.sweep_fetch(want_volume=True)[3], vol)
        np.testing.assert_array_equal(ctx.sweep_aggregate_fetch(), S)


# ---- state ----------------------------------------------------------------------------------------------------------------------
def _all_rules(ctx, W, H, D, cs, seed):
    """the cells and the selection of a rules_case, all three rules at once -> (tensors to keep alive, cells, maps after)"""
    index, cells, S, _ = clean_maps.rules_case(W, H, D, cs, seed)
    t_sel = inject(ctx, clean_maps.volume_for(index, D, cs), D)
    ctx.sweep_argmin()
    before = _maps(ctx)
    t_cells = inject(ctx, cells, D)
    got, report, _ = _clean_and_compare(ctx, before, cells, cs, None, 2, 10, 3, 2)
    assert all(report)
    return (t_sel, t_cells), cells, got


def test_poisoned_allocations(monkeypatch):
    """labels, roots, sizes and counters come from fresh allocations filled with 0xFF bytes: every word read must have been written by the call"""
    monkeypatch.setenv("MVS_POISON_ALLOC", "1")
    with mvs_amd.Context(129, 6, 0) as ctx:
        _all_rules(ctx, 129, 6, 65, 24, 0x12 + 65)
    W, H = clean_maps.PERCOLATION_SHAPE
    with mvs_amd.Context(W, H, 0) as ctx:
        _speckle_runs(ctx, clean_maps.percolation(W, H, 7, (4,)), 24, ((50, 1, None),))


def test_a_second_clean_rejects_nothing():
    with mvs_amd.Context(129, 6, 0) as ctx:
        keep, cells, once = _all_rules(ctx, 129, 6, 65, 24, 0x12 + 65)
        twice, report, _ = _clean_and_compare(ctx, once, cells, 24, None, 2, 10, 3, 2)
        assert report == [int((once[2] >= 0).sum()), 0, 0, 0]
        _same_maps(twice, once)
        # and with every rule off the call only counts
        again, report, _ = _clean_and_compare(ctx, once, cells, 24)
        assert report == [int((once[2] >= 0).sum()), 0, 0, 0]
        _same_maps(again, once)
    W, H = clean_maps.PERCOLATION_SHAPE
    with mvs_amd.Context(W, H, 0) as ctx:
        t, vol, before = _select(ctx, clean_maps.percolation(W, H, 11, (0, 2, 3)), 24)
        once, report, _ = _clean_and_compare(ctx, before, None, 24, speckle_min_size=30)
        assert report[3] > 0
        _, report, _ = _clean_and_compare(ctx, once, None, 24, speckle_min_size=30)
        assert report == [int((once[2] >= 0).sum()), 0, 0, 0]


def test_large_and_small_contexts_take_turns():
    big, small = clean_maps.percolation(203, 77, 21, (4,)), clean_maps.percolation(21, 5, 22, (4,))
    with mvs_amd.Context(203, 77, 0) as a, mvs_amd.Context(21, 5, 0) as b:
        for ctx, index in ((a, big), (b, small), (a, big), (b, small)):
            _speckle_runs(ctx, index, 24, ((6, 1, None),))


def test_speckle_only_after_a_fused_sweep_without_a_volume():
    W, H, D, V = 150, 70, 24, 2
    main_cam, main_img, side_cams, sides = synth.make_views(W, H, V, radius=0.8)[:4]
    with mvs_amd.Context(W, H, 0) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        ctx.sweep_run(0, V, mvs_amd.MVS_SWEEP_FUSED_ARGMIN)
        before = _maps(ctx)
        assert ctx.lib.mvs_sweep_clean(ctx.h, 2, 0, 0, 1, 0) == ESTATE and ctx.lib.mvs_sweep_clean(ctx.h, 0, 10, 0, 1, 0) == ESTATE
        _same_maps(_maps(ctx), before)
        _, report, sizes = _clean_and_compare(ctx, before, None, 24, min_views=1, speckle_min_size=40, speckle_max_diff=1)
        print("fused sweep, speckle only: report %s, %d components" % (report, len(np.unique(sizes))))
        assert report[3] > 0 and report[3] < report[0]


def test_errors_leave_the_maps_and_the_context_usable():
    W, H, D = 70, 5, 11
    index, cells, S, _ = clean_maps.rules_case(W, H, D, 24, 0x12 + D)
    with mvs_amd.Context(W, H, 0) as ctx:
        lib = ctx.lib
        out = (mvs_amd.C.c_int * 4)()
        sizes = np.empty((H, W), np.int32)

        def code(*args):
            return lib.mvs_sweep_clean(ctx.h, *args)

        # nothing selected yet, nothing cleaned yet
        assert code(0, 0, 4, 1, 0) == ESTATE and b"no depth selection" in lib.mvs_last_error(ctx.h)
        assert lib.mvs_sweep_clean_report(ctx.h, out) == ESTATE
        assert lib.mvs_sweep_clean_sizes_fetch(ctx.h, sizes.ctypes.data_as(mvs_amd._i32p)) == ESTATE and lib.mvs_sweep_clean_sizes_device(ctx.h) is None
        t = inject(ctx, cells, D)
        ctx.sweep_argmin()
        before = _maps(ctx)
        for args in ((-1, 0, 0, 1, 0), (256, 0, 0, 1, 0), (0, -1, 0, 1, 0), (0, 100, 0, 1, 0), (0, 0, -1, 1, 0), (0, 0, 4, -1, 0), (0, 0, 4, 256, 0),
                     (2, 10, 4, 1, 2), (2, 10, 4, 1, 0x80000001)):
            assert code(*args) == EINVAL, args
        assert b"flag" in lib.mvs_last_error(ctx.h)
        assert lib.mvs_sweep_clean(None, 2, 10, 4, 1, 0) == EINVAL and lib.mvs_sweep_clean_report(ctx.h, None) == EINVAL
        assert lib.mvs_sweep_clean_sizes_fetch(ctx.h, None) == EINVAL
        # the flag without sums, and with sums of another plane count
        assert code(0, 10, 0, 1, 1) == ESTATE and b"MVS_CLEAN_SCORES_AGGREGATED" in lib.mvs_last_error(ctx.h)
        ctx.sweep_aggregate(4, 16, 128, 4080)
        ctx.sweep_set_planes(D - 2)
        ctx.sweep_argmin()
        small = _maps(ctx)
        assert code(0, 10, 0, 1, 1) == ESTATE
        _same_maps(_maps(ctx), small)
        ctx.sweep_set_planes(D)
        ctx.sweep_argmin()
        # a volume one cell short of D * H * W
        short = t.reshape(-1)[:D * H * W - 1]
        ctx.sweep_use_volume(short.data_ptr(), short.numel() * 4)
        assert code(2, 0, 0, 1, 0) == ESTATE and code(0, 10, 0, 1, 0) == ESTATE and b"packed volume" in lib.mvs_last_error(ctx.h)
        assert lib.mvs_sweep_clean_report(ctx.h, out) == ESTATE, "no clean has run yet"
        ctx.sweep_use_volume(t.data_ptr(), t.numel() * 4)
        _same_maps(_maps(ctx), before)
        # still usable, and the report and the sizes follow the last clean
        _clean_and_compare(ctx, before, cells, 24, None, 2, 10, 3, 2)
        assert lib.mvs_sweep_clean_report(ctx.h, out) == 0 and lib.mvs_sweep_clean_sizes_fetch(ctx.h, sizes.ctypes.data_as(mvs_amd._i32p)) == 0
        assert code(0, 100, 0, 1, 0) == EINVAL
        assert lib.mvs_sweep_clean_report(ctx.h, out) == 0, "an error leaves the last report readable"
        ctx.sweep_argmin()
        _clean_and_compare(ctx, before, cells, 24, None, 2, 0, 0, 1)     # rule 3 off: no sizes (checked inside)
