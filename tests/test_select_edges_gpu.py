"""The depth selection and the sub-plane refinement on crafted volumes at the edges of their kernels (csrc/select.hip: argmin_volume in its
four instantiations and its partial form, combine_best, refine_depth): the volumes of tests/select_volumes.py go in through
mvs_sweep_use_volume + mvs_sweep_set_planes, no sweep runs, and the maps and the 8-byte records are compared bit for bit with the numpy
mirror (tests/select_mirror.py).  tests/test_select_cpu.py shows without a GPU what every volume is for.  The contract tests at the end
cover what mvs_sweep_refine_depth, mvs_sweep_clean and the entries that take a caller's volume refuse; every refused call there would stay
inside its buffers if it ran."""
import numpy as np
import pytest
import torch

import mvs_amd
import select_mirror as mirror
import select_volumes as sv

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _upload(vol, offset_cells=0):
    """the volume in device memory, `offset_cells` cells into its tensor -> (tensor that owns the memory, view of the volume)"""
    flat = torch.from_numpy(np.ascontiguousarray(vol).view(np.int32).reshape(-1).copy())   # a copy: the crafted volumes are read-only
    owner = torch.zeros(flat.numel() + offset_cells, dtype=torch.int32, device="cuda")
    view = owner[offset_cells:]
    view.copy_(flat)
    torch.cuda.synchronize()
    return owner, view


def _inject(ctx, vol, z_range, offset_cells=0):
    """make `vol` the context's volume of vol.shape[0] planes; the caller keeps the returned tensors alive while the context uses them"""
    owner, view = _upload(vol, offset_cells)
    ctx.sweep_use_volume(view.data_ptr(), view.numel() * 4)
    ctx.sweep_set_planes(vol.shape[0], *z_range)
    return owner, view


def _untouched(view, vol):
    return torch.equal(view.cpu(), torch.from_numpy(np.ascontiguousarray(vol).view(np.int32).reshape(-1).copy()))


def _maps(ctx):
    """(index, cost, depth), the order of the mirror"""
    depth, cost, index, _ = ctx.sweep_fetch()
    return index.copy(), cost.copy(), depth.copy()


def _same(got, want, what):
    for g, w, name in zip(got, want, ("index", "cost", "depth")):
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, "%s: %s differs in %d pixels; first at (y, x) = %s: %r, mirror %r" % (what, name, len(wrong), wrong[0], g[tuple(wrong[0])], w[tuple(wrong[0])])


def _set_index(ctx, index):
    """overwrite the context's index map (the stream is idle: _maps has synchronised)"""
    H, W = index.shape
    dst = torch.as_tensor(mvs_amd._DeviceArray(ctx.sweep_result_pointers()[2], (H, W), "<i4"), device="cuda")
    dst.copy_(torch.from_numpy(index.copy()).cuda())
    torch.cuda.synchronize()


def _select_and_refine(ctx, case, oracle, offset_cells=0):
    """argmin, refine, refine again (and the same for a foreign index) against the mirror -> tensors to keep alive"""
    vol, foreign = sv.volume(case)
    cs, z = sv.CS[case.sampler], oracle.plane_table(case.D, *case.z_range)
    keep = _inject(ctx, vol, case.z_range, offset_cells)
    ctx.sweep_argmin()
    want = mirror.select(vol, cs, z)
    _same(_maps(ctx), want, case.name + " argmin")
    for index in (want[0],) if foreign is None else (want[0], foreign):
        if index is foreign:
            _set_index(ctx, foreign)       # the selection exists: the argmin above made it over these planes
        refined = (index, want[1], mirror.refine(vol, cs, z, index))
        ctx.sweep_refine_depth()
        once = _maps(ctx)
        _same(once, refined, case.name + " refine")
        ctx.sweep_refine_depth()           # the kernel reads the index, not the depth
        _same(_maps(ctx), once, case.name + " refine twice")
        if case.D < 3:
            assert (_bits(once[2]) == _bits(mirror.plain_depth(z, index))).all(), case.name + ": a depth moved with D < 3"
    assert _untouched(keep[1], vol), case.name + ": the volume was written"
    return keep


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("gen", list(sv.GENERATORS))
def test_crafted_volumes(oracle, gen, sampler):
    """every case of a generator; one context per image size, so the plane count shrinks and grows between the cases too"""
    contexts, keep = {}, []
    try:
        for case in sv.cases_of(gen):
            if case.sampler != sampler:
                continue
            if (case.W, case.H) not in contexts:
                contexts[(case.W, case.H)] = mvs_amd.Context(case.W, case.H, 0, sampler=sampler)
            keep.append(_select_and_refine(contexts[(case.W, case.H)], case, oracle))
    finally:
        for ctx in contexts.values():
            ctx.close()


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_misaligned_pointer(oracle, sampler):
    """P % 4 == 0 but the volume starts 4 bytes past a 16-byte boundary: single-cell loads, the same maps"""
    for gen in ("mixed_counts", "ties", "extremes", "parabolas"):
        for case in sv.cases_of(gen):
            if case.sampler == sampler and case.W * case.H % 4 == 0 and case.D in (9, 17):
                with mvs_amd.Context(case.W, case.H, 0, sampler=sampler) as ctx:
                    owner, view = _select_and_refine(ctx, case, oracle, offset_cells=1)
                    assert owner.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4


def _records(ctx, view, case, split):
    """mvs_sweep_argmin_partial over every part of `split` -> (device tensor [parts, H, W, 2], the same as uint32 on the host)"""
    P = case.W * case.H
    recs = torch.full((len(split), case.H, case.W, 2), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    first = 0
    for k, count in enumerate(split):
        ctx.sweep_argmin_partial(view.data_ptr() + first * P * 4, first, count, recs[k].data_ptr())
        first += count
    ctx.synchronize()
    return recs, recs.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in sv.PARTIAL_CASES])
def test_partial_selection_and_merge(oracle, case):
    vol, _ = sv.volume(case)
    cs, z = sv.CS[case.sampler], oracle.plane_table(case.D, *case.z_range)
    want = mirror.select(vol, cs, z)
    with mvs_amd.Context(case.W, case.H, 0, sampler=case.sampler) as ctx:
        owner, view = _inject(ctx, vol, case.z_range)
        ctx.sweep_argmin()
        _same(_maps(ctx), want, case.name + " argmin")
        nobody = torch.zeros((1, case.H, case.W, 2), dtype=torch.int32, device="cuda")
        nobody[..., 1] = -1                # (0, 0xffffffff)
        for split in sv.SPLITS:
            what = "%s split %s" % (case.name, list(split) if len(split) < 10 else "%d x 1" % len(split))
            recs, host = _records(ctx, view, case, split)
            bounds = np.concatenate(([0], np.cumsum(split)))
            for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
                np.testing.assert_array_equal(host[k], mirror.select_partial(vol[a:b], cs, int(a)), err_msg="%s, records of part %d" % (what, k))
            if case.gen == "extremes" and len(split) > 1:
                assert (host[..., 1] == mirror.NONE_RECORD[1]).any(), "a part in which a pixel sees nothing"
            assert (_bits(mirror.combine(host, cs, z)[0]) == _bits(want[0])).all()
            ctx.sweep_combine_partials(recs.data_ptr(), len(split))
            _same(_maps(ctx), want, what + " merged")
            # a part in which nobody sees anything, in the middle and in front
            for parts in (torch.cat((recs[:1], nobody, recs[1:])), torch.cat((nobody, recs))):
                parts = parts.contiguous()
                torch.cuda.synchronize()
                ctx.sweep_combine_partials(parts.data_ptr(), parts.shape[0])
                _same(_maps(ctx), want, what + " merged with an empty part")
        # the merge is a depth selection over the current planes: the refinement follows it
        ctx.sweep_refine_depth()
        _same(_maps(ctx), (want[0], want[1], mirror.refine(vol, cs, z, want[0])), case.name + " refine after the merge")
        assert _untouched(view, vol)


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_a_cell_of_count_zero_is_unseen_whatever_its_sum_bits(oracle, sampler):
    """no sweep writes a count of 0 over a non-zero sum, a caller's volume may: nobody sees the cell, as a candidate and as a neighbour"""
    for gen in ("parabolas", "foreign_index", "extremes"):
        case = next(c for c in sv.cases_of(gen) if c.sampler == sampler and (c.W, c.D) == (132, 17))
        vol, foreign = sv.volume(case)
        cs, z = sv.CS[sampler], oracle.plane_table(case.D, *case.z_range)
        dirty = sv.sum_bits_in_unseen_cells(vol, cs, 0xD1127)
        with mvs_amd.Context(case.W, case.H, 0, sampler=sampler) as ctx:
            owner, view = _inject(ctx, dirty, case.z_range)
            ctx.sweep_argmin()
            want = mirror.select(vol, cs, z)           # of the clean volume: the sum bits change nothing
            _same(_maps(ctx), want, case.name + " argmin")
            if foreign is not None:
                _set_index(ctx, foreign)
            index = want[0] if foreign is None else foreign
            ctx.sweep_refine_depth()
            _same(_maps(ctx), (index, want[1], mirror.refine(vol, cs, z, index)), case.name + " refine")
            recs, host = _records(ctx, view, case, (8, 9))
            np.testing.assert_array_equal(host[0], mirror.select_partial(vol[:8], cs, 0))
            np.testing.assert_array_equal(host[1], mirror.select_partial(vol[8:], cs, 8))


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
def test_poisoned_allocations(oracle, monkeypatch, sampler):
    """fresh maps full of 0xFF bytes: every pixel of depth, cost and index is written by the selection, every depth by the refinement"""
    monkeypatch.setenv("MVS_POISON_ALLOC", "1")
    for gen in ("parabolas", "extremes"):
        case = next(c for c in sv.cases_of(gen) if c.sampler == sampler and (c.W, c.D) == (131, 17))
        with mvs_amd.Context(case.W, case.H, 0, sampler=sampler) as ctx:
            _select_and_refine(ctx, case, oracle)


def test_shrinking_and_growing_on_one_context(oracle):
    """D = 17, then 7, then 17 with other volumes on one context: nothing of the earlier call shows"""
    by_d = {D: [c for g in ("extremes", "parabolas", "ties") for c in sv.cases_of(g) if c.sampler == "fixed" and (c.W, c.D) == (132, D)] for D in (17, 7)}
    with mvs_amd.Context(132, 9, 0, sampler="fixed") as ctx:
        keep = [_select_and_refine(ctx, case, oracle) for case in (by_d[17][0], by_d[7][0], by_d[17][1], by_d[7][1], by_d[17][2])]
        assert len(keep) == 5


# ---- what the refinement and the cleaning refuse --------------------------------------------------------------------------------
def _refused(ctx, call, code, *words):
    """`call` returns `code`, the error names `words`, and the three maps are what they were"""
    before = _maps(ctx)
    assert call() == code, ctx.lib.mvs_last_error(ctx.h)
    err = ctx.lib.mvs_last_error(ctx.h)
    assert all(w in err for w in words), err
    _same(_maps(ctx), before, "maps after a refused call")


def test_refine_refuses_a_short_volume(oracle):
    """... and so do the entries that make the caller's volume the one of the current planes: mvs_sweep_argmin, mvs_sweep_volume_device and
    mvs_sweep_run with MVS_SWEEP_VOLUME"""
    from mvs_amd import synth
    case = next(c for c in sv.cases_of("parabolas") if c.sampler == "fixed" and (c.W, c.D) == (132, 17))
    vol, _ = sv.volume(case)
    cs, z = 24, oracle.plane_table(case.D, *case.z_range)
    N = vol.size
    with mvs_amd.Context(case.W, case.H, 0, sampler="fixed") as ctx:
        lib = ctx.lib
        owner, view = _inject(ctx, vol, case.z_range)
        ctx.sweep_argmin()
        want = mirror.select(vol, cs, z)
        # one cell short, inside the full-size tensor
        ctx.sweep_use_volume(view.data_ptr(), (N - 1) * 4)
        _refused(ctx, lambda: lib.mvs_sweep_refine_depth(ctx.h), EINVAL, b"mvs_sweep_refine_depth", b"%d bytes" % ((N - 1) * 4), b"need %d" % (N * 4))
        ctx.sweep_use_volume(view.data_ptr(), N * 4)       # exactly enough
        ctx.sweep_refine_depth()
        _same(_maps(ctx), (want[0], want[1], mirror.refine(vol, cs, z, want[0])), "refine on a volume of exactly D H W cells")
        short = (b"caller volume", b"%d bytes" % ((N - 1) * 4), b"need %d" % (N * 4))
        ctx.sweep_use_volume(view.data_ptr(), (N - 1) * 4)
        _refused(ctx, lambda: lib.mvs_sweep_argmin(ctx.h), EINVAL, *short)
        _refused(ctx, lambda: lib.mvs_sweep_volume_device(ctx.h, None), None, *short)      # a null pointer
        ctx.sweep_use_volume(view.data_ptr(), N * 4)
        assert ctx.sweep_volume_device() == (view.data_ptr(), N * 4)
        ctx.sweep_argmin()
        _same(_maps(ctx), want, "argmin on a volume of exactly D H W cells")
        assert _untouched(view, vol)
        # a sweep of two views into the caller's volume
        main_cam, main_img, side_cams, sides = synth.make_views(case.W, case.H, 2, radius=0.3)[:4]
        ctx.sweep_set(main_cam, main_img, side_cams, sides, case.D)
        ctx.sweep_use_volume(view.data_ptr(), (N - 1) * 4)
        _refused(ctx, lambda: lib.mvs_sweep_run(ctx.h, 0, 2, mvs_amd.MVS_SWEEP_VOLUME), EINVAL, *short)
        assert _untouched(view, vol)
        ctx.sweep_use_volume(view.data_ptr(), N * 4)
        ctx.sweep_run(0, 2, mvs_amd.MVS_SWEEP_VOLUME)
        swept = ctx.sweep_fetch(want_volume=True)[3]
        assert not _untouched(view, vol) and _untouched(view, swept), "the sweep wrote the caller's volume of exactly D H W cells"


def test_a_selection_over_other_planes_is_refused(oracle):
    """argmin over 17 planes, then 5 planes: the index map still holds planes up to 16.  (Every address an unchecked kernel would touch
    lies inside the buffers of the 17 planes.)"""
    case = next(c for c in sv.cases_of("parabolas") if c.sampler == "fixed" and (c.W, c.D) == (131, 17))
    vol, _ = sv.volume(case)
    cs, z17, z5 = 24, oracle.plane_table(17, *case.z_range), oracle.plane_table(5, *case.z_range)
    with mvs_amd.Context(case.W, case.H, 0, sampler="fixed") as ctx:
        lib = ctx.lib
        # before any selection
        owner, view = _inject(ctx, vol, case.z_range)
        assert lib.mvs_sweep_refine_depth(ctx.h) == ESTATE and b"depth selection" in lib.mvs_last_error(ctx.h)
        assert lib.mvs_sweep_clean(ctx.h, 2, 10, 4, 1, 0) == ESTATE and b"no depth selection" in lib.mvs_last_error(ctx.h)
        ctx.sweep_argmin()
        want17 = mirror.select(vol, cs, z17)
        assert want17[0].max() > 4
        _same(_maps(ctx), want17, "argmin over 17 planes")
        ctx.sweep_set_planes(5, *case.z_range)
        _refused(ctx, lambda: lib.mvs_sweep_refine_depth(ctx.h), ESTATE, b"mvs_sweep_refine_depth", b"17 planes", b"has 5")
        _refused(ctx, lambda: lib.mvs_sweep_clean(ctx.h, 2, 10, 0, 1, 0), ESTATE, b"mvs_sweep_clean", b"17 planes", b"has 5")
        _refused(ctx, lambda: lib.mvs_sweep_clean(ctx.h, 0, 0, 4, 1, 0), ESTATE, b"mvs_sweep_clean", b"17 planes", b"has 5")
        # the same plane count again changes nothing: the selection over 17 planes is good for 17 planes
        ctx.sweep_set_planes(17, *case.z_range)
        ctx.sweep_set_planes(17, *case.z_range)
        ctx.sweep_refine_depth()
        _same(_maps(ctx), (want17[0], want17[1], mirror.refine(vol, cs, z17, want17[0])), "refine after set_planes with the same count")
        ctx.sweep_clean(min_views=2)
        # and a selection over the 5 planes is good for 5
        ctx.sweep_set_planes(5, *case.z_range)
        ctx.sweep_argmin()
        want5 = mirror.select(vol[:5], cs, z5)
        ctx.sweep_refine_depth()
        _same(_maps(ctx), (want5[0], want5[1], mirror.refine(vol[:5], cs, z5, want5[0])), "argmin and refine over 5 planes")
        ctx.sweep_clean(speckle_min_size=2)
        assert _untouched(view, vol)


def test_refine_refuses_the_contexts_own_short_volume(oracle):
    """the context's own volume allocated for 5 planes, a selection over 17 whose planes are all below 4: the refusal is about the
    volume's size.  (An unchecked kernel would read planes 0..4 only.)"""
    case = next(c for c in sv.cases_of("parabolas") if c.sampler == "fixed" and (c.W, c.D) == (132, 7))
    vol = sv.volume(case)[0][:5]
    W, H, cs = case.W, case.H, 24
    z5 = oracle.plane_table(5, -1.0, 1.0)
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        lib = ctx.lib
        ctx.sweep_set_planes(5)
        ptr, nbytes = ctx.sweep_volume_device()        # allocates the context's own volume; nothing is swept
        assert nbytes == 5 * H * W * 4
        own = torch.as_tensor(mvs_amd._DeviceArray(ptr, (5, H, W), "<i4"), device="cuda")
        own.copy_(torch.from_numpy(vol.view(np.int32).copy()).cuda())
        recs = torch.from_numpy(mirror.select_partial(vol[:4], cs, 0).view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        ctx.sweep_set_planes(17)
        ctx.sweep_combine_partials(recs.data_ptr(), 1)  # a selection over the 17 planes; the volume is not grown
        assert _maps(ctx)[0].max() <= 3
        _refused(ctx, lambda: lib.mvs_sweep_refine_depth(ctx.h), ESTATE, b"mvs_sweep_refine_depth", b"context's volume", b"%d bytes" % nbytes,
                 b"need %d" % (17 * H * W * 4))
        ctx.sweep_set_planes(5)
        _refused(ctx, lambda: lib.mvs_sweep_refine_depth(ctx.h), ESTATE, b"17 planes", b"has 5")
        ctx.sweep_argmin()
        want = mirror.select(vol, cs, z5)
        ctx.sweep_refine_depth()
        _same(_maps(ctx), (want[0], want[1], mirror.refine(vol, cs, z5, want[0])), "argmin and refine on the context's own 5 planes")


def test_row_bands_over_new_planes_select_once_they_cover_every_row(oracle):
    """a fused run over one band after the plane count went from 17 to 5 leaves the other rows with planes up to 16: no selection until
    the bands, each touching what the earlier ones covered, reach every row.  (All that an unchecked kernel would read lies inside the
    buffers of the 17 planes.)"""
    from mvs_amd import synth
    W, H = 132, 20
    both = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
    main_cam, main_img, side_cams, sides = synth.make_views(W, H, 2, radius=0.3)[:4]
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        lib = ctx.lib
        assert ctx.row_granularity() == 8
        ctx.sweep_set(main_cam, main_img, side_cams, sides, 17)
        ctx.sweep_run(0, 2, both)
        ctx.sweep_refine_depth()
        ctx.sweep_set_planes(5)
        for row_first, row_count in ((0, 8), (16, 4), (8, 8)):      # [0, 8); [16, 20) starts over; [8, 20)
            ctx.sweep_run_rows(row_first, row_count, flags=both)
            _refused(ctx, lambda: lib.mvs_sweep_refine_depth(ctx.h), ESTATE, b"mvs_sweep_refine_depth", b"depth selection")
            _refused(ctx, lambda: lib.mvs_sweep_clean(ctx.h, 2, 10, 0, 1, 0), ESTATE, b"mvs_sweep_clean", b"depth selection")
        ctx.sweep_run_rows(0, 8, flags=both)                           # [0, 20)
        depth, cost, index, vol = [a.copy() for a in ctx.sweep_fetch(want_volume=True)]
        assert index.max() <= 4
        ctx.sweep_refine_depth()
        want = oracle.refine_depth(vol, oracle.plane_table(5, -1.0, 1.0), index, sampler="fixed")
        _same(_maps(ctx), (index, cost, want), "refine after bands that cover every row")
        ctx.sweep_clean(min_views=2, uniqueness=10)
