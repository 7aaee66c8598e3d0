"""The sweep kernels on the crafted cameras of tests/sweep_cameras.py: every kernel path of both samplers equals tests/sweep_mirror.py -- the
contract of DESIGN.md section 2 restated without the oracle -- on volume, depth, cost and index, by exact equality: no cell budget.

Paths of the fixed sampler: the default (sweep_fx_rect where the plan takes it), MVS_SWEEP_NO_RECT (sweep_fx_tiled), the same in a context
created under MVS_NO_SEP=1, without the plane-independent-w path, without the region look-ahead, with linear tile order, and
MVS_SWEEP_FORCE_GENERIC (the un-tiled kernel).  Of the exact sampler: the default (sweep_exact_rect where it plans), MVS_SWEEP_NO_RECT
(sweep_tiled), its 4 x 16 shape, without paired reads, and the un-tiled kernel.  Each path runs as volume + fused selection, fused selection
alone and volume + mvs_sweep_argmin; between two runs a run over zero views empties volume and maps, so no run can pass on what its
predecessor left.  Cases with 33 planes also run with 1, 2 and 3 workgroups per tile.  The contexts of the path tests are created under
MVS_PLAN_DUMP and are reused across the cases of a size: the planner's descriptors show that a case took the modes it is there for."""
import numpy as np
import pytest

import mvs_amd
import sweep_cameras as sc

pytestmark = pytest.mark.gpu

VOL, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
NO_RECT, UNTILED = mvs_amd.MVS_SWEEP_NO_RECT, mvs_amd.MVS_SWEEP_FORCE_GENERIC

# name -> (flags, context created under MVS_NO_SEP=1)
PATHS = {
    "fixed": {"default": (0, False), "no_rect": (NO_RECT, False), "no_rect_no_sep": (NO_RECT, True), "no_const_w": (NO_RECT | (4 << 8), False),
              "no_lookahead": (NO_RECT | (8 << 8), False), "linear_tiles": (NO_RECT | (2 << 8), False), "untiled": (UNTILED, False)},
    "exact": {"default": (0, False), "no_rect": (NO_RECT, False), "4x16": (8 << 8, False), "no_paired_reads": (16 << 8, False), "untiled": (UNTILED, False)},
}
NAMES = sorted(sc.CASES)


class Contexts:
    """one context per (size, sampler, hooks), created on first use under the hooks' environment and closed with the module"""

    def __init__(self, tmp):
        self.tmp, self.have = tmp, {}

    def get(self, W, H, sampler, no_sep=False, dump=True):
        key = (W, H, sampler, no_sep, dump)
        if key not in self.have:
            path = self.tmp / ("plan_%d_%d_%s_%d.bin" % (W, H, sampler, no_sep))
            with pytest.MonkeyPatch.context() as mp:
                if dump:
                    mp.setenv("MVS_PLAN_DUMP", str(path))
                if no_sep:
                    mp.setenv("MVS_NO_SEP", "1")
                self.have[key] = (mvs_amd.Context(W, H, sampler=sampler), path)
        return self.have[key]

    def close(self):
        for ctx, _ in self.have.values():
            ctx.close()


@pytest.fixture(scope="module")
def contexts(tmp_path_factory):
    c = Contexts(tmp_path_factory.mktemp("sweep_cases"))
    yield c
    c.close()


def _equal(got, m, what, volume=True):
    for a, key in zip(got, ("depth", "cost", "index", "volume")):
        if key == "volume" and not volume:
            continue
        bad = np.argwhere(a != m[key])
        assert len(bad) == 0, "%s, %s: %d of %d differ, the first at %s: device %r, mirror %r" % (
            what, key, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], m[key][tuple(bad[0])])


def _empty(ctx):
    ctx.sweep_run(0, 0, VOL | FUSED)


def _three_ways(ctx, V, flags, m, what):
    _empty(ctx)
    ctx.sweep_run(0, V, VOL | FUSED | flags)
    _equal(ctx.sweep_fetch(want_volume=True), m, what + ", volume + fused")
    _empty(ctx)
    ctx.sweep_run(0, V, FUSED | flags)
    _equal(ctx.sweep_fetch(want_volume=False), m, what + ", fused alone", volume=False)
    _empty(ctx)
    ctx.sweep_run(0, V, VOL | flags)
    ctx.sweep_argmin()
    _equal(ctx.sweep_fetch(want_volume=True), m, what + ", volume + mvs_sweep_argmin")


def _rectified(c):
    """True: pure shifts within the rectified kernels' boxes; False: a view they cannot take (shear, or w not constant); None: boxes decide"""
    if any(not (q[0, 1] == 0 and q[1, 0] == 0 and q[2, 0] == 0 and q[2, 1] == 0 and q[2, 2] == 0 and q[2, 3] > 0) for q in c.q()):
        return False
    return True if c.rect else None


def _set(ctx, c):
    main, sides = c.frames()
    ctx.sweep_set(c.main_cam, main, c.side_cams, sides, c.D)
    np.testing.assert_array_equal(ctx.sweep_view_matrices(), c.q())


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("name", NAMES)
def test_every_path_equals_the_mirror(contexts, name, sampler):
    c = sc.CASES[name]
    m = sc.mirror_of(name, sampler)
    rect = _rectified(c)
    for path, (flags, no_sep) in PATHS[sampler].items():
        ctx, dump = contexts.get(c.W, c.H, sampler, no_sep)
        if dump.exists():
            dump.unlink()
        _set(ctx, c)
        _three_ways(ctx, c.V, flags, m, "%s, %s, %s" % (name, sampler, path))
        shape = ctx.plan_shape()
        if path == "default" and rect is not None:
            want = ((4,) if rect else (3,)) if sampler == "fixed" else ((5,) if rect else (1, 2))
            assert shape in want, "%s, %s: plan shape %d, expected %s" % (name, sampler, shape, want)
        if path == "4x16":
            assert shape == 2
        if path == "no_rect":
            premise = c.plan_premise if sampler == "fixed" else c.exact_plan_premise
            assert shape in ((3, 4) if sampler == "fixed" else (1, 2))
            plan = sc.read_plan(dump)
            assert plan.shape[3] == c.V and plan.shape[1] == (c.W + 63) // 64
            if premise:
                premise(c, plan)


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("name", sc.D33)
def test_forced_plane_splits(contexts, name, sampler, nsplit):
    """33 planes: 3 chunks of 16 (2 of 32 in the exact sampler's 2 x 32 shape) over 1, 2 and 3 workgroups per tile, the tail chunk on clamped z"""
    c = sc.CASES[name]
    m = sc.mirror_of(name, sampler)
    ctx, dump = contexts.get(c.W, c.H, sampler)
    _set(ctx, c)
    for path in ("default", "no_rect") + (("no_lookahead",) if sampler == "fixed" else ("4x16",)):
        _three_ways(ctx, c.V, PATHS[sampler][path][0] | (nsplit << 16), m, "%s, %s, %s, %d workgroups per tile" % (name, sampler, path, nsplit))
    if sampler == "fixed" and c.plan_premise:
        c.plan_premise(c, sc.read_plan(dump))


@pytest.mark.parametrize("sampler", ["fixed", "exact"])
@pytest.mark.parametrize("size", sorted({(c.W, c.H) for c in sc.CASES.values()}), ids=lambda s: "%dx%d" % s)
def test_two_orders_on_one_context(size, sampler):
    """the cases of a size on ONE context with the plan cache at work (no MVS_PLAN_DUMP), forwards and backwards: the same bytes, and the
    mirror's -- a plan or a quad image that outlives its case shows here"""
    names = [n for n in NAMES if (sc.CASES[n].W, sc.CASES[n].H) == size and sc.CASES[n].V <= 8]
    with mvs_amd.Context(size[0], size[1], sampler=sampler) as ctx:
        seen = {}
        for name in names + names[::-1]:
            c = sc.CASES[name]
            _set(ctx, c)
            for flags in (0, NO_RECT):
                ctx.sweep_run(0, c.V, VOL | FUSED | flags)
                got = ctx.sweep_fetch(want_volume=True)
                _equal(got, sc.mirror_of(name, sampler), "%s, %s, flags %d" % (name, sampler, flags))
                key = (name, flags)
                if key in seen:
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, seen[key]))
                seen[key] = got
