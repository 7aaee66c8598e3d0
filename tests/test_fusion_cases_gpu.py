"""mvs_fuse_depth, mvs_tsdf_integrate, mvs_tsdf_integrate_frames, mvs_tsdf_shade and mvs_tsdf_surface on the crafted cases of
tests/fusion_cases.py: general (rotated, rolled, shifted, mirrored) cameras, values ON every decision of the contracts, a depth step, holes on
the tile seams.  Every comparison is bit for bit against the mirrors, with the matrices of mvs_depth_slot_matrices; every case's premise is
asserted here again, with those matrices (tests/test_fusion_cases_cpu.py shows it with the host's, and that a subtly wrong kernel would
change the bytes compared here)."""
import functools

import numpy as np
import pytest

import appearance_mirror as am
import fusion_cases as fc
import mvs_amd
import tsdf_mirror as tm

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32


@functools.lru_cache(maxsize=None)
def _context(W, H):
    """the stores of fusion_cases.store(W, H) on the device -> (context, the kernels' matrices per depth slot)"""
    st = fc.store(W, H)
    ctx = mvs_amd.Context(W, H)
    ctx.depth_store(fc.DEPTH_CAP)
    ctx.frame_store(fc.FRAME_CAP)
    for s in range(fc.DEPTH_CAP):
        ctx.depth_upload(s, st["cams"][s], st["depths"][s], st["costs"][s])
    for fs, img in st["frames"].items():
        ctx.frame_upload(fs, img)
    return ctx, {s: ctx.depth_slot_matrices(s) for s in range(fc.DEPTH_CAP)}


@functools.lru_cache(maxsize=None)
def _snapshots(W, H, G):
    return fc.tsdf_snapshots(fc.store(W, H), _context(W, H)[1], G)


def _same_rows(got, exp, what):
    assert got.shape == exp.shape, "%s: %d rows, mirror %d" % (what, len(got), len(exp))
    bad = np.nonzero((got.view(u32) != exp.view(u32)).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d rows differ; first %d: %s vs %s" % (what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]])


def _same_fields(got, exp_sum, exp_count, what):
    s, c = got
    assert np.array_equal(c, exp_count), "%s: %d counts differ" % (what, int((c != exp_count).sum()))
    bad = s.view(u32) != exp_sum.view(u32)
    assert not bad.any(), "%s: %d sums differ; first %s: %r vs %r" % (what, int(bad.sum()), np.argwhere(bad)[0], s[bad][0], exp_sum[bad][0])


def _same_cells(got, exp, what):
    bad = got != exp
    assert not bad.any(), "%s: %d cells differ; first %s: %#x vs %#x" % (what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], exp[bad][0])


def _integrate_frames(ctx, pairs, **kw):
    ctx.tsdf_integrate_frames([d for d, _ in pairs], [f for _, f in pairs], **kw)


# ---- mvs_fuse_depth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.FUSE_CASES, ids=[c[0] for c in fc.FUSE_CASES])
def test_fusion_case(case):
    """the rows equal the mirror's, the case's premise holds with the kernels' matrices, and a second run gives the same rows"""
    name, size, ref, nbrs, _, _ = case
    ctx, mats = _context(*size)
    kw = fc.fuse_parameters(case, mats)
    exp = fc.fuse_expected(case, mats)
    fc.check_fuse_premise(case, exp, mats)
    got = ctx.fuse_depth(ref, nbrs, **kw)
    _same_rows(got, exp["rows"], name)
    again = ctx.fuse_depth(ref, nbrs, **kw)
    assert again.tobytes() == got.tobytes()


# ---- mvs_tsdf_integrate, mvs_tsdf_integrate_frames: the rotated set --------------------------------------------------------------------------
@pytest.mark.parametrize("size", fc.TSDF_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("G", fc.GRIDS)
def test_rotated_set_lists(G, size):
    """every prefix length of the slot list from a cleared volume, through both entry points; then the lists under max_cost = 0.5 and
    max_cost = 0 on top; the whole sequence one slot per call"""
    ctx, mats = _context(*size)
    snaps, final = _snapshots(size[0], size[1], G)
    origin, h = fc.cube(G)
    for n in fc.LENGTHS:
        es, ec, ecells = snaps[n]
        ctx.tsdf_volume(G, origin, h, 4 * h)
        ctx.tsdf_integrate(fc.TSDF_LIST[:n])
        _same_fields(ctx.tsdf_fetch(), es, ec, "%d slots" % n)
        ctx.tsdf_volume(G, origin, h, 4 * h)
        _integrate_frames(ctx, fc.pairs(fc.TSDF_LIST[:n]))
        _same_fields(ctx.tsdf_fetch(), es, ec, "%d pairs" % n)
        _same_cells(ctx.tsdf_appearance_fetch(), ecells, "%d pairs" % n)
    votes, _ = am.split(ecells)
    assert (ec > 0).mean() > 0.2 and (votes > 0).mean() > 0.05 and (ec > votes).any()
    for key, slots, mc in (("cost", fc.TSDF_LIST_COST, fc.MAX_COST), ("zero", fc.TSDF_LIST_ZERO, 0.0)):
        _integrate_frames(ctx, fc.pairs(slots), max_cost=float(mc))
        assert (snaps[key][1] != ec).any()
        es, ec, ecells = snaps[key]
        _same_fields(ctx.tsdf_fetch(), es, ec, key)
        _same_cells(ctx.tsdf_appearance_fetch(), ecells, key)
    # one slot per call: the plain path, then the frames path
    calls = [([s], {}) for s in fc.TSDF_LIST] + [([s], {"max_cost": float(fc.MAX_COST)}) for s in fc.TSDF_LIST_COST] + [([s], {"max_cost": 0.0}) for s in fc.TSDF_LIST_ZERO]
    ctx.tsdf_volume(G, origin, h, 4 * h)
    for slots, kw in calls:
        ctx.tsdf_integrate(slots, **kw)
    _same_fields(ctx.tsdf_fetch(), final.sum, final.count, "one slot per call")
    ctx.tsdf_volume(G, origin, h, 4 * h)
    for slots, kw in calls:
        _integrate_frames(ctx, fc.pairs(slots), **kw)
    _same_fields(ctx.tsdf_fetch(), final.sum, final.count, "one pair per call")
    _same_cells(ctx.tsdf_appearance_fetch(), final.cells, "one pair per call")


# ---- the tie volumes ------------------------------------------------------------------------------------------------------------------------
def _crafted(ctx, vol, cams, depths, frames, slots, make_volume):
    """both entry points on crafted maps (frame slot = depth slot) against the mirror: every prefix length of the list from a cleared volume,
    then the whole list one slot per call -> the mirror's volume after the whole list"""
    for s, d in enumerate(depths):
        ctx.depth_upload(s, cams[s], d)
        ctx.frame_upload(s, frames[s])
    mats = {s: ctx.depth_slot_matrices(s) for s in range(len(cams))}
    snaps = fc.crafted_snapshots(vol, depths, mats, frames, slots)
    for n in fc.LENGTHS:
        es, ec, ecells = snaps[n]
        make_volume()
        ctx.tsdf_integrate(slots[:n])
        _same_fields(ctx.tsdf_fetch(), es, ec, "%d slots" % n)
        make_volume()
        ctx.tsdf_integrate_frames(slots[:n], slots[:n])
        _same_fields(ctx.tsdf_fetch(), es, ec, "%d pairs" % n)
        _same_cells(ctx.tsdf_appearance_fetch(), ecells, "%d pairs" % n)
    make_volume()
    for s in slots:
        ctx.tsdf_integrate([s])
    _same_fields(ctx.tsdf_fetch(), es, ec, "one slot per call")
    make_volume()
    for s in slots:
        ctx.tsdf_integrate_frames([s], [s])
    _same_fields(ctx.tsdf_fetch(), es, ec, "one pair per call")
    _same_cells(ctx.tsdf_appearance_fetch(), ecells, "one pair per call")
    return vol


def test_band_ties():
    """nodes whose t is exactly -1, the float below it, exactly 1 and the float below it (built with the kernels' matrices): updated with -1, not
    updated, counted without a vote, counted with one"""
    W, H, G = fc.BAND_W, fc.BAND_H, fc.BAND_G
    cams = fc.band_cameras()
    frames = fc.crafted_frames(2, W, H, 0xBA9D)
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(2)
        ctx.frame_store(2)
        for s, cam in enumerate(cams):
            ctx.depth_upload(s, cam, np.ones((H, W), f32))
        mats = {s: ctx.depth_slot_matrices(s) for s in range(2)}
        depths, placed, nodes = fc.band_ties(mats)
        assert all(n >= 8 for cam in placed for n in cam), placed
        make = lambda: ctx.tsdf_volume(G, fc.BAND_ORIGIN, fc.BAND_H_NODE, fc.BAND_TAU)   # noqa: E731
        exp = _crafted(ctx, fc.band_volume(), cams, depths, frames, fc.BAND_LIST, make)
        assert 0.05 < (exp.count > 0).mean() < 0.5
        for s in (0, 1):     # one slot alone: the tie nodes read as rule 4 and rule B say
            make()
            ctx.tsdf_integrate_frames([s], [s])
            total, count = ctx.tsdf_fetch()
            votes, _ = am.split(ctx.tsdf_appearance_fetch())
            for node, k in nodes[s]:
                expect = [(f32(-1.0), 1, 1), (f32(0.0), 0, 0), (f32(1.0), 1, 0), (fc.T_TIES[3], 1, 1)][k]
                assert (total[node], count[node], votes[node]) == expect, (s, node, k)


def test_pixel_rounding():
    """nodes ON the optical axis, ON pixel seams, ON fc = W and fr = H, outside every border, behind two of the cameras and ON one's centre"""
    W, H, G = fc.ROUND_W, fc.ROUND_H, fc.ROUND_G
    frames = fc.crafted_frames(3, W, H, 0x90D)
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(3)
        ctx.frame_store(3)
        make = lambda: ctx.tsdf_volume(G, fc.ROUND_ORIGIN, fc.ROUND_H_NODE, fc.ROUND_TAU)   # noqa: E731
        exp = _crafted(ctx, fc.round_volume(), fc.round_cameras(), fc.round_depths(), frames, fc.ROUND_LIST, make)
    votes, _ = am.split(exp.cells)
    assert (exp.count > 0).sum() >= 3000 and (votes > 0).sum() >= 1000 and exp.count.max() >= 4


# ---- mvs_tsdf_shade, mvs_tsdf_surface over the rotated set's volume ---------------------------------------------------------------------------
def _mirror_volume(G, fields):
    origin, h = fc.cube(G)
    vol = am.Volume(G, origin, h, 4 * h)
    vol.sum, vol.count, vol.cells = fields
    return vol


# depth slot -> least pixels without a grey level (holes, tie blocks on the near and far planes, surface outside every other frustum)
SHADED = {fc.ROLLED: 4, fc.SHIFTED: 10, fc.DEEP: 150, fc.HOLEY_ROLLED: 500, fc.TIES: 60}


@pytest.mark.parametrize("slot", sorted(SHADED))
def test_shading_a_general_camera(slot):
    """the stored map of a rotated camera (rolled; shifted; its own near / far; rolled with holes; with depth-rule ties), shaded from the
    volume the whole list made"""
    W, H = fc.SIZES[0]
    G = 50
    ctx, mats = _context(W, H)
    st = fc.store(W, H)
    origin, h = fc.cube(G)
    ctx.tsdf_volume(G, origin, h, 4 * h)
    _integrate_frames(ctx, fc.pairs(fc.TSDF_LIST))
    got = ctx.tsdf_shade(st["cams"][slot], ctx.depth_slot_pointer(slot))
    exp = am.shade(_mirror_volume(G, _snapshots(W, H, G)[0][19]), mats[slot], st["depths"][slot])
    have = exp[..., 1] == 255
    assert have.mean() > 0.5 and (~have).sum() >= SHADED[slot] and len(np.unique(exp[..., 0][have])) > 50
    bad = (got != exp).any(-1)
    assert not bad.any(), "%d pixels differ; first %s: %r vs %r" % (int(bad.sum()), np.argwhere(bad)[0], got[bad][0], exp[bad][0])


@pytest.mark.parametrize("min_obs", [1, 3])
def test_surface_of_the_rotated_volume(min_obs):
    """the field and mask kernel on the ragged support real rotated frusta leave: faces equal the surface-nets oracle's on the fetched fields,
    vertices within tests/test_tsdf_gpu.py's bound"""
    W, H = fc.SIZES[0]
    G = 65
    ctx, _ = _context(W, H)
    origin, h = fc.cube(G)
    ctx.tsdf_volume(G, origin, h, 4 * h)
    ctx.tsdf_integrate(fc.TSDF_LIST)
    total, count = ctx.tsdf_fetch()
    es, ec, _ = _snapshots(W, H, G)[0][19]
    _same_fields((total, count), es, ec, "the whole list")
    v, f = ctx.tsdf_surface(min_obs)
    vol = tm.Volume(G, origin, h, 4 * h)
    vol.sum, vol.count = total, count
    rv, rf = vol.surface(min_obs)
    seen = count >= min_obs
    assert 0.1 < seen.mean() < 0.6 and len(f) > 1000
    assert np.array_equal(f, rf) and len(v) == len(rv)
    assert np.abs(v - rv).max() <= 2e-6 * float(np.abs(origin).max() + G * h)
