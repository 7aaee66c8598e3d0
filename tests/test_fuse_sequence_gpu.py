"""Support planes, mvs_fuse_depth_masked, mvs_tsdf_integrate_masked and mvs_fuse_sequence on the GPU (csrc/fuse.hip, csrc/tsdf.hip,
csrc/fuse_sequence.hip) against tests/fuse_sequence_mirror.py, bit for bit, on the cases of
tests/fuse_sequence_cases.py (tests/test_fuse_sequence_cpu.py asserts their premises), with the matrices mvs_depth_slot_matrices returns.
The three identities hold on the device: a second store whose masked depths were overwritten with 1.0 gives the masked calls' bytes,
min_support = 0 gives today's calls' bytes, and nrefs = 1 gives the single call's rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import appearance_mirror as am
import fuse_mirror as fm
import fuse_sequence_cases as sc
import fuse_sequence_mirror as sm
import fusion_cases as fc
import mvs_amd

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
EINVAL, ESTATE = -1, -3
MS = sc.MIN_SUPPORT
INF = float("inf")
_i32p, _fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)


def _ip(a):
    return a.ctypes.data_as(_i32p)


@functools.lru_cache(maxsize=None)
def _context(W, H):
    """fusion_cases.store(W, H) on the device with the planes of fuse_sequence_cases -> (context, the kernels' matrices per depth slot)"""
    st = fc.store(W, H)
    ctx = mvs_amd.Context(W, H)
    ctx.depth_store(fc.DEPTH_CAP)
    ctx.frame_store(fc.FRAME_CAP)
    for s in range(fc.DEPTH_CAP):
        ctx.depth_upload(s, st["cams"][s], st["depths"][s], st["costs"][s])
        ctx.depth_support_upload(s, sc.planes(W, H)[s])
    for fs, img in st["frames"].items():
        ctx.frame_upload(fs, img)
    return ctx, {s: ctx.depth_slot_matrices(s) for s in range(fc.DEPTH_CAP)}


@functools.lru_cache(maxsize=None)
def _overwritten(W, H):
    """the same store with every depth whose support is below MIN_SUPPORT overwritten with 1.0, and no planes"""
    st = fc.store(W, H)
    ctx = mvs_amd.Context(W, H)
    ctx.depth_store(fc.DEPTH_CAP)
    ctx.frame_store(fc.FRAME_CAP)
    md = sm.masked(dict(enumerate(st["depths"])), sc.supports(W, H), MS)
    for s in range(fc.DEPTH_CAP):
        ctx.depth_upload(s, st["cams"][s], md[s], st["costs"][s])
    for fs, img in st["frames"].items():
        ctx.frame_upload(fs, img)
    return ctx


def _maps(size):
    st = fc.store(*size)
    return dict(enumerate(st["depths"])), dict(enumerate(st["costs"])), sc.supports(*size)


def _same_rows(got, exp, what):
    assert got.shape == exp.shape, "%s: %d rows, mirror %d" % (what, len(got), len(exp))
    bad = np.nonzero((got.view(u32) != exp.view(u32)).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d rows differ; first %d: %s vs %s" % (what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]])


def _fuse_masked_raw(ctx, ref, nbrs, min_support, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, max_cost=INF):
    """mvs_fuse_depth_masked itself (Context.fuse_depth issues mvs_fuse_depth for min_support = 0) -> (return code, rows)"""
    nb = np.ascontiguousarray(list(nbrs) or [0], np.int32)
    out = np.zeros((ctx.H * ctx.W, 7), f32)
    n = C.c_int(-5)
    rc = ctx.lib.mvs_fuse_depth_masked(ctx.h, int(ref), len(nbrs), _ip(nb), int(min_consistent), float(max_reproj_px), float(max_rel_depth), float(max_cost),
                                       int(min_support), out.ctypes.data_as(_fp), C.byref(n))
    return rc, out[:max(n.value, 0)]


def _sequence_raw(ctx, refs, nb, min_support=0, max_rows=0, out=None, counts=True, nrefs=None, nneighbours=None, min_consistent=2, max_reproj_px=1.0,
                  max_rel_depth=0.01, max_cost=INF, total=True, refs_null=False):
    """mvs_fuse_sequence itself -> (return code, total, per-reference counts)"""
    refs = np.ascontiguousarray(refs, np.int32)
    nb = np.ascontiguousarray(nb, np.int32)
    cnt = np.full(max(len(refs), 1), -7, np.int32)
    n = C.c_longlong(-5)
    rc = ctx.lib.mvs_fuse_sequence(ctx.h, len(refs) if nrefs is None else nrefs, None if refs_null else _ip(refs), nb.shape[1] if nneighbours is None else nneighbours,
                                   _ip(nb), int(min_consistent), float(max_reproj_px), float(max_rel_depth), float(max_cost), int(min_support), int(max_rows),
                                   out.ctypes.data_as(_fp) if out is not None else None, _ip(cnt) if counts else None, C.byref(n) if total else None)
    return rc, n.value, cnt


# ---- the planes ---------------------------------------------------------------------------------------------------------------------------
def test_plane_round_trips():
    W, H = 67, 45
    st = fc.store(W, H)
    planes = sc.planes(W, H)
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(3)
        lib, h = ctx.lib, ctx.h
        buf = np.zeros((H, W), np.uint8)
        p8 = buf.ctypes.data_as(C.POINTER(C.c_uint8))
        # refusals, each followed by a call that succeeds
        assert lib.mvs_depth_support_upload(h, 0, p8) == ESTATE and b"holds no depth map" in lib.mvs_last_error(h)
        ctx.depth_upload(0, st["cams"][0], st["depths"][0])
        assert lib.mvs_depth_support_upload(h, 3, p8) == EINVAL and lib.mvs_depth_support_upload(h, -1, p8) == EINVAL
        assert lib.mvs_depth_support_upload(h, 0, None) == EINVAL and lib.mvs_depth_support_upload_device(h, 0, None) == EINVAL
        assert lib.mvs_depth_support_fetch(h, 0, p8) == ESTATE and b"no support plane" in lib.mvs_last_error(h)
        assert lib.mvs_depth_support_fetch(h, 0, None) == EINVAL and lib.mvs_depth_support_fetch(h, 7, p8) == EINVAL
        assert lib.mvs_depth_support_drop(h, 3) == EINVAL
        ctx.depth_support_upload(0, planes[0])
        assert np.array_equal(ctx.depth_support_fetch(0), planes[0])
        # device upload into another slot; the first one's plane stays
        ctx.depth_upload(2, st["cams"][2], st["depths"][2], st["costs"][2])
        dev = torch.as_tensor(planes[5].copy(), device="cuda")
        ctx.depth_support_upload_device(2, dev.data_ptr())
        assert np.array_equal(ctx.depth_support_fetch(2), planes[5]) and np.array_equal(ctx.depth_support_fetch(0), planes[0])
        assert lib.mvs_depth_support_fetch(h, 1, p8) == ESTATE
        # an upload replaces, a drop forgets, the depth map stays
        ctx.depth_support_upload(2, planes[3])
        assert np.array_equal(ctx.depth_support_fetch(2), planes[3])
        ctx.depth_support_drop(2)
        assert lib.mvs_depth_support_fetch(h, 2, p8) == ESTATE
        assert len(ctx.fuse_depth(2, [0], min_consistent=1)) > 0
        with pytest.raises(mvs_amd.MvsError, match="no support plane"):
            ctx.fuse_depth(2, [0], min_consistent=1, min_support=1)
        # a depth upload into the slot drops its plane (host and device form)
        ctx.depth_upload(0, st["cams"][0], st["depths"][0])
        assert lib.mvs_depth_support_fetch(h, 0, p8) == ESTATE
        ctx.depth_support_upload(0, planes[0])
        ctx.depth_upload_device(0, st["cams"][2], ctx.depth_slot_pointer(2))
        assert lib.mvs_depth_support_fetch(h, 0, p8) == ESTATE
        # re-sizing empties the store, planes included
        ctx.depth_support_upload(0, planes[0])
        ctx.depth_store(2)
        assert lib.mvs_depth_support_fetch(h, 0, p8) == ESTATE and lib.mvs_depth_support_upload(h, 0, p8) == ESTATE
        ctx.depth_upload(1, st["cams"][1], st["depths"][1])
        ctx.depth_support_upload(1, planes[1])
        assert np.array_equal(ctx.depth_support_fetch(1), planes[1])


# ---- mvs_fuse_depth_masked ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.MASKED_CASES, ids=[c[0] for c in sc.MASKED_CASES])
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_fuse_depth_masked(size, case):
    name, ref, nbrs, kw = case
    ctx, mats = _context(*size)
    depths, costs, supports = _maps(size)
    exp = sm.fuse_masked(depths, costs, supports, mats, ref, nbrs, min_support=MS, **kw)
    got = ctx.fuse_depth(ref, nbrs, min_support=MS, **kw)
    _same_rows(got, exp["rows"], name)
    assert len(got) > 0
    _same_rows(_overwritten(*size).fuse_depth(ref, nbrs, **kw), got, name + ": the overwritten store")
    plain = ctx.fuse_depth(ref, nbrs, **kw)
    rc, zero = _fuse_masked_raw(ctx, ref, nbrs, 0, **kw)
    assert rc == 0
    _same_rows(zero, plain, name + ": min_support = 0")
    _same_rows(plain, fm.fuse(depths, costs, mats, ref, nbrs, **kw)["rows"], name + ": unmasked")
    assert len(plain) > len(got)
    # the rows of the masked call are what mvs_fuse_points_device returns
    ctx.fuse_depth(ref, nbrs, min_support=MS, **kw)
    torch.cuda.synchronize()
    dev = torch.as_tensor(mvs_amd._DeviceArray(ctx.fuse_points_device(), (len(got), 7), "<f4"), device="cuda").cpu().numpy()
    assert dev.tobytes() == got.tobytes()


def test_fuse_depth_masked_errors():
    size = sc.SIZES[2]
    ctx, _ = _context(*size)
    lib, h = ctx.lib, ctx.h
    good = lambda: _fuse_masked_raw(ctx, fc.ROLLED, [fc.TILTED, fc.WIDE], MS)   # noqa: E731
    rc, rows = good()
    assert rc == 0 and len(rows) > 0
    for ms in (-1, 256):
        assert _fuse_masked_raw(ctx, fc.ROLLED, [fc.TILTED, fc.WIDE], ms)[0] == EINVAL and b"min_support" in lib.mvs_last_error(h)
        assert good()[1].tobytes() == rows.tobytes()
    assert _fuse_masked_raw(ctx, fc.ROLLED, [fc.ROLLED], MS, min_consistent=1)[0] == EINVAL
    assert _fuse_masked_raw(ctx, fc.ROLLED, [fc.DEPTH_CAP], MS, min_consistent=1)[0] == EINVAL
    assert _fuse_masked_raw(ctx, fc.ROLLED, [fc.TILTED], MS, min_consistent=2)[0] == EINVAL
    assert good()[1].tobytes() == rows.tobytes()
    for victim in (fc.ROLLED, fc.WIDE):   # the reference's plane, a neighbour's plane
        ctx.depth_support_drop(victim)
        assert good()[0] == ESTATE and b"no support plane" in lib.mvs_last_error(h)
        assert _fuse_masked_raw(ctx, fc.ROLLED, [fc.TILTED, fc.WIDE], 0)[0] == 0   # planes are not read and need not exist
        ctx.depth_support_upload(victim, sc.planes(*size)[victim])
        assert good()[1].tobytes() == rows.tobytes()


# ---- mvs_tsdf_integrate_masked ----------------------------------------------------------------------------------------------------------------
def _fields(ctx, frames):
    return ctx.tsdf_fetch() + ((ctx.tsdf_appearance_fetch(),) if frames else ())


def _same_fields(got, exp, what):
    assert np.array_equal(got[1], exp[1]), "%s: %d counts differ" % (what, int((got[1] != exp[1]).sum()))
    assert got[0].tobytes() == exp[0].tobytes(), "%s: %d sums differ" % (what, int((got[0].view(u32) != exp[0].view(u32)).sum()))
    if len(exp) > 2:
        assert np.array_equal(got[2], exp[2]), "%s: %d cells differ" % (what, int((got[2] != exp[2]).sum()))


@pytest.mark.parametrize("frames", [False, True], ids=["plain", "frames"])
def test_tsdf_integrate_masked(frames):
    size, G = sc.SIZES[0], 16
    slots = fc.TSDF_LIST[:17]   # two chunks of 16
    fslots = [f for _, f in fc.pairs(slots)]
    ctx, mats = _context(*size)
    other = _overwritten(*size)
    depths, costs, supports = _maps(size)
    origin, h = fc.cube(G)
    lib = ctx.lib
    sl, fs = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(fslots, np.int32)
    for max_cost in (INF, float(fc.MAX_COST)):
        what = "max_cost %g" % max_cost
        vol = sm.integrate_masked(am.Volume(G, origin, h, 4 * h), depths, costs, supports, mats, slots, MS, max_cost, fc.store(*size)["frames"] if frames else None,
                                  fslots if frames else None)
        exp = (vol.sum, vol.count) + ((vol.cells,) if frames else ())
        ctx.tsdf_volume(G, origin, h, 4 * h)
        if frames:
            ctx.tsdf_integrate_frames(slots, fslots, max_cost=max_cost, min_support=MS)
        else:
            ctx.tsdf_integrate(slots, max_cost=max_cost, min_support=MS)
        got = _fields(ctx, frames)
        _same_fields(got, exp, what + ": the mirror")
        other.tsdf_volume(G, origin, h, 4 * h)
        if frames:
            other.tsdf_integrate_frames(slots, fslots, max_cost=max_cost)
        else:
            other.tsdf_integrate(slots, max_cost=max_cost)
        _same_fields(_fields(other, frames), got, what + ": the overwritten store")
        # min_support = 0 through the new entry point: today's calls' bytes
        ctx.tsdf_volume(G, origin, h, 4 * h)
        if frames:
            ctx.tsdf_integrate_frames(slots, fslots, max_cost=max_cost)
        else:
            ctx.tsdf_integrate(slots, max_cost=max_cost)
        plain = _fields(ctx, frames)
        ctx.tsdf_volume(G, origin, h, 4 * h)
        assert lib.mvs_tsdf_integrate_masked(ctx.h, len(slots), _ip(sl), _ip(fs) if frames else None, max_cost, 0) == 0
        _same_fields(_fields(ctx, frames), plain, what + ": min_support = 0")
        assert (plain[1] != got[1]).any() and got[1].sum() > 0.3 * plain[1].sum()
    # refusals, each followed by a call that succeeds
    ctx.tsdf_volume(G, origin, h, 4 * h)
    for ms in (-1, 256):
        assert lib.mvs_tsdf_integrate_masked(ctx.h, len(slots), _ip(sl), None, INF, ms) == EINVAL and b"min_support" in lib.mvs_last_error(ctx.h)
    ctx.depth_support_drop(slots[16])
    assert lib.mvs_tsdf_integrate_masked(ctx.h, len(slots), _ip(sl), None, INF, MS) == ESTATE and b"no support plane" in lib.mvs_last_error(ctx.h)
    assert lib.mvs_tsdf_integrate_masked(ctx.h, len(slots), _ip(sl), None, INF, 0) == 0
    ctx.depth_support_upload(slots[16], sc.planes(*size)[slots[16]])
    assert lib.mvs_tsdf_integrate_masked(ctx.h, len(slots), _ip(sl), None, INF, MS) == 0 and ctx.tsdf_fetch()[1].any()


# ---- mvs_fuse_sequence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_support", [0, MS])
@pytest.mark.parametrize("order", sorted(sc.ORDERS))
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_fuse_sequence(size, order, min_support):
    """rows, per-reference counts and total equal the mirror; the counting call; the same call twice; device rows equal downloaded rows"""
    ctx, mats = _context(*size)
    refs = sc.ORDERS[order]
    exp = sc.expected(size, order, min_support, mats, "device")
    rows, counts = ctx.fuse_sequence(refs, sc.lists(refs), min_support=min_support, **sc.SEQ_KW)
    assert np.array_equal(counts, exp["counts"]), (counts, exp["counts"])
    _same_rows(rows, exp["rows"], "order %s" % order)
    assert exp["total"] > 0
    # the counting call: totals without rows, no row buffer written
    rc, total, cnt = _sequence_raw(ctx, refs, sc.padded(refs), min_support)
    assert rc == 0 and total == exp["total"] and np.array_equal(cnt, exp["counts"])
    # the same call twice (S1 clears the planes), and the rows on the device
    again, _ = ctx.fuse_sequence(refs, sc.lists(refs), min_support=min_support, max_rows=exp["total"], **sc.SEQ_KW)
    assert again.tobytes() == rows.tobytes()
    none, counts = ctx.fuse_sequence(refs, sc.lists(refs), min_support=min_support, max_rows=exp["total"], copy=False, **sc.SEQ_KW)
    assert none is None and np.array_equal(counts, exp["counts"])
    torch.cuda.synchronize()
    dev = torch.as_tensor(mvs_amd._DeviceArray(ctx.fuse_sequence_points_device(), (exp["total"], 7), "<f4"), device="cuda").cpu().numpy()
    assert dev.tobytes() == rows.tobytes()


@pytest.mark.parametrize("size", sc.SEQ_SIZES, ids=lambda s: "%dx%d" % s)
def test_fuse_sequence_max_rows(size):
    """max_rows = total - 1 and = 1: the rows that fit are equal, the total is unchanged, the host buffer behind them is untouched"""
    ctx, mats = _context(*size)
    refs = sc.ORDERS["b"]
    exp = sc.expected(size, "b", MS, mats, "device")
    total = exp["total"]
    for fit in (total - 1, 1, total + 5):
        out = np.full((total + 8, 7), np.float32(-77.0), f32)
        rc, n, cnt = _sequence_raw(ctx, refs, sc.padded(refs), MS, max_rows=fit, out=out)
        assert rc == 0 and n == total and np.array_equal(cnt, exp["counts"])
        k = min(fit, total)
        assert out[:k].tobytes() == exp["rows"][:k].tobytes() and (out[k:] == np.float32(-77.0)).all(), fit
    # the optional outputs: no counts, rows left on the device
    rc, n, cnt = _sequence_raw(ctx, refs, sc.padded(refs), MS, max_rows=total, counts=False)
    assert rc == 0 and n == total and (cnt == -7).all()


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_one_reference_is_the_single_call(size):
    ctx, _ = _context(*size)
    ref = fc.WIDE
    nbrs = sc.NEIGHBOURS[ref]
    for ms in (0, MS):
        rows, counts = ctx.fuse_sequence([ref], [nbrs], min_support=ms, **sc.SEQ_KW)
        single = ctx.fuse_depth(ref, nbrs, min_support=ms, **sc.SEQ_KW)
        assert rows.tobytes() == single.tobytes() and counts.tolist() == [len(single)] and len(single) > 0


def test_fuse_sequence_errors():
    """every refusal is followed by a call that succeeds and gives the same bytes"""
    size = sc.SIZES[2]
    ctx, mats = _context(*size)
    lib, h = ctx.lib, ctx.h
    refs = sc.ORDERS["a"]
    nb = sc.padded(refs)
    exp = sc.expected(size, "a", MS, mats, "device")

    def good():
        out = np.zeros((exp["total"], 7), f32)
        rc, n, cnt = _sequence_raw(ctx, refs, nb, MS, max_rows=exp["total"], out=out)
        assert rc == 0 and n == exp["total"] and out.tobytes() == exp["rows"].tobytes() and np.array_equal(cnt, exp["counts"])

    good()
    twice = [refs[0], refs[1], refs[0]]
    other = nb.copy()
    other[1, 0] = refs[1]   # a neighbour that is its reference
    outside = nb.copy()
    outside[2, 1] = fc.DEPTH_CAP
    negative = nb.copy()
    negative[0, 1] = -2     # only -1 means none
    refusals = [
        ("nrefs", dict(nrefs=0), EINVAL), ("nrefs", dict(nrefs=fc.DEPTH_CAP + 1), EINVAL), ("ref_slots is null", dict(refs_null=True), EINVAL),
        ("out_count is null", dict(total=False), EINVAL), ("listed twice", dict(refs=twice, nb=nb[[0, 1, 0]]), EINVAL),
        ("nneighbours", dict(nneighbours=17), EINVAL), ("nneighbours", dict(nneighbours=-1), EINVAL), ("max_rows", dict(max_rows=-1), EINVAL),
        ("is the reference slot", dict(nb=other), EINVAL), ("outside the depth store", dict(nb=outside), EINVAL),
        ("outside the depth store", dict(nb=negative), EINVAL), ("outside the depth store", dict(refs=[fc.DEPTH_CAP] + list(refs[1:])), EINVAL),
        ("min_support", dict(min_support=256), EINVAL), ("min_support", dict(min_support=-1), EINVAL), ("min_consistent", dict(min_consistent=6), EINVAL),
        ("thresholds", dict(max_reproj_px=-1.0), EINVAL), ("thresholds", dict(max_rel_depth=float("nan")), EINVAL),
    ]
    for needle, change, code in refusals:
        kw = dict(refs=refs, nb=nb, min_support=MS, max_rows=0)
        kw.update(change)
        rc, n, _ = _sequence_raw(ctx, kw.pop("refs"), kw.pop("nb"), **kw)
        assert rc == code and needle.encode() in lib.mvs_last_error(h), (needle, rc, lib.mvs_last_error(h))
        assert n in (0, -5)
        good()
    # state: a plane missing under min_support > 0 (fine under 0); a finite max_cost and a slot stored without a cost map; an empty slot
    ctx.depth_support_drop(fc.AXIS)
    assert _sequence_raw(ctx, refs, nb, MS)[0] == ESTATE and b"no support plane" in lib.mvs_last_error(h)
    assert _sequence_raw(ctx, refs, nb, 0)[0] == 0
    ctx.depth_support_upload(fc.AXIS, sc.planes(*size)[fc.AXIS])
    good()
    with mvs_amd.Context(*size) as bare:
        st = fc.store(*size)
        bare.depth_store(3)
        one = np.zeros((1, 1), np.int32)
        assert _sequence_raw(bare, [0], one + 1, 0, min_consistent=1)[0] == ESTATE and b"holds no depth map" in bare.lib.mvs_last_error(bare.h)
        bare.depth_upload(0, st["cams"][0], st["depths"][0])
        bare.depth_upload(1, st["cams"][1], st["depths"][1], st["costs"][1])
        assert _sequence_raw(bare, [1], one * 0, 0, min_consistent=1, max_cost=0.5)[0] == ESTATE and b"without a cost map" in bare.lib.mvs_last_error(bare.h)
        assert bare.fuse_sequence_points_device() == 0
        rows, counts = bare.fuse_sequence([1, 0], [[0], [1]], min_consistent=1)
        assert len(rows) == counts.sum() > 0 and bare.fuse_sequence_points_device() != 0
        # no neighbours at all: every reference keeps what has a normal and is unclaimed -- nothing claims
        rows, counts = bare.fuse_sequence([0, 1], [[], []], min_consistent=0)
        assert counts.tolist() == [len(bare.fuse_depth(0, [], min_consistent=0)), len(bare.fuse_depth(1, [], min_consistent=0))]


# ---- propagate_two_stage(support=True) --------------------------------------------------------------------------------------------------------
def test_two_stage_support(oracle):
    """the planes of slots n + i equal the support maps the mirror of the second stage gives, fuse_sequence(min_support = 2) on them equals the
    mirror, and support=False leaves the slots without planes"""
    import band_bestk_cases as bb
    import consistency_mirror as cm
    import propagate_mirror as pm
    from mvs_amd import synth
    from test_consistency_gpu import PROPAGATE, TERM, ZNCC, _run

    W, H, D, r, keep, n = 48, 32, 8, 1, 2, 3
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, 2)
    cams, imgs = [main_cam] + list(side_cams), [main_img] + list(sides)
    cost = dict(cost="zncc", radius=r, keep=keep)
    frame_slots = [4, 1, 3]
    side_slots = [[frame_slots[j] for j in range(n) if j != i] for i in range(n)]
    side_cams_of = [np.stack([cams[j] for j in range(n) if j != i]) for i in range(n)]
    step = 2.0 / D
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.frame_store(5)
        for i in range(n):
            ctx.frame_upload(frame_slots[i], imgs[i])
        ctx.depth_store(2 * n)
        args = (ctx, frame_slots, np.stack(cams), side_slots, np.stack(side_cams_of), D)
        plain = mvs_amd.propagate_two_stage(*args, cost=cost, propagate=PROPAGATE, consistency=TERM)
        for s in range(2 * n):
            with pytest.raises(mvs_amd.MvsError, match="no support plane"):
                ctx.depth_support_fetch(s)
        got = mvs_amd.propagate_two_stage(*args, cost=cost, propagate=PROPAGATE, consistency=TERM, support=True)
        assert got.tobytes() == plain.tobytes()
        planes = {n + i: ctx.depth_support_fetch(n + i) for i in range(n)}
        for i in range(n):
            with pytest.raises(mvs_amd.MvsError, match="no support plane"):
                ctx.depth_support_fetch(i)
        assert np.array_equal(planes[2 * n - 1], ctx.propagate_support()), "the stage still holds the last frame's support map"
        mats = {s: ctx.depth_slot_matrices(s) for s in range(2 * n)}
        scenes = [pm.Scene(oracle, cams[i], imgs[i], side_cams_of[i], [imgs[j] for j in range(n) if j != i]) for i in range(n)]
        first = []
        for i in range(n):
            views = (cams[i], imgs[i], side_cams_of[i], [imgs[j] for j in range(n) if j != i])
            start = bb.global_level(oracle, views, D, -1.0, 1.0, ZNCC, r, keep)[1]
            first.append(_run(pm.State(scenes[i], start, ZNCC, r, keep, slopes=True), PROPAGATE, step))
        for i in range(n):
            term = cm.Term(mats[i], [(mats[j][0], mats[j][1], first[j].z) for j in range(n) if j != i], **TERM)
            second = _run(cm.State(scenes[i], first[i].z, ZNCC, r, keep, slopes=True, term=term), PROPAGATE, step)
            assert second.z.tobytes() == got[i].tobytes()
            assert np.array_equal(planes[n + i], second.support()), "frame %d" % i
        assert set(np.unique(np.stack(list(planes.values())))) == {0, 1, 2}
        # the sequence over the second-stage slots, masked by their planes
        refs = [n + i for i in range(n)]
        lists = [[s for s in refs if s != ref] for ref in refs]
        kw = dict(min_consistent=1, max_reproj_px=2.0, max_rel_depth=0.05)
        depths = {n + i: got[i] for i in range(n)}
        for ms in (0, 2):
            exp = sm.fuse_sequence(depths, {}, planes, mats, refs, lists, min_support=ms, **kw)
            rows, counts = ctx.fuse_sequence(refs, lists, min_support=ms, **kw)
            print("min_support %d: %d rows (%s)" % (ms, exp["total"], exp["counts"]))
            assert np.array_equal(counts, exp["counts"]) and exp["total"] > 0
            _same_rows(rows, exp["rows"], "min_support %d" % ms)


def test_masking_does_not_make_the_occluder_cloud_worse():
    """section 27's estimated maps with their support, stored for all five views of the occluder scene: the share of the sequence cloud's rows
    more than 1.5 plane steps off is recorded; masking by support >= 3 of 4 must not increase it"""
    q = sc.occluder_sequence_quality()
    plain, mask = q[0], q[sc.QUALITY_MIN_SUPPORT]
    print("unmasked: %d rows %s, %.2f %% bad; support >= %d: %d rows %s, %.2f %% bad" %
          (plain["rows"], plain["counts"], plain["bad_share"], sc.QUALITY_MIN_SUPPORT, mask["rows"], mask["counts"], mask["bad_share"]))
    assert 0 < mask["rows"] <= plain["rows"] and mask["bad_share"] <= plain["bad_share"]
