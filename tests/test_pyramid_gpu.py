"""The resolution pyramid on the device (csrc/pyramid.hip), bit-identical to the mirror (tests/pyramid_mirror.py)
throughout: rule D on packed frames, mvs_pyramid_stage behind every staging path of the fine context and down a chain, rule U on crafted
maps, the ordering between the two contexts' streams, the coarse-to-fine helper and every error of the list."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_cases as bc
import band_mirror as bm
import mvs_amd
import pyramid_cases as pc
import pyramid_mirror as pm
from mvs_amd import synth

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _same_floats(got, ref, what):
    """equal as bits"""
    np.testing.assert_array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(ref, np.float32).view(np.uint32), err_msg=what)


def _same_sweep(got, ref, what):
    """(depth, cost, index, packed volume) of two sweeps"""
    for g, r, name in zip(got, ref, ("depth", "cost", "index", "volume")):
        np.testing.assert_array_equal(g, r, err_msg="%s: %s" % (what, name))


def _floats_at(ctx, ptr, H, W):
    """the H x W f32 map at a device address of the context, after its stream has drained"""
    ctx.synchronize()
    return torch.as_tensor(mvs_amd._DeviceArray(ptr, (H, W), "<f4"), device="cuda").cpu().numpy()


def _noise_views(W, H, V, seed):
    """general (unrectified) cameras with i.i.d. frames: every texel counts in rule D"""
    main_cam, _, side_cams, _, _ = bc.general_views(W, H, V)
    rng = np.random.Generator(np.random.PCG64(seed))
    return main_cam, rng.integers(0, 256, (H, W), dtype=np.uint8), side_cams, [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(V)]


# ---- rule D -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,offset", [(72, 40, 0), (70, 42, 0), (72, 40, 1)])
def test_downsample(W, H, offset):
    """72 x 40: coarse rows of 36 bytes, the dword paths; 70 x 42: coarse 35 x 21, the byte paths and a partial last thread; offset 1: a
    source that starts at an odd address"""
    n = 3
    rng = np.random.Generator(np.random.PCG64(W * H + offset))
    frames = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    src = _device(np.concatenate([np.zeros(offset, np.uint8), frames.reshape(-1)]))
    dst = torch.full((n * (H // 2) * (W // 2) + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with mvs_amd.Context(W, H, 0) as ctx:
        ctx.pyramid_downsample_device(src.data_ptr() + offset, dst.data_ptr(), n)
        ctx.synchronize()
    out = dst.cpu().numpy()
    np.testing.assert_array_equal(out[:-8].reshape(n, H // 2, W // 2), pm.downsample(frames))
    assert (out[-8:] == 0xAB).all()        # nothing past the last frame


# ---- stage --------------------------------------------------------------------------------------------------------------------------
def _stage_host(ctx, views, keep):
    ctx.sweep_set(*views, 5)


def _stage_device(ctx, views, keep):
    main_cam, main_img, side_cams, sides = views
    keep += [_device(main_img)] + [_device(s) for s in sides]
    ctx.sweep_set_main_device(main_cam, keep[-1 - len(sides)].data_ptr())
    ctx.sweep_set_views_device(side_cams, [t.data_ptr() for t in keep[-len(sides):]])
    ctx.sweep_set_planes(5)


def _stage_handles(ctx, views, keep):
    main_cam, main_img, side_cams, sides = views
    slots = [2, 5, 1, 3]                 # main, then the side views: not ascending
    ctx.frame_store(6)
    for slot, frame in zip(slots, [main_img] + list(sides)):
        ctx.frame_upload(slot, frame)
    ctx.sweep_handles(slots[0], main_cam, slots[1:], side_cams, 8)     # leaves the slots staged


def _coarse_reference(oracle, views, D, nlevels=2):
    """the sweep of the mirror's frames at the last level: on a context staged from the host, and by the oracle"""
    main_cam, main_img, side_cams, sides = views
    m, s = pc.levels(main_img, sides, nlevels)[-1]
    H, W = m.shape
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ref:
        ref.sweep_set(main_cam, m, side_cams, s, D)
        ref.sweep_run(0, len(s), BOTH)
        host = ref.sweep_fetch(want_volume=True)
    orc = oracle.sweep(main_cam, m, side_cams, s, D, want_volume=True, nthreads=4, sampler="fixed")
    _same_sweep(host, orc, "host-staged context against the oracle")
    assert len(np.unique(host[2])) > 3 and (host[3] >> 24).max() == len(s)
    return host


@pytest.fixture(scope="module")
def stage_case(oracle):
    views = _noise_views(76, 44, 3, 0x57A6E)
    return views, _coarse_reference(oracle, views, 9)


@pytest.mark.parametrize("stage", [_stage_host, _stage_device, _stage_handles])
def test_stage(stage_case, stage):
    views, ref = stage_case
    keep = []
    with mvs_amd.Context(76, 44, 0, sampler="fixed") as fine, mvs_amd.Context(38, 22, 0, sampler="fixed") as coarse:
        stage(fine, views, keep)
        fine.pyramid_stage(coarse)
        coarse.sweep_set_planes(9)
        coarse.sweep_run(0, 3, BOTH)
        _same_sweep(coarse.sweep_fetch(want_volume=True), ref, stage.__name__)
        # again, over what the first call left on the coarse context
        fine.pyramid_stage(coarse)
        coarse.sweep_run(0, 3, BOTH)
        _same_sweep(coarse.sweep_fetch(want_volume=True), ref, stage.__name__ + ", staged twice")


def test_stage_chain(oracle):
    views = _noise_views(80, 48, 3, 0xC4A12)
    ref = _coarse_reference(oracle, views, 9, nlevels=3)
    with mvs_amd.Context(80, 48, 0) as full, mvs_amd.Context(40, 24, 0) as half, mvs_amd.Context(20, 12, 0) as quarter:
        full.sweep_set(*views, 5)
        full.pyramid_stage(half)
        half.pyramid_stage(quarter)
        quarter.sweep_set_planes(9)
        quarter.sweep_run(0, 3, BOTH)
        _same_sweep(quarter.sweep_fetch(want_volume=True), ref, "80 x 48 -> 40 x 24 -> 20 x 12")


# ---- rule U -------------------------------------------------------------------------------------------------------------------------
def test_prior(oracle):
    c = pc.crafted_prior()
    Wc, Hc, W, H, V = c.Wc, c.Hc, 2 * c.Wc, 2 * c.Hc, 3
    main_cam, _, side_cams, sides = _noise_views(W, H, V, 0x9120)
    explicit = _device(c.depth)
    with mvs_amd.Context(W, H, 0) as fine, mvs_amd.Context(Wc, Hc, 0) as coarse:
        assert fine.sweep_band_pointers() == (0, 0)
        fine.sweep_set(main_cam, c.fine_guide, side_cams, sides, 5, -0.1, 0.1)
        coarse.sweep_set(main_cam, c.coarse_guide, side_cams, [pm.downsample(s) for s in sides], 4)
        # the coarse context's own map: a sweep's, then overwritten with the crafted one through its device pointer
        coarse.sweep_run(0, V, BOTH)
        coarse.synchronize()
        own = torch.as_tensor(mvs_amd._DeviceArray(coarse.sweep_result_pointers()[0], (Hc, Wc), "<f4"), device="cuda")
        own.copy_(explicit)
        torch.cuda.synchronize()
        refs = {}
        for tau in (255, 20, 0):
            refs[tau] = pm.prior(c.depth, tau, c.coarse_guide, c.fine_guide)
            for ptr, how in ((explicit.data_ptr(), "explicit pointer"), (None, "the coarse context's map")):
                got_ptr = fine.pyramid_prior(coarse, ptr, tau)
                assert got_ptr and got_ptr == fine.sweep_band_pointers()[1]
                _same_floats(_floats_at(fine, got_ptr, H, W), refs[tau], "tau %d, %s" % (tau, how))
        assert not np.array_equal(refs[255], refs[20]) and not np.array_equal(refs[20], refs[0])
        assert np.isnan(c.depth).any() and (refs[255] == 1.0).any() and not np.isnan(refs[255]).any()
        # a band run on the buffer itself (no copy: band.hip skips it for this pointer)
        ptr = fine.pyramid_prior(coarse, None, 20)
        fine.sweep_run_band(ptr, 0, V, BOTH)
        got = fine.sweep_fetch(want_volume=True)
        delta = oracle.plane_table(5, -0.1, 0.1)
        vol = bm.band_volume(oracle, main_cam, c.fine_guide, side_cams, sides, refs[20], delta)
        _same_sweep(got, oracle.argmin(vol, delta, sampler="fixed") + (vol,), "band run on the pyramid's prior")
        assert (vol != 0).mean() > 0.3


# ---- helper and ordering ------------------------------------------------------------------------------------------------------------
def _scene(W, H, V, seed):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, seed=seed, freq_scale=0.4)
    return main_cam, main_img, side_cams, sides


@pytest.mark.parametrize("nlevels,tau", [(2, 255), (3, 255), (2, 20)])
def test_helper(oracle, nlevels, tau):
    W, H, V, DC, DB = 80, 48, 4, 16, 16
    views = _scene(W, H, V, synth.SEED_SCENE)
    depth, prior, vol, maps = pc.coarse_to_fine(oracle, *views, nlevels, DC, DB, 1.5, tau)
    ctxs = [mvs_amd.Context(W >> k, H >> k, 0) for k in range(nlevels)]
    try:
        ctxs[0].sweep_set(*views, 1)
        got = mvs_amd.pyramid_coarse_to_fine(ctxs, DC, DB, 1.5, tau=tau)
        _same_floats(got, depth, "pyramid_coarse_to_fine, %d levels, tau %d" % (nlevels, tau))
        _same_sweep(ctxs[0].sweep_fetch(want_volume=True), maps + (vol,), "the finest level's band")
        _same_floats(_floats_at(ctxs[0], ctxs[0].sweep_band_pointers()[1], H, W), prior, "the finest level's prior")
        assert ctxs[0].sweep_band_report() == bm.report(prior, maps[0], maps[2], DB)
        assert (np.asarray(depth) != 1.0).mean() > 0.9
    finally:
        for ctx in ctxs:
            ctx.close()


def test_a_context_without_a_pyramid_is_unchanged(oracle):
    W, H, V, D = 80, 48, 4, 12
    views = _scene(W, H, V, synth.SEED_SCENE)
    with mvs_amd.Context(W, H, 0) as ctx:
        ctx.sweep_set(*views, D)
        ctx.sweep_run(0, V, BOTH)
        _same_sweep(ctx.sweep_fetch(want_volume=True), oracle.sweep(*views, D, want_volume=True, nthreads=4, sampler="fixed"), "plain sweep")
        assert ctx.sweep_band_pointers() == (0, 0)      # and nothing of the band or the pyramid was allocated


def _helper_with_waits(ctxs, DC, DB, tau):
    """pyramid_coarse_to_fine call for call, the host waiting for every context after every step"""
    def wait():
        for ctx in ctxs:
            ctx.synchronize()

    for above, below in zip(ctxs, ctxs[1:]):
        above.pyramid_stage(below)
        wait()
    ctxs[-1].sweep_set_planes(DC, -1.0, 1.0)
    ctxs[-1].sweep_run(0, None, BOTH)
    wait()
    ctxs[-1].sweep_refine_depth()
    wait()
    step, ptr = 2.0 / DC, None
    for level in range(len(ctxs) - 2, -1, -1):
        ctx = ctxs[level]
        ctx.pyramid_prior(ctxs[level + 1], ptr, tau)
        wait()
        hb = float(np.float32(1.5 * step))
        ctx.sweep_set_planes(DB, -hb, hb)
        ctx.sweep_run_band(ctx.sweep_band_pointers()[1], 0, None, BOTH)
        wait()
        ctx.sweep_refine_depth()
        wait()
        out = ctx.sweep_band_resolve(fetch=True)
        wait()
        ptr, step = ctx.sweep_band_pointers()[0], 2.0 * hb / DB
    return out


def test_ordering_between_the_streams():
    """two frames through the three-level helper back to back: frames staged from device memory (no host wait), fetch=False, each result
    parked in a depth-store slot by a stream-ordered copy; nothing waits until both are queued"""
    W, H, V, DC, DB, tau = 80, 48, 4, 16, 16, 20
    scenes = [_scene(W, H, V, synth.SEED_SCENE), _scene(W, H, V, synth.SEED_SCENE + 7)]
    assert not np.array_equal(scenes[0][1], scenes[1][1])
    frames = [[_device(f) for f in [s[1]] + list(s[3])] for s in scenes]

    def stage(ctx, k):
        ctx.sweep_set_main_device(scenes[k][0], frames[k][0].data_ptr())
        ctx.sweep_set_views_device(scenes[k][2], [t.data_ptr() for t in frames[k][1:]])

    def contexts():
        return [mvs_amd.Context(W >> k, H >> k, 0) for k in range(3)]

    ctxs = contexts()
    try:
        refs = []
        for k in range(2):
            stage(ctxs[0], k)
            refs.append(_helper_with_waits(ctxs, DC, DB, tau))
    finally:
        for ctx in ctxs:
            ctx.close()
    assert not np.array_equal(refs[0], refs[1])
    ctxs = contexts()
    try:
        ctxs[0].depth_store(2)
        for k in range(2):
            stage(ctxs[0], k)
            assert mvs_amd.pyramid_coarse_to_fine(ctxs, DC, DB, 1.5, tau=tau, fetch=False) is None
            ctxs[0].depth_upload_device(k, scenes[k][0], ctxs[0].sweep_band_pointers()[0])
        for k in range(2):
            _same_floats(_floats_at(ctxs[0], ctxs[0].depth_slot_pointer(k), H, W), refs[k], "frame %d without waits" % k)
    finally:
        for ctx in ctxs:
            ctx.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_errors(oracle):
    W, H, V = 76, 44, 3
    views = _noise_views(W, H, V, 0x57A6E)
    ref = _coarse_reference(oracle, views, 9)
    rng = np.random.Generator(np.random.PCG64(3))
    zc = rng.uniform(-0.9, 0.9, (H // 2, W // 2)).astype(np.float32)
    zc_dev, src = _device(zc), _device(np.stack([views[1]] + list(views[3])))
    dst = torch.zeros(((V + 1) * (H // 2) * (W // 2),), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    zp, sp, dp = C.c_void_p(zc_dev.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    with mvs_amd.Context(W, H, 0) as fine, mvs_amd.Context(W // 2, H // 2, 0) as coarse, mvs_amd.Context(W // 2, H // 2 + 1, 0) as wrong, \
            mvs_amd.Context(W + 1, H, 0) as odd, mvs_amd.Context(W, H + 1, 0) as odd_rows:
        lib, f, c = fine.lib, fine.h, coarse.h

        def good(what):
            """a valid call of each entry after the refused one, against the mirror"""
            fine.pyramid_downsample_device(src.data_ptr(), dst.data_ptr(), V + 1)
            fine.synchronize()
            np.testing.assert_array_equal(dst.cpu().numpy().reshape(V + 1, H // 2, W // 2), pm.downsample(src.cpu().numpy()), err_msg=what)
            if fine_staged:
                fine.pyramid_stage(coarse)
                coarse.sweep_set_planes(9)
                coarse.sweep_run(0, V, BOTH)
                _same_sweep(coarse.sweep_fetch(want_volume=True), ref, what)
                tau, guides = 20, (pm.downsample(views[1]), views[1])
            else:
                tau, guides = 255, (None, None)
            _same_floats(_floats_at(fine, fine.pyramid_prior(coarse, zc_dev.data_ptr(), tau), H, W), pm.prior(zc, tau, *guides), what)

        fine_staged = False
        # mvs_pyramid_downsample_device
        for args in ((None, sp, dp, 1), (f, None, dp, 1), (f, sp, None, 1), (f, sp, dp, 0), (f, sp, dp, -3), (f, sp, dp, 65536), (f, sp, sp, 1),
                     (f, sp, C.c_void_p(src.data_ptr() + W * H - 1), 1), (f, C.c_void_p(dst.data_ptr() + 5), dp, 1), (odd.h, sp, dp, 1)):
            assert lib.mvs_pyramid_downsample_device(*args) == EINVAL, args
        assert b"overlap" in lib.mvs_last_error(f) and b"even" in lib.mvs_last_error(odd.h)
        good("after the downsample's EINVALs")
        # the pair
        for fn in (lambda a, b: lib.mvs_pyramid_stage(a, b), lambda a, b: lib.mvs_pyramid_prior(a, b, zp, 255)):
            for a, b in ((None, c), (f, None), (None, None), (f, f), (f, wrong.h), (f, odd.h), (c, f), (odd.h, c), (odd_rows.h, c)):
                assert fn(a, b) == EINVAL, (a, b)
        devices = torch.cuda.device_count()
        if devices > 1:
            with mvs_amd.Context(W // 2, H // 2, 1) as other:
                assert lib.mvs_pyramid_stage(f, other.h) == EINVAL and b"devices" in lib.mvs_last_error(f)
                assert lib.mvs_pyramid_prior(f, other.h, zp, 255) == EINVAL
        for tau in (-1, 256, 1000):
            assert lib.mvs_pyramid_prior(f, c, zp, tau) == EINVAL and b"tau" in lib.mvs_last_error(f)
        good("after the pair's EINVALs")
        # states: nothing staged on the fine context; no depth map on the coarse one; no guides
        assert lib.mvs_pyramid_stage(f, c) == ESTATE and b"main view" in lib.mvs_last_error(f)
        fine.sweep_set_main(views[0], views[1])
        assert lib.mvs_pyramid_stage(f, c) == ESTATE
        assert lib.mvs_pyramid_prior(f, c, None, 255) == ESTATE and b"depth map" in lib.mvs_last_error(f)
        assert lib.mvs_pyramid_prior(f, c, zp, 20) == ESTATE and b"main image" in lib.mvs_last_error(f)      # the coarse context has no main image
        assert lib.mvs_pyramid_prior(f, c, zp, 254) == ESTATE
        good("after the ESTATEs of empty contexts")
        fine.sweep_set(*views, 5)
        fine_staged = True
        for who in (fine, coarse):
            who.set_sampler("exact")
            assert lib.mvs_pyramid_stage(f, c) == ESTATE and b"FIXED" in lib.mvs_last_error(f)
            who.set_sampler("fixed")
        good("after the exact sampler")
        # the coarse context's guide alone is missing: a fresh fine / coarse pair, the fine one staged
        with mvs_amd.Context(W // 2, H // 2, 0) as bare:
            assert lib.mvs_pyramid_prior(f, bare.h, zp, 20) == ESTATE
            assert lib.mvs_pyramid_prior(f, bare.h, None, 255) == ESTATE
            assert bare.sweep_band_pointers() == (0, 0)
        good("the contexts stay usable")
