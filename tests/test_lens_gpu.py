"""The lens on the device (csrc/lens.hip): every comparison is exact equality with tests/lens_mirror.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import lens_mirror
import lens_scenes
import mvs_amd
import scenes
from mvs_amd import synth

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
SMALL = (67, 35)      # neither dimension is a multiple of the 64 x 4 workgroup: partial workgroups on both edges


def _frames(W, H):
    return {"noise": lens_scenes.noise(W, H), "checkerboard": lens_scenes.checkerboard(W, H), "white": np.full((H, W), 255, np.uint8)}


@pytest.mark.parametrize("lens", lens_scenes.LENS_NAMES)
def test_map_and_frames_equal_the_mirror_at_a_ragged_size(lens):
    W, H = SMALL
    k, c = lens_scenes.lenses(W, H)[lens]
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(k, c)
        got_k, got_c = ctx.lens()
        np.testing.assert_array_equal(got_k, lens_mirror.k_of(k))
        assert got_c == (float(np.float32(c[0])), float(np.float32(c[1])))
        np.testing.assert_array_equal(ctx.undistort_map(), lens_mirror.undistort_map(W, H, k, c))
        for name, frame in _frames(W, H).items():
            np.testing.assert_array_equal(ctx.undistort(frame), lens_mirror.undistort(frame, k, c), err_msg=name)


def test_map_and_frame_equal_the_mirror_at_640_x_480():
    W, H = 640, 480
    k, c = lens_scenes.lenses(W, H)["koberec"]
    frame = lens_scenes.noise(W, H, seed=21)
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(k, c)
        np.testing.assert_array_equal(ctx.undistort_map(), lens_mirror.undistort_map(W, H, k, c))
        np.testing.assert_array_equal(ctx.undistort(frame), lens_mirror.undistort(frame, k, c))


def test_three_frames_in_one_launch_equal_three_calls_and_aliasing_is_refused():
    W, H = SMALL
    k, c = lens_scenes.lenses(W, H)["offcentre"]
    frames = np.stack([lens_scenes.noise(W, H, seed=s) for s in (1, 2, 3)])
    src = torch.as_tensor(frames, device="cuda").contiguous()
    dst = torch.full_like(src, 77)
    torch.cuda.synchronize()
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(k, c)
        singles = np.stack([ctx.undistort(f) for f in frames])
        ctx.undistort_device(src.data_ptr(), dst.data_ptr(), 3)
        ctx.synchronize()
        np.testing.assert_array_equal(dst.cpu().numpy(), singles)
        np.testing.assert_array_equal(singles, np.stack([lens_mirror.undistort(f, k, c) for f in frames]))
        # src == dst, and ranges that overlap by one frame: refused, nothing written
        P = W * H
        for s, d, n in ((src.data_ptr(), src.data_ptr(), 3), (src.data_ptr(), src.data_ptr() + P, 2), (src.data_ptr() + P, src.data_ptr(), 2)):
            assert ctx.lib.mvs_undistort_device(ctx.h, s, d, n) == EINVAL
        assert ctx.lib.mvs_undistort_device(ctx.h, src.data_ptr(), dst.data_ptr(), 0) == EINVAL
        ctx.synchronize()
        np.testing.assert_array_equal(src.cpu().numpy(), frames)
        # disjoint halves of one allocation are fine
        ctx.undistort_device(src.data_ptr(), src.data_ptr() + 2 * P, 1)
        ctx.synchronize()
        np.testing.assert_array_equal(src.cpu().numpy()[2], singles[0])


@pytest.mark.parametrize("size", [SMALL, (640, 480)])
def test_identity_lens_returns_the_input(size):
    W, H = size
    frame = lens_scenes.noise(W, H, seed=9)
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens((0.0, 0.0, 0.0))                 # centre: the frame's
        np.testing.assert_array_equal(ctx.undistort(frame), frame)


@pytest.fixture(scope="module")
def lens_views():
    """96 x 64, 2 side views seen through koberec's lens, and the mirror's undistorted frames"""
    W, H, V = 96, 64, 2
    k, c = lens_scenes.lenses(W, H)["koberec"]
    main_cam, d_main, side_cams, d_sides, _ = lens_scenes.make_views(W, H, V, k, c, radius=0.25)
    return {"W": W, "H": H, "V": V, "k": k, "c": c, "main_cam": main_cam, "side_cams": side_cams, "main": d_main, "sides": d_sides,
            "u_main": lens_mirror.undistort(d_main, k, c), "u_sides": [lens_mirror.undistort(s, k, c) for s in d_sides]}


def test_lens_uploads_feed_the_sweep_and_the_frame_pipeline(oracle, lens_views):
    v = lens_views
    W, H, V, D = v["W"], v["H"], v["V"], 16
    ref = oracle.sweep(v["main_cam"], v["u_main"], v["side_cams"], v["u_sides"], D, nthreads=4, sampler="fixed")[:3]
    verts, faces = scenes.heightfield_mesh(48, extent=1.4)
    side_t = torch.as_tensor(v["sides"][1], device="cuda").contiguous()
    torch.cuda.synchronize()
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(v["k"], v["c"])
        ctx.frame_store(4)
        ctx.frame_upload(2, v["main"], lens=True)
        ctx.frame_upload(0, v["sides"][0], lens=True)
        ctx.frame_upload_device(3, side_t.data_ptr(), lens=True)         # the device form, straight into the slot
        depth, cost = ctx.sweep_handles(2, v["main_cam"], [0, 3], v["side_cams"], D, want_cost=True)
        index = ctx.sweep_fetch()[2]
        np.testing.assert_array_equal(depth, ref[0])
        np.testing.assert_array_equal(cost, ref[1])
        np.testing.assert_array_equal(index, ref[2])
        ctx.load_mesh(verts, faces)
        for farneback in (False, True):
            exp, exp_depth = ctx.process_frame(v["main_cam"], v["u_main"], v["side_cams"], v["u_sides"], farneback, want_depth=True)
            pts, d_after = ctx.process_frame_slots(v["main_cam"], 2, v["side_cams"], [0, 3], farneback, want_depth=True)
            np.testing.assert_array_equal(d_after, exp_depth)
            np.testing.assert_array_equal(pts, exp)
    # the premise: the lens frames as they are give another answer
    assert (oracle.sweep(v["main_cam"], v["main"], v["side_cams"], v["sides"], D, nthreads=4, sampler="fixed")[0] != ref[0]).any()


def test_lens_upload_equals_undistort_then_upload(lens_views):
    """the slot's bytes through the device form with the frame INSIDE the store's own slot (staged), and plain uploads beside a set lens"""
    v = lens_views
    W, H, V, D = v["W"], v["H"], v["V"], 16
    with mvs_amd.Context(W, H) as plain:
        plain.frame_store(3)
        plain.frame_upload(0, v["main"])
        plain.frame_upload(1, v["sides"][0])
        plain.frame_upload(2, v["sides"][1])
        d_plain, c_plain = plain.sweep_handles(0, v["main_cam"], [1, 2], v["side_cams"], D, want_cost=True)
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(v["k"], v["c"])
        ctx.frame_store(3)
        # plain uploads beside a set lens are unchanged, byte for byte, against a context without a lens
        ctx.frame_upload(0, v["main"])
        ctx.frame_upload(1, v["sides"][0])
        ctx.frame_upload(2, v["sides"][1])
        d, c = ctx.sweep_handles(0, v["main_cam"], [1, 2], v["side_cams"], D, want_cost=True)
        np.testing.assert_array_equal(d, d_plain)
        np.testing.assert_array_equal(c, c_plain)
        # undistort then upload == upload through the lens
        for s, f in enumerate([v["main"]] + v["sides"]):
            ctx.frame_upload(s, ctx.undistort(f))
        d_two, c_two = ctx.sweep_handles(0, v["main_cam"], [1, 2], v["side_cams"], D, want_cost=True)
        for s, f in enumerate([v["main"]] + v["sides"]):
            ctx.frame_upload(s, f, lens=True)
        d_one, c_one = ctx.sweep_handles(0, v["main_cam"], [1, 2], v["side_cams"], D, want_cost=True)
        np.testing.assert_array_equal(d_one, d_two)
        np.testing.assert_array_equal(c_one, c_two)
        assert (d_one != d_plain).any()


def test_state_a_context_carries(oracle, lens_views):
    v = lens_views
    W, H, D = v["W"], v["H"], 16
    frame = v["main"]
    out = np.full((H, W), 5, np.uint8)
    u8p = mvs_amd._u8p
    with mvs_amd.Context(W, H) as ctx:
        assert ctx.lens() is None
        ctx.set_lens(v["k"], v["c"])
        np.testing.assert_array_equal(ctx.undistort(frame), v["u_main"])
        ctx.set_lens(None)                                                # cleared: MVS_ESTATE is back
        assert ctx.lens() is None
        assert ctx.lib.mvs_undistort(ctx.h, mvs_amd._ptr(frame, u8p), mvs_amd._ptr(out, u8p)) == ESTATE
        assert (out == 5).all()
        # a changed lens between two uploads affects only the second slot
        k2, c2 = lens_scenes.lenses(W, H)["pincushion"]
        ctx.frame_store(3)
        ctx.set_lens(v["k"], v["c"])
        ctx.frame_upload(0, v["main"], lens=True)
        ctx.frame_upload(1, v["sides"][0], lens=True)
        ctx.set_lens(k2, c2)
        ctx.frame_upload(2, v["sides"][1], lens=True)
        got = ctx.sweep_handles(0, v["main_cam"], [1, 2], v["side_cams"], D)
    exp = oracle.sweep(v["main_cam"], v["u_main"], v["side_cams"], [v["u_sides"][0], lens_mirror.undistort(v["sides"][1], k2, c2)], D, nthreads=4,
                       sampler="fixed")[0]
    np.testing.assert_array_equal(got, exp)
    # two contexts of different sizes taking turns
    Wb, Hb = SMALL
    kb, cb = lens_scenes.lenses(Wb, Hb)["offcentre"]
    fb = lens_scenes.noise(Wb, Hb, seed=4)
    with mvs_amd.Context(W, H) as a, mvs_amd.Context(Wb, Hb) as b:
        a.set_lens(v["k"], v["c"])
        b.set_lens(kb, cb)
        for _ in range(2):
            np.testing.assert_array_equal(a.undistort(frame), v["u_main"])
            np.testing.assert_array_equal(b.undistort(fb), lens_mirror.undistort(fb, kb, cb))
            np.testing.assert_array_equal(b.undistort_map(), lens_mirror.undistort_map(Wb, Hb, kb, cb))


def test_every_error():
    W, H = SMALL
    P = W * H
    frame = lens_scenes.noise(W, H)
    out = np.full((H, W), 5, np.uint8)
    fmap = np.full((H, W, 2), 5, np.float32)
    u8p, fp = mvs_amd._u8p, mvs_amd._fp
    dev = torch.zeros(2 * P, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def k3(*k):
        return mvs_amd._ptr(np.asarray(k, np.float32), fp)

    with mvs_amd.Context(W, H) as ctx:
        lib, h = ctx.lib, ctx.h
        # mvs_set_lens: what it refuses leaves the context without a lens
        for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (16.5, 0, 0), (0, -17, 0), (0, 0, 16.001)):
            assert lib.mvs_set_lens(h, k3(*bad), W / 2.0, H / 2.0) == EINVAL, bad
        for centre in ((np.nan, 1.0), (1.0, np.inf)):
            assert lib.mvs_set_lens(h, k3(0, 0, 0), *centre) == EINVAL
        assert lib.mvs_set_lens(h, k3(-1.5, 0, 0), W / 2.0, H / 2.0) == EINVAL          # folds over inside the frame
        assert "folds over" in lib.mvs_last_error(h).decode()
        assert lens_mirror.folds_over(W, H, (-1.5, 0, 0)) and not lens_mirror.folds_over(W, H, (16, 16, 16))
        assert lib.mvs_lens(h, None, None, None) == 0
        # without a lens: MVS_ESTATE from everything that needs one, nothing written
        ctx.frame_store(2)
        assert lib.mvs_undistort(h, mvs_amd._ptr(frame, u8p), mvs_amd._ptr(out, u8p)) == ESTATE
        assert lib.mvs_undistort_device(h, dev.data_ptr(), dev.data_ptr() + P, 1) == ESTATE
        assert lib.mvs_undistort_map(h, mvs_amd._ptr(fmap, fp)) == ESTATE
        assert lib.mvs_frame_upload_lens(h, 0, frame.ctypes.data) == ESTATE
        assert lib.mvs_frame_upload_lens_device(h, 0, dev.data_ptr()) == ESTATE
        with pytest.raises(mvs_amd.MvsError):
            ctx.sweep_handles(0, synth.camera_at([0, 0, 0], W, H), [], np.zeros((0, 4, 4), np.float32), 16)   # slot 0 was not filled
        # the largest accepted coefficients are a lens; a refused call leaves the lens that was set
        assert lib.mvs_set_lens(h, k3(16, 16, 16), W / 2.0, H / 2.0) == 0
        assert lib.mvs_set_lens(h, k3(np.nan, 0, 0), W / 2.0, H / 2.0) == EINVAL
        np.testing.assert_array_equal(ctx.lens()[0], [16, 16, 16])
        # NULL arguments
        assert lib.mvs_undistort(h, None, mvs_amd._ptr(out, u8p)) == EINVAL
        assert lib.mvs_undistort(h, mvs_amd._ptr(frame, u8p), None) == EINVAL
        assert lib.mvs_undistort_device(h, None, dev.data_ptr(), 1) == EINVAL
        assert lib.mvs_undistort_device(h, dev.data_ptr(), None, 1) == EINVAL
        assert lib.mvs_undistort_map(h, None) == EINVAL
        assert lib.mvs_frame_upload_lens(h, 0, None) == EINVAL
        assert lib.mvs_frame_upload_lens_device(h, 0, None) == EINVAL
        # slots outside the store
        for slot in (-1, 2):
            assert lib.mvs_frame_upload_lens(h, slot, frame.ctypes.data) == EINVAL
            assert lib.mvs_frame_upload_lens_device(h, slot, dev.data_ptr()) == EINVAL
        ctx.synchronize()
        assert (out == 5).all() and (fmap == 5).all() and not dev.cpu().numpy().any()
    with mvs_amd.Context(W, H) as ctx:                                    # an unsized store has no slots
        ctx.set_lens((0.0, 0.0, 0.0))
        assert ctx.lib.mvs_frame_upload_lens(ctx.h, 0, frame.ctypes.data) == EINVAL
        assert ctx.lib.mvs_frame_upload_lens_device(ctx.h, 0, dev.data_ptr()) == EINVAL


def test_lens_launches_are_timed_as_projection():
    W, H = SMALL
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(lens_scenes.lenses(W, H)["zatisi"][0])
        ctx.profile_enable(True)
        ctx.undistort(lens_scenes.noise(W, H))
        ctx.undistort_map()
        ms, launches = ctx.profile_read()
        assert launches[mvs_amd.MVS_K_PROJECT] == 2 and sum(launches) == 2


def test_configuration_undistort_through_the_selftest(tmp_path, oracle):
    """Configuration --undistort: host_selftest's frames mode with the option, on the clip the frames-mode test decodes, equals the mirror
    applied to the frames the mode writes without the option (zatisi's lens, its centre from the file)"""
    import tracks_yaml
    import y4m_common
    y4m_common.run(tmp_path, oracle, scale=1)                       # writes the clip, runs the mode without the option, checks its frames
    t = tracks_yaml.load("zatisi.yaml")
    W, H = t["width"], t["height"]
    und = tmp_path / "undistorted"
    und.mkdir()
    r = subprocess.run([y4m_common.SELFTEST, "frames", str(tmp_path / "zatisi.yaml"), str(und), "3", "undistort"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = 0
    for name in sorted(os.listdir(tmp_path)):
        if not name.startswith("gray_"):
            continue
        plain = np.fromfile(tmp_path / name, np.uint8).reshape(H, W)
        got = np.fromfile(und / name, np.uint8).reshape(H, W)
        np.testing.assert_array_equal(got, lens_mirror.undistort(plain, t["distortion"], (t["center_x"], t["center_y"])), err_msg=name)
        assert (got != plain).any()
        seen += 1
    assert seen == 8
    # a tracks file without (two) coefficients: the option fails, with estimateExposure's words for the same lack
    text = open(tmp_path / "zatisi.yaml").read()
    import re
    bare = re.sub(r"distortion: \[[^\]]*\]", "distortion: [0.1]", text)
    assert bare != text
    (tmp_path / "bare.yaml").write_text(bare)
    r = subprocess.run([y4m_common.SELFTEST, "frames", str(tmp_path / "bare.yaml"), str(und), "3", "undistort"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "the tracks file gives no lens distortion" in r.stdout + r.stderr, r.stdout + r.stderr
