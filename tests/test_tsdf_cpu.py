"""TSDF fusion without a GPU: the new entry points' argument checks through the library, and the contract's float32 restatement
(tests/tsdf_mirror.py) on exact depth maps of synth.Scene's height field and on the properties the contract promises."""
import ctypes as C

import numpy as np
import pytest

import mvs_amd
import tsdf_mirror as tm
from mvs_amd import synth

mo = tm.mo

W, H = 320, 240
RING = 0.15
G = 64
SIDE = 3.4                                  # the cube: x, y in [-1.7, 1.7], z in [-4.7, -1.3] around the height field (z in [-3.4, -2.6])
ORIGIN = np.array([-1.7, -1.7, -4.7], np.float32)
HS = np.float32(SIDE / (G - 1))


def _centres():
    return [(0.0, 0.0, 0.0)] + [(RING * np.cos(a), RING * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(4) / 4]


@pytest.fixture(scope="module")
def ring():
    """the five axis-parallel cameras of tests/test_fuse_cpu.py: w-maps of the exact NDC depth maps, and the slot matrices in f32"""
    sc = synth.Scene()
    maps, mats = {}, {}
    for s, c in enumerate(_centres()):
        cam = synth.camera_at(c, W, H)
        P, Pi, Cc = tm.fm.slot_matrices(cam)
        mats[s] = (P.astype(np.float32), Pi.astype(np.float32), Cc.astype(np.float32))
        maps[s] = tm.wmap(sc.render(c, W, H, want_depth=True)[1], None, mats[s])
    return maps, mats


def _volume():
    return tm.Volume(G, ORIGIN, HS, 4 * HS)


def test_entry_points_refuse_a_null_context():
    lib = mvs_amd.load_library()
    assert mvs_amd.MVS_K_TSDF == 7
    o = np.zeros(3, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    slots = np.zeros(1, np.int32)
    s = C.c_void_p()
    assert lib.mvs_tsdf_volume(None, 64, fp(o), 0.1, 0.4) == -1
    assert lib.mvs_tsdf_integrate(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), float("inf")) == -1
    assert lib.mvs_tsdf_fetch(None, None, None) == -1
    assert lib.mvs_tsdf_surface(None, 1, C.byref(s)) == -1
    assert not s.value


def test_mirror_meshes_exact_maps_onto_the_height_field(ring):
    """G = 64 over the five ring maps at 320 x 240 (h = 0.054, about 6 pixels at w = 3; truncation 4 h).  Measured: median distance 0.0070 h,
    99th percentile 0.022 h, every face toward the centre camera"""
    maps, mats = ring
    vol = _volume().integrate(maps, mats, range(5))
    v, f = vol.surface(1)
    assert len(v) > 1000 and len(f) > 2000
    d = np.abs(v[:, 2].astype(np.float64) - synth.Scene.height(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64))) / float(HS)
    med, p99 = float(np.median(d)), float(np.percentile(d, 99))
    print("exact maps, mirror: %d vertices, %d faces; distance to the height field: median %.4f h, 99th percentile %.4f h" % (len(v), len(f), med, p99))
    assert med <= 0.1 and p99 <= 0.5
    p = v[:, :3].astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    n = np.cross(b - a, c - a)
    toward = -(a + b + c) / 3.0                # the centre camera sits at the origin
    facing = (n * toward).sum(1) > 0
    print("faces toward the centre camera: %.5f" % facing.mean())
    assert facing.mean() >= 0.99


def test_mirror_split_lists_equal_one_list(ring):
    maps, mats = ring
    one = _volume().integrate(maps, mats, [1, 3])
    two = _volume().integrate(maps, mats, [1]).integrate(maps, mats, [3])
    assert one.sum.tobytes() == two.sum.tobytes() and np.array_equal(one.count, two.count)
    assert one.count.max() == 2


def test_mirror_ignores_a_camera_facing_away_and_an_empty_map(ring):
    maps, mats = ring
    base = _volume().integrate(maps, mats, range(5))
    flip = np.diag([-1.0, 1.0, -1.0])          # a half turn about y: the camera looks up +z, away from the surface
    cam = synth.camera_at((0.0, 0.0, 0.0), W, H, rot=flip)
    P, Pi, Cc = tm.fm.slot_matrices(cam)
    extra_mats = dict(mats)
    extra_mats[5] = (P.astype(np.float32), Pi.astype(np.float32), Cc.astype(np.float32))
    d = synth.Scene().render((0.0, 0.0, 0.0), W, H, want_depth=True)[1]   # valid depths: in front of this camera they lie above it
    extra = dict(maps)
    extra[5] = tm.wmap(d, None, extra_mats[5])
    extra[6] = tm.wmap(np.ones((H, W), np.float32), None, mats[0])        # the empty value everywhere
    extra_mats[6] = mats[0]
    assert np.isfinite(extra[5]).mean() > 0.99 and not np.isfinite(extra[6]).any()
    got = _volume().integrate(extra, extra_mats, [0, 1, 5, 2, 6, 3, 4])
    assert got.sum.tobytes() == base.sum.tobytes() and np.array_equal(got.count, base.count)


def test_mirror_counts_a_slot_listed_twice_twice(ring):
    maps, mats = ring
    once = _volume().integrate(maps, mats, [2])
    twice = _volume().integrate(maps, mats, [2, 2])
    assert np.array_equal(twice.count, 2 * once.count) and once.count.max() == 1
    seen = once.count > 0
    assert np.array_equal(twice.sum[seen], (once.sum + once.sum)[seen])
    F1, m1 = once.field(1)
    F2, m2 = twice.field(2)
    assert np.array_equal(m1, m2) and np.array_equal(F1, F2)    # (x + x) / 2 = x exactly
    assert mo.surface_nets(F1, np.float32(0.0), ORIGIN, HS, m1)[1].shape == twice.surface(2)[1].shape
