"""Crafted TSDF volumes and cameras for the ray-cast tests (tests/test_raycast_cpu.py checks each case's premise with the mirror,
tests/test_raycast_gpu.py uploads the same fields with mvs_tsdf_upload and compares the kernel with the mirror bit for bit).

The box is [-1, 1]^2 x [-4, -2]: origin (-1, -1, -4), h = 2 / (G - 1).  A volume is (sum [G, G, G] f32, count [G, G, G] i32), [k][j][i].
CASES lists (name, volume, G, (W, H), camera, step, min_observations, least hits, least empty pixels): the two counts are the case's premise,
so that no comparison can pass on an all-empty (or all-hit) map by accident.
"""
import numpy as np

import tsdf_mirror as tm
from mvs_amd import synth

f32 = np.float32
ORIGIN = np.array([-1.0, -1.0, -4.0], f32)
CENTRE = np.array([0.0, 0.0, -3.0])
R = 0.6


def spacing(G):
    return f32(2.0 / (G - 1))


def nodes(G):
    """float64 node coordinates (x, y, z), each [G, G, G] in [k][j][i] order"""
    t = np.arange(G) * float(spacing(G))
    z, y, x = np.meshgrid(ORIGIN[2] + t, ORIGIN[1] + t, ORIGIN[0] + t, indexing="ij")
    return x, y, z


def _pack(F, count=None):
    F = np.asarray(F, f32)
    c = np.ones(F.shape, np.int32) if count is None else np.asarray(count, np.int32)
    return (F * c.astype(f32)).astype(f32), c


def _radius(G):
    x, y, z = nodes(G)
    return np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2)


def sphere(G):
    """a solid ball of radius 0.6 about (0, 0, -3), truncation 4 h"""
    return _pack(np.clip((_radius(G) - R) / (4 * float(spacing(G))), -1, 1))


def shell(G):
    """solid between radii 0.45 and 0.75 (a cavity inside): front and back faces along every ray through it"""
    return _pack(np.clip((np.abs(_radius(G) - R) - 0.15) / (4 * float(spacing(G))), -1, 1))


def holes(G):
    """the ball with a slab of unobserved nodes (count 0) through its surface, two nodes thick, at x about 0.2"""
    s, c = sphere(G)
    i0 = int(round(1.2 / float(spacing(G))))
    c[:, :, i0:i0 + 2] = 0
    return s, c


def random_counts(G):
    """the ball with counts 1..5 drawn per node (one node in ten below 3): min_observations = 3 leaves a ragged support, about 0.9^8 = 43 %
    of the cells"""
    rng = np.random.Generator(np.random.PCG64(0x7A7C + G))
    F = np.clip((_radius(G) - R) / (4 * float(spacing(G))), -1, 1)
    return _pack(F, rng.choice([1, 2, 3, 4, 5], F.shape, p=[0.05, 0.05, 0.3, 0.3, 0.3]))


def last_cells(G):
    """a block whose three faces toward +x, +y and +z lie half a spacing inside the box's upper faces: every crossing through them is in cell
    G - 2 of that axis"""
    h = float(spacing(G))
    x, y, z = nodes(G)
    F = np.maximum(np.maximum(x - (1.0 - 0.5 * h), y - (1.0 - 0.5 * h)), z - (-2.0 - 0.5 * h)) / (4 * h)
    return _pack(np.clip(F, -1, 1))


TINY = f32(2.0 ** -30)


def tiny_positives(G):
    """free space (F = 1) over a solid floor (F = -1 at j <= 7) in the bricks below; on the box's upper y face the nodes at k below the middle hold
    2^-30 and the others 0.5.  A sample ON that face (fraction f_y = 1 exactly) interpolates 1 + 1 (2^-30 - 1) = 0 <= 0 with no corner <= 0:
    the camera "graze" (centre ON the face's plane, y = 1) sends its middle pixel row along the face, |d_y| about 1e-8 (G = 17: h = 1/8 and
    every coordinate involved is exact).  Those of its 67 rays that are still inside the box at z = -3, where the 2^-30 begin (|x| <= 1 there:
    about 48), hit"""
    F = np.ones((G, G, G), f32)
    F[:, :8, :] = -1.0
    F[:, G - 1, :] = 0.5
    F[:G // 2, G - 1, :] = TINY
    return _pack(F)


VOLUMES = {"sphere": sphere, "shell": shell, "holes": holes, "random": random_counts, "last": last_cells, "tiny": tiny_positives}

_c, _s = np.cos(np.pi / 4), np.sin(np.pi / 4)
HALF_TURN = np.diag([-1.0, 1.0, -1.0])                       # about y: the camera looks up +z
YAW45 = np.array([[_c, 0, -_s], [0, 1, 0], [_s, 0, _c]])    # looks along (-sin 45, 0, -cos 45)
DOWN = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])   # looks along -y
ROLL_HALF = np.diag([-1.0, -1.0, 1.0])                      # about z: looks down -z, upside down

# name -> (centre, world-to-camera rotation or None, near)
CAMERAS = {
    "front": ((0.0, 0.0, 0.0), None, synth.NEAR),
    "far_side": ((0.0, 0.0, -6.0), HALF_TURN, synth.NEAR),
    "oblique": ((1.8, 0.4, -1.2), YAW45, 0.5),
    "above": ((0.0, 3.2, -3.0), DOWN, synth.NEAR),
    "in_box": ((0.0, 0.0, -2.2), None, 0.05),
    "in_box_default_near": ((0.0, 0.0, -2.2), None, synth.NEAR),   # hits, but all in front of the near plane: empty by rule 5
    "in_cavity": ((0.0, 0.0, -3.0), None, 0.05),
    "in_solid": ((0.0, 0.0, -3.0), None, 0.05),
    "away": ((0.0, 0.0, 0.0), HALF_TURN, synth.NEAR),
    "misses": ((0.0, 2.5, 0.0), None, synth.NEAR),
    "graze": ((0.0, 1.0, 0.0), None, synth.NEAR),
    "graze_flipped": ((0.0, 1.0, 0.0), ROLL_HALF, synth.NEAR),
}


def camera(name, W, H):
    c, rot, near = CAMERAS[name]
    return synth.camera_at(c, W, H, near=near, rot=rot)


def volume(name, G):
    """tsdf_mirror.Volume holding the crafted fields (truncation 4 h, as the fields assume)"""
    h = spacing(G)
    vol = tm.Volume(G, ORIGIN, h, 4 * h)
    vol.sum, vol.count = VOLUMES[name](G)
    return vol


# (name, volume, G, (W, H), camera, step, min_observations, least hits, least empty).  Pixels: 67 x 45 = 3015, 64 x 48 = 3072, 130 x 9 = 1170.
# Where the issue's table gives a count the bounds bracket it loosely; elsewhere they follow from the geometry: the ball's silhouette from
# the origin has angular radius asin(0.2) = 11.5 deg against a half field of view of 24.7 deg by 17.1 deg.
CASES = [
    ("sphere_front_16", "sphere", 16, (67, 45), "front", 0.5, 1, 600, 2200),
    ("sphere_front_17", "sphere", 17, (64, 48), "front", 0.25, 1, 600, 2200),
    ("sphere_front_25", "sphere", 25, (67, 45), "front", 1.0, 1, 600, 2200),
    ("sphere_front_50", "sphere", 50, (67, 45), "front", 1.7, 1, 600, 2200),
    ("sphere_strip_50", "sphere", 50, (130, 9), "front", 0.5, 1, 400, 500),
    ("sphere_far_side", "sphere", 25, (67, 45), "far_side", 0.5, 1, 600, 2200),
    ("sphere_oblique", "sphere", 17, (67, 45), "oblique", 0.5, 1, 700, 1900),
    ("shell_front", "shell", 25, (67, 45), "front", 0.5, 1, 900, 1800),
    ("shell_oblique", "shell", 50, (64, 48), "oblique", 0.25, 1, 900, 1500),
    ("shell_cavity", "shell", 25, (67, 45), "in_cavity", 0.5, 1, 3015, 0),
    ("sphere_in_box", "sphere", 16, (67, 45), "in_box", 0.5, 1, 2500, 0),
    ("sphere_in_box_near", "sphere", 16, (67, 45), "in_box_default_near", 0.5, 1, 0, 3015),
    ("sphere_in_solid", "sphere", 25, (67, 45), "in_solid", 0.5, 1, 0, 3015),
    ("sphere_away", "sphere", 17, (67, 45), "away", 0.5, 1, 0, 3015),
    ("sphere_misses", "sphere", 17, (130, 9), "misses", 1.0, 1, 0, 1170),
    ("holes_front", "holes", 25, (67, 45), "front", 0.5, 1, 400, 2200),
    ("holes_oblique", "holes", 50, (67, 45), "oblique", 1.0, 1, 400, 1900),
    ("random_min1", "random", 25, (67, 45), "front", 0.5, 1, 600, 2200),
    ("random_min3", "random", 25, (67, 45), "front", 0.5, 3, 100, 2200),
    ("random_min3_50", "random", 50, (64, 48), "oblique", 0.25, 3, 100, 1900),
    ("last_front", "last", 17, (67, 45), "front", 0.5, 1, 2500, 0),
    ("last_oblique", "last", 16, (67, 45), "oblique", 0.25, 1, 2500, 50),
    ("last_above", "last", 25, (64, 48), "above", 1.0, 1, 2500, 100),
    ("last_above_50", "last", 50, (130, 9), "above", 1.7, 1, 900, 20),
    ("tiny_graze", "tiny", 17, (67, 45), "graze", 0.5, 1, 40, 300),
    ("tiny_graze_flipped", "tiny", 17, (67, 45), "graze_flipped", 0.5, 1, 40, 300),
]


# ---- the exact-map setup of tests/test_tsdf_cpu.py: five ring cameras at 320 x 240, G = 64 over the height field, truncation 4 h ----
RING_W, RING_H, RING_G, RING_RADIUS = 320, 240, 64, 0.15
RING_ORIGIN = np.array([-1.7, -1.7, -4.7], f32)
RING_H_NODE = f32(3.4 / (RING_G - 1))


def ring_centres():
    return [(0.0, 0.0, 0.0)] + [(RING_RADIUS * np.cos(a), RING_RADIUS * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(4) / 4]


def exact_map_figures(depth, normals, cam, centre, exact_depth):
    """the figures of the exact-map table for one ray-cast map of the height field: hit share; the hit points'
    distance to the height field in node spacings (median, 99th percentile); |NDC z - the exact map| (median, 99th percentile, maximum);
    the normals' angle to the analytic ones in degrees (median, 99th percentile); the share of normals on the camera's side.
    Hit points are back-projected in float64."""
    H, W = depth.shape
    hit = depth < 1.0
    Pi = np.linalg.inv(np.asarray(cam, np.float64))
    rows, cols = np.nonzero(hit)
    q = Pi @ np.stack([(2.0 * cols + 1.0) / W - 1.0, 1.0 - (2.0 * rows + 1.0) / H, depth[hit].astype(np.float64), np.ones(len(rows))])
    X = (q[:3] / q[3]).T
    dist = np.abs(X[:, 2] - synth.Scene.height(X[:, 0], X[:, 1])) / float(RING_H_NODE)
    dz = np.abs(depth[hit].astype(np.float64) - exact_depth[hit].astype(np.float64))
    dhx = -0.52 * np.cos(1.3 * X[:, 0] + 0.7) * np.cos(1.1 * X[:, 1] - 0.2)
    dhy = 0.44 * np.sin(1.3 * X[:, 0] + 0.7) * np.sin(1.1 * X[:, 1] - 0.2)
    nr = np.stack([-dhx, -dhy, np.ones_like(dhx)], 1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    n = normals[hit].astype(np.float64)
    ang = np.degrees(np.arccos(np.clip((n * nr).sum(1), -1, 1)))
    facing = ((n * (np.asarray(centre, np.float64)[None, :] - X)).sum(1) > 0).mean()
    return {"hit": float(hit.mean()), "dist_med": float(np.median(dist)), "dist_p99": float(np.percentile(dist, 99)),
            "z_med": float(np.median(dz)), "z_p99": float(np.percentile(dz, 99)), "z_max": float(dz.max()),
            "ang_med": float(np.median(ang)), "ang_p99": float(np.percentile(ang, 99)), "facing": float(facing),
            "unit": float(np.abs(np.linalg.norm(n, axis=1) - 1.0).max())}


def assert_exact_map_figures(f):
    """the bounds of the exact-map table"""
    assert f["hit"] >= 0.95, f
    assert f["dist_med"] <= 0.1 and f["dist_p99"] <= 0.5, f
    assert f["z_med"] <= 4e-4 and f["z_p99"] <= 1.5e-3, f
    assert f["ang_med"] <= 1.5 and f["ang_p99"] <= 5.0, f
    assert f["facing"] >= 0.99, f
    assert f["unit"] <= 1e-6, f
