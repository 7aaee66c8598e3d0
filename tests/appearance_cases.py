"""Inputs shared by tests/test_appearance_cpu.py (which checks each case's premise with the mirror) and tests/test_appearance_gpu.py (which
compares the kernels with the mirror bit for bit): the depth and frame stores of tests/test_tsdf_gpu.py's kind, the pair lists, the crafted
appearance cells with their points and depth maps, and the exact-map accuracy setup of DESIGN.md section 15.
"""
import functools

import numpy as np

import appearance_mirror as am
from mvs_amd import synth

f32 = np.float32
u32 = np.uint32
RING = 0.15


def ring_centres():
    return [(0.0, 0.0, 0.0)] + [(RING * np.cos(a), RING * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(4) / 4]


def cube(G, side=3.4, low=(-1.7, -1.7, -4.7)):
    """tests/test_tsdf_gpu.py's cube around the height field: (origin, node spacing)"""
    return np.asarray(low, f32), f32(side / (G - 1))


# ---- stores ------------------------------------------------------------------------------------------------------------------------
# depth slots 0-4: the ring's exact maps; 5: a camera facing away; 6: an empty map; 7: ring camera 1 with NaN and 1.0 holes; 8: ring camera 2
# again (tests/test_tsdf_gpu.py's store160).  The frame store has another capacity, and depth slot s goes with frame slot FRAME_OF[s]: not
# the identity, so a frame taken from the depth slot's index is another camera's (or an unfilled slot).  Frame slot EXTRA_FRAME holds a
# second, different image that is paired with depth slot 0 where PAIRS lists that slot again; frame slots 6 and 8 stay unfilled.
DEPTH_CAP, FRAME_CAP = 9, 12
FRAME_OF = [7, 2, 9, 0, 5, 11, 4, 1, 3]
EXTRA_FRAME = 10
UNFILLED_FRAME = 6
_DEPTH_LIST = [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 7, 2, 3, 1, 0, 8]   # 19 entries: two launch chunks
PAIRS = [(s, EXTRA_FRAME if e == 8 else FRAME_OF[s]) for e, s in enumerate(_DEPTH_LIST)]
LENGTHS = [1, 8, 9, 16, 17, 19]             # one batch less, one batch, one more; one chunk, one more; two chunks
PAIRS_COST = [(8, FRAME_OF[8]), (0, EXTRA_FRAME), (4, FRAME_OF[4])]       # under a finite max_cost
MAX_COST = 0.5
SIZES = [(61, 47), (160, 120)]
GRIDS = [16, 50, 65]                        # 65: one lane in the second 64-block; 50: a ragged last block of rows


@functools.lru_cache(maxsize=None)
def store(W, H):
    """-> dict: cams [9], depths [9], costs [9] (uniform in [0, 1)), frames {frame slot: [H, W] u8}"""
    sc = synth.Scene(freq_scale=W / 1920.0)
    rng = np.random.Generator(np.random.PCG64(0xA99E + W))
    cams, depths, images = [], [], []
    for c in ring_centres():
        img, d = sc.render(c, W, H, want_depth=True)
        cams.append(synth.camera_at(c, W, H))
        depths.append(d)
        images.append(img)
    cams.append(synth.camera_at((0.0, 0.0, 0.0), W, H, rot=np.diag([-1.0, 1.0, -1.0])))
    depths.append(depths[0].copy())
    images.append(rng.integers(0, 256, (H, W), dtype=np.uint8))
    cams.append(cams[0])
    depths.append(np.ones((H, W), f32))
    images.append(rng.integers(0, 256, (H, W), dtype=np.uint8))
    holes = depths[1].copy()
    pick = rng.random((H, W))
    holes[pick < 0.1] = np.nan
    holes[(pick >= 0.1) & (pick < 0.2)] = 1.0
    cams.append(cams[1])
    depths.append(holes)
    images.append(images[1])
    cams.append(cams[2])
    depths.append(depths[2].copy())
    images.append(images[2])
    costs = [rng.random((H, W)).astype(f32) for _ in depths]
    frames = {FRAME_OF[s]: images[s] for s in range(DEPTH_CAP)}
    frames[EXTRA_FRAME] = (255 - images[0]).astype(np.uint8)
    for a in depths + costs + list(frames.values()):
        a.setflags(write=False)
    return {"cams": cams, "depths": depths, "costs": costs, "frames": frames}


def mirror_snapshots(st, mats, G):
    """the mirror's volume after each prefix of PAIRS in LENGTHS (a split list gives the same bytes: tests/test_appearance_cpu.py), and after
    PAIRS_COST on top of the whole list -> ({n: (sum, count, cells)}, the final am.Volume)"""
    origin, h = cube(G)
    vol = am.Volume(G, origin, h, 4 * h)
    maps = {s: am.tm.wmap(st["depths"][s], None, mats[s]) for s in range(DEPTH_CAP)}
    snaps, done = {}, 0
    for n in LENGTHS:
        vol.integrate_frames(maps, mats, st["frames"], PAIRS[done:n])
        done = n
        snaps[n] = (vol.sum.copy(), vol.count.copy(), vol.cells.copy())
    maps_c = {s: am.tm.wmap(st["depths"][s], st["costs"][s], mats[s], MAX_COST) for s, _ in PAIRS_COST}
    vol.integrate_frames(maps_c, mats, st["frames"], PAIRS_COST)
    return snaps, vol


# ---- crafted cells -------------------------------------------------------------------------------------------------------------------
# The box is [1, 3]^3: origin (1, 1, 1), G = 17, h = 1/8, so node coordinates, x - o and g = (x - o) 8 are exact for the points below, and
# the float next to a face on the outside also has its g outside (next to -1 or 0 it would round back onto the face).
CG = 17
CORIGIN = np.array([1.0, 1.0, 1.0], f32)
CH = f32(0.125)
LO, HI = f32(1.0), f32(3.0)


def pack(count, total):
    return (np.asarray(count, np.int64) << 24 | np.asarray(total, np.int64)).astype(u32)


def crafted_volume(cells):
    vol = am.Volume(CG, CORIGIN, CH, 4 * CH)
    vol.cells = np.ascontiguousarray(cells, u32)
    return vol


def cells_single():
    """one node with a vote: (i, j, k) = (5, 6, 7) holds 3 votes summing to 301"""
    c = np.zeros((CG,) * 3, u32)
    c[7, 6, 5] = pack(3, 301)
    return c


def cells_random():
    """every node present: counts 1..255, sums up to 255 per vote"""
    rng = np.random.Generator(np.random.PCG64(0xCE11))
    n = rng.integers(1, 256, (CG,) * 3)
    n[rng.random(n.shape) < 0.05] = 255
    return pack(n, (n * rng.random(n.shape) * 255).astype(np.int64))


def cells_sparse():
    """two nodes in three without a vote: most cells have absent corners, many have none present"""
    c = cells_random()
    rng = np.random.Generator(np.random.PCG64(0x5BA5))
    c[rng.random(c.shape) < 0.67] = 0
    return c


def cells_constant(count, total):
    return np.full((CG,) * 3, pack(count, total), u32)


def node(i, j, k):
    return [1.0 + 0.125 * i, 1.0 + 0.125 * j, 1.0 + 0.125 * k]


def _up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def _down(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def point_sets():
    """name -> (cells, points [N, 4] f32, expected: 'all', 'none' or None (mixed: the mirror decides; both outcomes must occur))"""
    rng = np.random.Generator(np.random.PCG64(0x9017))
    inside = lambda n: np.concatenate([1.0 + 2.0 * rng.random((n, 3)), np.ones((n, 1))], 1)   # noqa: E731
    sets = {}
    # a single present corner: points inside the 8 cells that share the node see only it; its own value whatever the weight
    near = np.array(node(5, 6, 7)) + 0.125 * (rng.random((64, 3)) * 1.9 - 0.95)
    sets["single_corner"] = (cells_single(), np.concatenate([near, np.ones((64, 1))], 1), "all")
    sets["no_corner"] = (cells_single(), np.array([node(10, 10, 10) + [1.0], [2.3, 1.1, 2.9, 1.0], node(5, 6, 9) + [1.0]]), "none")
    # the present corner has weight 0: points on the far faces of the cells around the node (fraction 0 toward it)
    zero_w = [node(4, 6, 7), node(5, 5, 7), node(5, 6, 6), [1.5, 1.0 + 0.125 * 6.5, 1.0 + 0.125 * 7.5], node(6, 6, 7), node(5, 7, 8)]
    sets["weight_zero"] = (cells_single(), np.concatenate([np.array(zero_w), np.ones((6, 1))], 1), "none")
    # on the box's upper faces: cell G - 2, fraction 1; and the corners and lower faces of the box
    faces = [[3.0, 1.7, 2.2], [1.3, 3.0, 2.9], [2.6, 1.01, 3.0], [3.0, 3.0, 3.0], [1.0, 1.0, 1.0], [1.0, 3.0, 2.0], [3.0, 2.0, 1.0]]
    sets["upper_faces"] = (cells_random(), np.concatenate([np.array(faces), np.ones((7, 1))], 1), "all")
    out = []
    for a in range(3):
        for x in (_up(3.0), _down(1.0), 3.5, 0.0, -7.0, np.inf, -np.inf, np.nan):
            p = [2.0, 2.0, 2.0]
            p[a] = x
            out.append(p)
    sets["one_ulp_outside"] = (cells_random(), np.concatenate([np.array(out), np.ones((len(out), 1))], 1), "none")
    # w != 1 and w = 0: rows (x w, y w, z w, w)
    base = inside(200)
    w = np.concatenate([rng.choice([0.5, 2.0, -1.0, 3.7, 1e-3, 1e4], 180), np.zeros(20)])
    sets["homogeneous"] = (cells_random(), np.concatenate([base[:, :3] * w[:, None], w[:, None]], 1), None)
    sets["zero_w_rows"] = (cells_random(), np.concatenate([base[:20, :3], np.zeros((20, 1))], 1), "none")
    sets["sparse"] = (cells_sparse(), inside(3000), None)
    # 300 points and no multiple of the block
    sets["rounding"] = (cells_constant(2, 509), inside(300), "all")
    return {k: (c, np.ascontiguousarray(p, f32), e) for k, (c, p, e) in sets.items()}


CRAFT_W, CRAFT_H = 61, 47


def crafted_camera(flip_sign=False):
    """looks down -z at the box from (2, 2, 6): the box spans w = 3 .. 5.  flip_sign: the same projection with every entry negated, so
    (P (X, 1)).w < 0 at every point the camera sees"""
    cam = synth.camera_at((2.0, 2.0, 6.0), CRAFT_W, CRAFT_H)
    return (-cam).astype(f32) if flip_sign else cam


def plane_depth(cam, w):
    """NDC z of synth's cameras at linear depth w (synth.Scene.render's formula)"""
    near, far = synth.NEAR, synth.FAR
    return f32((far + near) / (far - near) + (2.0 * far * near / (near - far)) / w)


def depth_maps():
    """name -> (cells, camera, depth [H, W] f32, least shaded pixels, least unshaded pixels)"""
    W, H = CRAFT_W, CRAFT_H
    cam = crafted_camera()
    rng = np.random.Generator(np.random.PCG64(0xDE97))
    # a slanted sheet through the box, wider than the box (the frustum at w = 4 is 3.7 wide): inside it in the middle, outside at the sides
    slant = np.array([[plane_depth(cam, 3.2 + 1.6 * c / (W - 1)) for c in range(W)]] * H, f32)
    holes = slant.copy()
    pick = rng.random((H, W))
    holes[pick < 0.1] = np.nan
    holes[(pick >= 0.1) & (pick < 0.2)] = 1.0
    holes[(pick >= 0.2) & (pick < 0.25)] = -1.0
    holes[(pick >= 0.25) & (pick < 0.3)] = np.inf
    flat = np.full((H, W), plane_depth(cam, 4.0), f32)
    return {
        "random_slant": (cells_random(), cam, slant, 400, 400),
        "random_holes": (cells_random(), cam, holes, 300, 800),
        "sparse_slant": (cells_sparse(), cam, slant, 200, 600),
        "single_flat": (cells_single(), cam, np.full((H, W), plane_depth(cam, 4.1), f32), 4, 2500),   # z = 1.9: in the node's layer of cells
        "w_not_positive": (cells_random(), crafted_camera(True), flat, 0, W * H),
        "value_254_5": (cells_constant(2, 509), cam, slant, 400, 400),
        "value_255": (cells_constant(1, 255), cam, slant, 400, 400),
        "clamp_above_255": (cells_constant(1, 300), cam, slant, 400, 400),
        "behind_the_box": (cells_random(), cam, np.full((H, W), plane_depth(cam, 5.5), f32), 0, W * H),
    }


# ---- accuracy: DESIGN.md section 15 ----------------------------------------------------------------------------------------------------
ACC_W, ACC_H, ACC_G = 160, 120, 64


def accuracy_inputs():
    """five exact ring maps at 160 x 120 with their frames (texture wavelengths fixed in pixels) -> (cams, depths, frames)"""
    sc = synth.Scene(freq_scale=ACC_W / 1920.0)
    cams, depths, frames = [], [], []
    for c in ring_centres():
        img, d = sc.render(c, ACC_W, ACC_H, want_depth=True)
        cams.append(synth.camera_at(c, ACC_W, ACC_H))
        depths.append(d)
        frames.append(img)
    return cams, depths, frames


def accuracy_figures(ray_depth, shaded, frame):
    """(shaded / hit, median, 99th percentile and maximum of |shaded - frame| over the shaded pixels)"""
    hit = ray_depth < 1.0
    have = shaded[..., 1] == 255
    assert not (have & ~hit).any()
    d = np.abs(shaded[..., 0][have].astype(np.int64) - frame[have].astype(np.int64))
    return {"hit": int(hit.sum()), "shaded_of_hit": float(have.sum() / hit.sum()), "median": float(np.median(d)), "p99": float(np.percentile(d, 99)),
            "max": int(d.max())}


def assert_accuracy_figures(f):
    assert f["hit"] > 0.5 * ACC_W * ACC_H, f
    assert f["shaded_of_hit"] >= 0.999, f
    assert f["median"] <= 2 and f["p99"] <= 8 and f["max"] <= 16, f
