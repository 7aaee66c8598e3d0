"""Inputs shared by tests/test_fusion_cases_cpu.py (which checks each case's premise with the mirrors) and tests/test_fusion_cases_gpu.py
(which compares mvs_fuse_depth, mvs_tsdf_integrate, mvs_tsdf_integrate_frames, mvs_tsdf_shade and mvs_tsdf_surface with the mirrors bit for
bit): exact depth maps of a scene with a step and a ball for cameras of any orientation, the camera sets, the stores per image size, the
builders that put values ON the decisions of the contracts (DESIGN.md sections 11, 12 and 15), and the case tables with their premises.

The scene (world units, about z = -3 like synth.Scene's height field): a tilted back plane, a tilted rectangular occluder 0.6 in front of it
(the step), and a ball of radius 0.25 clear of both.  Depth maps are computed in float64 from the camera's 4 x 4 matrix alone and rounded to
float32 once; synth.Scene.render (axis-parallel cameras only) is not used.
"""
import functools

import numpy as np

import appearance_mirror as am
import fuse_mirror as fm
from mvs_amd import synth

f32 = np.float32


def up(x):
    return f32(np.nextafter(f32(x), f32(np.inf)))


def down(x):
    return f32(np.nextafter(f32(x), f32(-np.inf)))


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
class Plane:
    """n . X = d, optionally bounded by a predicate on the hit point"""

    def __init__(self, point, normal, inside=None):
        self.n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        self.d = float(self.n @ np.asarray(point, np.float64))
        self.inside = inside if inside is not None else (lambda X: np.ones(X[0].shape, bool))

    def hits(self, A, D):
        with np.errstate(all="ignore"):
            return [(self.d - np.einsum("i,i...->...", self.n, A)) / np.einsum("i,i...->...", self.n, D)]

    def distance(self, X):
        d = np.abs(np.einsum("i,i...->...", self.n, X) - self.d)
        return np.where(self.inside(X), d, np.inf)

    def normal(self, X):
        return np.broadcast_to(self.n.reshape((3,) + (1,) * (X.ndim - 1)), X.shape)


class Sphere:
    def __init__(self, centre, radius):
        self.c = np.asarray(centre, np.float64)
        self.r = float(radius)

    def inside(self, X):
        return np.ones(X[0].shape, bool)

    def hits(self, A, D):
        rel = A - self.c.reshape((3,) + (1,) * (A.ndim - 1))
        a = (D * D).sum(0)
        b = 2.0 * (D * rel).sum(0)
        c = (rel * rel).sum(0) - self.r ** 2
        with np.errstate(all="ignore"):
            root = np.sqrt(b * b - 4.0 * a * c)   # NaN: the ray misses
            return [(-b - root) / (2.0 * a), (-b + root) / (2.0 * a)]

    def distance(self, X):
        return np.abs(np.linalg.norm(X - self.c.reshape((3,) + (1,) * (X.ndim - 1)), axis=0) - self.r)

    def normal(self, X):
        n = X - self.c.reshape((3,) + (1,) * (X.ndim - 1))
        return n / np.linalg.norm(n, axis=0)


BACK = Plane((0.0, 0.0, -3.3), (0.25, -0.18, 1.0))
OCCLUDER = Plane((0.1, -0.05, -2.7), (-0.1, 0.05, 1.0), lambda X: (np.abs(X[0] - 0.1) < 0.35) & (np.abs(X[1] + 0.05) < 0.3))
BALL = Sphere((-0.55, 0.35, -2.8), 0.25)
SCENE = (BACK, OCCLUDER, BALL)
FLOOR = (Plane((0.0, 0.0, -4.03), (0.02, -0.01, 1.0)),)   # the pixel-rounding volume's scene: one unbounded plane


def exact_depth(cam, W, H, prims=SCENE):
    """NDC depth map [H, W] f32 of `cam` (any 4 x 4 projection): per pixel centre the ray through the back-projections of NDC depths -0.5 and
    0.5, its hits with every primitive, and of those with w > 0 and -1 < z < 1 the one nearest the camera (least w); 1.0 where there is none"""
    P = np.asarray(cam, np.float64).reshape(4, 4)
    Pi = np.linalg.inv(P)
    rows, cols = np.mgrid[0:H, 0:W]
    xn = (2.0 * cols + 1.0) / W - 1.0
    yn = 1.0 - (2.0 * rows + 1.0) / H

    def unproject(z):
        h = np.einsum("ij,j...->i...", Pi, np.stack([xn, yn, np.full(xn.shape, z), np.ones(xn.shape)]))
        return h[:3] / h[3]

    A = unproject(-0.5)
    D = unproject(0.5) - A
    best_w = np.full((H, W), np.inf)
    best_z = np.ones((H, W))
    with np.errstate(all="ignore"):
        for prim in prims:
            for s in prim.hits(A, D):
                X = A + s * D
                h = np.einsum("ij,j...->i...", P, np.concatenate([X, np.ones((1, H, W))]))
                w, z = h[3], h[2] / h[3]
                ok = np.isfinite(s) & (w > 0.0) & (z > -1.0) & (z < 1.0) & prim.inside(X) & (w < best_w)
                best_w = np.where(ok, w, best_w)
                best_z = np.where(ok, z, best_z)
    return best_z.astype(f32)


def scene_distance(X, prims=SCENE):
    """float64 distance of points X [3, ...] to the nearest primitive (a bounded plane counts where the point lies over its rectangle) and
    that primitive's unit normal there"""
    X = np.asarray(X, np.float64)
    d = np.stack([p.distance(X) for p in prims])
    which = d.argmin(0)
    n = np.zeros(X.shape)
    for i, p in enumerate(prims):
        n = np.where(which == i, p.normal(X), n)
    return d.min(0), n, which


# ---- cameras --------------------------------------------------------------------------------------------------------------------------
def rotation(yaw, pitch, roll):
    """world -> camera: a yaw about y, then a pitch about x, then a roll about the optical axis (degrees)"""
    a, b, c = np.radians([yaw, pitch, roll])
    Ry = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), np.sin(b)], [0, -np.sin(b), np.cos(b)]])
    Rz = np.array([[np.cos(c), np.sin(c), 0], [-np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


TARGET = np.array([0.0, 0.0, -3.0])


def looking(W, H, yaw, pitch, roll, dist=3.0, target=TARGET, mirror=False, **kw):
    """synth.camera_at of a camera `dist` away from `target`, looking at it"""
    R = rotation(yaw, pitch, roll)
    centre = np.asarray(target, np.float64) + dist * (R.T @ np.array([0.0, 0.0, 1.0]))   # the camera looks down its own -z
    if mirror:
        R = np.diag([-1.0, 1.0, 1.0]) @ R
    return synth.camera_at(centre, W, H, rot=R, **kw)


# the rotated set.  AXIS stays axis-parallel (the sparse matrices of the older suites, in the same calls); ROLLED has its rows x and y mixed by
# a 75 degree roll; WIDE another fovx; DEEP its own near / far (its NDC depth means something else than its neighbours'); SHIFTED its
# principal point off centre; MIRRORED a left-handed image (tc x tr already faces the camera: the normal's flip is NOT taken); CUT a near
# plane behind the occluder and through the ball, so it sees the ball's inner far side and the back plane through the occluder
AXIS, TILTED, ROLLED, WIDE, DEEP, SHIFTED, MIRRORED, CUT = range(8)
NCAM = 8
VOTING = (TILTED, ROLLED, WIDE, DEEP, SHIFTED)   # general cameras that see the whole scene: each must have every coefficient non-zero
CUT_NEAR = 2.75


def cameras(W, H):
    cams = [synth.camera_at((0.0, 0.0, 0.0), W, H),
            looking(W, H, 8.0, -5.0, 12.0),
            looking(W, H, -10.0, 6.0, 75.0),
            looking(W, H, 5.0, 9.0, -30.0, fovx=1.05),
            looking(W, H, -6.0, -8.0, 20.0, near=2.2, far=6.0),
            looking(W, H, 3.0, -3.0, -50.0),
            looking(W, H, 7.0, 4.0, 33.0, mirror=True),
            looking(W, H, 12.0, 4.0, -15.0, near=CUT_NEAR)]
    shifted = cams[SHIFTED].copy()
    shifted[0] += f32(0.07) * shifted[3]
    shifted[1] -= f32(0.05) * shifted[3]
    cams[SHIFTED] = shifted
    return [np.ascontiguousarray(c, f32) for c in cams]


# coefficients of rows x, y, w of P (12) and of P^-1 (14: a projective camera's P^-1[3][0] and P^-1[3][1] are zero by construction --
# the back-projection's w does not depend on the pixel -- and a shifted principal point changes the last column only)
P_COEFFS = [(r, c) for r in (0, 1, 3) for c in range(4)]
PI_COEFFS = [(r, c) for r in range(4) for c in range(4) if (r, c) not in ((3, 0), (3, 1))]


def mats32(cam):
    """(P, P^-1, centre) in float32 as the library derives them, up to the last bit of P^-1 (tests/fuse_mirror.py: slot_matrices)"""
    return tuple(np.asarray(m, f32) for m in fm.slot_matrices(cam))


# ---- sizes, lists -----------------------------------------------------------------------------------------------------------------------
SIZES = [(131, 67), (64, 4), (67, 45)]      # two 64-column tiles and three columns, sixteen 4-row tiles and three rows; one tile; odd
TSDF_SIZES = [(131, 67), (67, 45)]          # 8777 and 3015 pixels: neither a multiple of the w-map kernel's 256
GRIDS = [16, 50, 65]
LENGTHS = [1, 8, 9, 16, 17, 19]             # one batch less, one batch, one more; one chunk, one more; two chunks
# slots beyond the cameras': ROLLED and AXIS with seam holes, TILTED with depth-rule ties, WIDE seeing the back plane alone
HOLEY_ROLLED, TIES, HOLEY_AXIS, PLANE_ONLY = 8, 9, 10, 11
# and five cameras (all with synth's near / far) whose exact maps are moved along their rays by up to 2 % of the depth, a draw per pixel: the
# relative-depth test of their votes is then populated on both sides of max_rel_depth = 0.01 while the reference keeps its tangents
NOISY = [12, 13, 14, 15, 16]
NOISY_CAMS = [AXIS, TILTED, WIDE, SHIFTED, MIRRORED]
NOISE = 0.02
HALF = 17   # AXIS with its principal point half a pixel off both ways: AXIS' pixel centres land ON its pixel seams, up to the roundings
DEPTH_CAP, FRAME_CAP = 18, 19
CAM_OF = list(range(NCAM)) + [ROLLED, TILTED, AXIS, WIDE] + NOISY_CAMS + [AXIS]
FRAME_OF = [(7 * s + 3) % FRAME_CAP for s in range(DEPTH_CAP)]   # a permutation that is not the identity
TSDF_LIST = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2, 2, 0, 5, 1, 11, 3, 7]
TSDF_LIST_COST = [9, 1, 4, 8]               # on top, under max_cost = MAX_COST
TSDF_LIST_ZERO = [2, 9, 0]                  # on top of that, under max_cost = 0
MAX_COST = f32(0.5)
TINY = f32(np.nextafter(f32(0.0), f32(1.0)))   # the float next to 0: a denormal
# every cost map draws from these: ON max_cost = 0.5 and its two neighbours, ON max_cost = 0 (both zeros) and its two neighbours, and
# uniform values.  Under max_cost = 0.5 about 80 % of the pixels are valid, under max_cost = 0 about 40 %
COST_VALUES = [MAX_COST, up(MAX_COST), down(MAX_COST), f32(0.0), f32(-0.0), TINY, -TINY]
COST_SHARES = [0.1, 0.1, 0.1, 0.2, 0.1, 0.1, 0.1]
Z_TIES = [f32(-1.0), up(-1.0), down(1.0), f32(1.0), f32(np.nan), f32(np.inf), f32(-np.inf)]   # only the second and the third are valid


def cube(G, side=3.4, low=(-1.7, -1.7, -4.7)):
    """tests/test_tsdf_gpu.py's cube: (origin, node spacing); the scene lies between z = -3.6 and -2.5"""
    return np.asarray(low, f32), f32(side / (G - 1))


def punch_seams(depth):
    """holes (1.0 and NaN in turn) about the 64-column and 4-row tile seams of csrc/fuse.hip and in the image corners, so that every one-sided
    tangent variant (lower neighbour only, upper only, none) occurs across a tile border and at an image border; an isolated valid pixel;
    a 64-pixel segment and a whole row with nothing valid"""
    d = np.array(depth, f32)
    H, W = d.shape
    hole = np.zeros((H, W), bool)
    rows, cols = np.mgrid[0:H, 0:W]
    if H < 40:                                 # the one-tile image: the tile's border is the image's
        hole[0, :] = True                      # its one segment per row: a whole row (rows 1, 2, 3 then read: upper only, both, lower only)
        hole[2, [1, 10, 20, 22, 40]] = True    # (2, 0), (2, 21): no neighbour along the row; (2, 9) and (2, 11): one
        hole[1, [21, 30, 62]] = True           # (1, 63): none along the row at the last column
        hole[3, [0, 21, 30, 63]] = True        # (2, 21) is isolated; (2, 30) has no neighbour along the column
        d[hole & ((rows + cols) % 2 == 0)] = 1.0
        d[hole & ((rows + cols) % 2 == 1)] = np.nan
        return d
    for c0 in (62, 126):                       # columns c0 .. c0 + 3 straddle a seam between c0 + 1 and c0 + 2; 126 .. 130 end the image
        if c0 + 1 >= W:
            continue
        pattern = {0: [2], 1: [1], 2: [0, 1, 2, 3], 3: [1, 3]}   # per row % 8: which of the four columns are holes (rows 4 .. 7: none)
        for k, offs in pattern.items():
            for o in offs:
                if c0 + o < W:
                    hole[(rows % 8 == k) & (cols == c0 + o)] = True
    if W > 129:
        hole[(rows % 8 == 5) & (cols == 129)] = True   # beside the last column: column 130 has no neighbour on either side there
    for r0 in (2, 62):                         # rows r0 .. r0 + 3 straddle a seam between r0 + 1 and r0 + 2; 66 ends the 67-row image
        if r0 + 1 >= H:
            continue
        pattern = {0: [2], 1: [1], 2: [0, 1, 2, 3], 3: [1, 3]}   # per column % 8 (the other four keep the seam whole)
        for k, offs in pattern.items():
            for o in offs:
                if r0 + o < H:
                    hole[(cols % 8 == k) & (rows == r0 + o)] = True
    for r in (0, H - 1):                       # the corners themselves, and the pixels next to the far corners
        for c in (0, W - 1):
            hole[r, c] = True
    hole[0, 1] = hole[H - 1, W - 2] = True
    hole[18:23, 28:33] = True                  # an isolated valid pixel
    hole[20, 30] = False
    hole[10, 64:128] = True                    # a whole segment of the second tile column
    hole[30, :] = True                         # a whole row
    d[hole & ((rows + cols) % 2 == 0)] = 1.0
    d[hole & ((rows + cols) % 2 == 1)] = np.nan
    return d


def place_z_ties(depth):
    """3 x 3 blocks of each of Z_TIES: a block of valid values (the floats next to -1 and 1 on the inside) is its own surface, far from its
    surroundings, and keeps its tangents; a block of the others is a hole"""
    d = np.array(depth, f32)
    H, W = d.shape
    for r0 in (0, H // 2) if H >= 16 else (0,):
        for b, z in enumerate(Z_TIES):
            d[r0:r0 + 3, 4 + 8 * b:7 + 8 * b] = z
    return d


@functools.lru_cache(maxsize=None)
def store(W, H):
    """-> dict: cams [DEPTH_CAP], depths, costs, frames {frame slot: [H, W] u8} (read-only arrays)"""
    rng = np.random.Generator(np.random.PCG64(0xFC5E + 1000 * W + H))
    base = cameras(W, H)
    cams = [base[CAM_OF[s]] for s in range(DEPTH_CAP)]
    half = cams[HALF].copy()
    half[0] += f32(1.0 / W) * half[3]
    half[1] -= f32(1.0 / H) * half[3]
    cams[HALF] = half
    depths = [exact_depth(c, W, H) for c in base]
    depths.append(punch_seams(depths[ROLLED]))
    depths.append(place_z_ties(depths[TILTED]))
    depths.append(punch_seams(depths[AXIS]))
    depths.append(exact_depth(base[WIDE], W, H, (BACK,)))
    A = (synth.FAR + synth.NEAR) / (synth.FAR - synth.NEAR)      # z = A + B / w: w (1 + e) is z' = A + (z - A) / (1 + e)
    for c in NOISY_CAMS:
        e = NOISE * (2.0 * rng.random((H, W)) - 1.0)
        depths.append((A + (depths[c].astype(np.float64) - A) / (1.0 + e)).astype(f32))
    depths.append(exact_depth(half, W, H))
    costs = []
    for _ in depths:
        pick = rng.choice(len(COST_VALUES) + 1, (H, W), p=COST_SHARES + [1.0 - sum(COST_SHARES)])
        cost = rng.random((H, W)).astype(f32)
        for i, v in enumerate(COST_VALUES):
            cost[pick == i] = v
        costs.append(cost)
    frames = {FRAME_OF[s]: rng.integers(0, 256, (H, W), dtype=np.uint8) for s in range(DEPTH_CAP)}
    for a in depths + costs + list(frames.values()) + cams:
        a.setflags(write=False)
    return {"cams": cams, "depths": depths, "costs": costs, "frames": frames}


# ---- fusion cases -----------------------------------------------------------------------------------------------------------------------
def tangent_variants(res, max_rel):
    """how csrc/fuse.hip's tangent() reads the two neighbours of every pixel, from a mirror result: (along the row, along the column), each
    [H, W] with 0 = neither usable, 1 = the lower-index neighbour only, 2 = the upper only, 3 = both (meaningful where res["valid"])"""
    w = np.pad(np.asarray(res["w"]), 1)
    c = w[1:-1, 1:-1]
    t = c.dtype.type

    def usable(n):
        with np.errstate(all="ignore"):
            return (n > 0) & (np.abs(n - c) / c <= t(max_rel))

    return usable(w[1:-1, :-2]) * 1 + usable(w[1:-1, 2:]) * 2, usable(w[:-2, 1:-1]) * 1 + usable(w[2:, 1:-1]) * 2


def _others(s):
    return [o for o in range(NCAM) if o != s]


# thresholds near the medians of the mirror's own sqrt(du^2 + dv^2) and |sw - w| / w over the NOISY neighbours (the nearest-pixel sample of a
# neighbour lies up to half a pixel off; the noise is uniform in +-2 %): both sides of both tests are well populated
MID_REPROJ, MID_REL = 0.5, 0.01


def thresholds_on_samples(size, ref, nbrs, min_consistent, mats):
    """(max_reproj_px, max_rel_depth) next to MID_REPROJ and MID_REL that are the mirror's own values: among the samples that agree at kept
    pixels under (MID_REPROJ, MID_REL) and pass the other test with a margin, the |sw - w| / w nearest MID_REL, and the du^2 + dv^2 nearest
    MID_REPROJ^2 that is the float32 square of its own root -- so one agreeing sample sits ON each `<=` (with these matrices)"""
    st = store(*size)
    res = fm.fuse(dict(enumerate(st["depths"])), {}, mats, ref, list(nbrs), min_consistent=min_consistent, max_reproj_px=MID_REPROJ, max_rel_depth=MID_REL)
    keep = res["keep"]
    reached = np.concatenate([t[0][keep] for t in res["tests"]])
    d2 = np.concatenate([t[1][keep] for t in res["tests"]])
    rel = np.concatenate([t[2][keep] for t in res["tests"]])
    with np.errstate(all="ignore"):
        root = np.sqrt(d2)
        square = reached & (root * root == d2) & (d2 <= f32(MID_REPROJ) * f32(MID_REPROJ)) & (rel <= f32(MID_REL) * f32(0.8))
        inside = reached & (rel <= f32(MID_REL)) & (d2 <= f32(MID_REPROJ) * f32(MID_REPROJ) * f32(0.8))
    px = root[square][np.abs(root[square] - f32(MID_REPROJ)).argmin()]
    rl = rel[inside][np.abs(rel[inside] - f32(MID_REL)).argmin()]
    return float(px), float(rl)


def tangent_rel_on_a_pixel(size, ref, mats, share=0.8):
    """a max_rel_depth that is the mirror's own |n.w - c.w| / c.w of one pixel of the reference map and its right-hand or lower neighbour,
    the one that leaves `share` of all such pairs usable: that pair sits ON the same-surface test's `<=`"""
    st = store(*size)
    res = fm.fuse({ref: st["depths"][ref]}, {}, mats, ref, [], min_consistent=0)
    w = res["w"]
    with np.errstate(all="ignore"):
        rel = np.concatenate([(np.abs(w[:, 1:] - w[:, :-1]) / w[:, :-1])[(w[:, 1:] > 0) & (w[:, :-1] > 0)],
                              (np.abs(w[1:] - w[:-1]) / w[:-1])[(w[1:] > 0) & (w[:-1] > 0)]])
    return float(np.sort(rel)[int(share * len(rel))])


def fuse_parameters(case, mats):
    """the case's parameters; the thresholds case takes its two from the mirror's samples"""
    _, size, ref, nbrs, kw, premise = case
    if premise.get("mid"):
        kw = dict(kw)
        kw["max_reproj_px"], kw["max_rel_depth"] = thresholds_on_samples(size, ref, nbrs, kw["min_consistent"], mats)
    if premise.get("surface_tie"):
        kw = dict(kw, max_rel_depth=tangent_rel_on_a_pixel(size, ref, mats))
    return kw


def _fuse_cases():
    """(name, (W, H), reference slot, neighbour slots, parameters, premise).  Premise keys: kept, dropped (least counts), agree (every value
    of agree from 0 to K occurs among the pixels with a normal), at_min (pixels with agree == min_consistent and == min_consistent - 1 both
    occur), seams (each tangent variant occurs on a tile seam and at an image border), all (every pixel is kept)"""
    cases = []
    for size in SIZES:
        big = size == SIZES[0]
        tag = "%dx%d" % size
        px = size[0] * size[1]
        # every slot of the rotated set as the reference, with and without a finite max_cost
        for s in range(NCAM) if big else (AXIS, ROLLED, SHIFTED):
            for cost in (np.inf, MAX_COST):
                cases.append(("turn%d_%s_%s" % (s, "cost" if cost < np.inf else "all", tag), size, s, _others(s),
                              dict(min_consistent=2, max_cost=float(cost)), dict(kept=px // 50, dropped=px // 50, at_min=True)))
        cases.append(("thresholds_" + tag, size, ROLLED, NOISY,
                      dict(min_consistent=2, max_reproj_px=MID_REPROJ, max_rel_depth=MID_REL), dict(kept=px // 50, dropped=px // 5, at_min=True, agree=big, mid=True)))
        cases.append(("seams_votes_" + tag, size, HOLEY_AXIS, [TILTED, ROLLED, WIDE], dict(min_consistent=1), dict(kept=px // 50, dropped=px // 10, seams=True)))
        cases.append(("seams_alone_" + tag, size, HOLEY_AXIS, [], dict(min_consistent=0), dict(kept=px // 10, dropped=px // 20, seams=True)))
        cases.append(("seams_rolled_" + tag, size, HOLEY_ROLLED, [TILTED, DEEP, SHIFTED, MIRRORED], dict(min_consistent=1), dict(kept=px // 50, dropped=px // 10, seams=True)))
        cases.append(("all_kept_" + tag, size, PLANE_ONLY, [], dict(min_consistent=0), dict(all=True)))
        cases.append(("ties_reference_" + tag, size, TIES, [AXIS, ROLLED, WIDE], dict(min_consistent=0, max_cost=float(MAX_COST)), dict(kept=px // 10, dropped=px // 10)))
        cases.append(("ties_neighbours_" + tag, size, AXIS, [TIES, HOLEY_ROLLED, MIRRORED], dict(min_consistent=1, max_cost=float(MAX_COST)),
                      dict(kept=px // 20, dropped=px // 10, at_min=True)))
        cases.append(("surface_tie_" + tag, size, ROLLED, [], dict(min_consistent=0), dict(kept=px // 50, dropped=px // 50, surface_tie=True)))
        cases.append(("half_pixel_" + tag, size, AXIS, [HALF, TILTED], dict(min_consistent=1), dict(kept=px // 10, dropped=1, at_min=True, half=True)))
        cases.append(("cost_zero_" + tag, size, TILTED, [AXIS, ROLLED, WIDE, DEEP, SHIFTED, TIES], dict(min_consistent=1, max_cost=0.0),
                      dict(kept=px // 100, dropped=px // 2, at_min=True)))
    return cases


FUSE_CASES = _fuse_cases()


def fuse_expected(case, mats, mirror=fm, dtype=np.float32):
    """the mirror's result of a fusion case; mats: slot -> (P, P^-1, centre)"""
    _, size, ref, nbrs, _, _ = case
    st = store(*size)
    return mirror.fuse(dict(enumerate(st["depths"])), dict(enumerate(st["costs"])), mats, ref, list(nbrs), dtype=dtype, **fuse_parameters(case, mats))


def check_fuse_premise(case, res, mats):
    name, (W, H), ref, nbrs, _, premise = case
    kw = fuse_parameters(case, mats)
    keep = res["keep"]
    if premise.get("all"):
        assert keep.all(), (name, int((~keep).sum()))
        return
    assert keep.sum() >= premise["kept"] and (~keep).sum() >= premise["dropped"], (name, int(keep.sum()), int((~keep).sum()))
    agree = res["agree"][res["has_normal"]]
    if premise.get("at_min"):
        m = kw["min_consistent"]
        assert (agree == m).any() and (agree == m - 1).any(), (name, np.bincount(agree, minlength=len(nbrs) + 1))
    if premise.get("agree"):
        assert set(range(len(nbrs) + 1)) <= set(agree.tolist()), (name, np.bincount(agree, minlength=len(nbrs) + 1))
    if premise.get("mid"):   # both threshold tests decide both ways on a fair share of the samples that reach them
        hn = res["has_normal"]
        reached = np.concatenate([t[0][hn] for t in res["tests"]])
        d2 = np.concatenate([t[1][hn] for t in res["tests"]])[reached]
        rel = np.concatenate([t[2][hn] for t in res["tests"]])[reached]
        t = d2.dtype.type
        below = (d2 <= t(kw["max_reproj_px"]) * t(kw["max_reproj_px"])).mean(), (rel <= t(kw["max_rel_depth"])).mean()
        assert len(d2) >= 20 and all(0.25 <= b <= 0.75 for b in below), (name, len(d2), below)
        assert (d2 == t(kw["max_reproj_px"]) * t(kw["max_reproj_px"])).any() and (rel == t(kw["max_rel_depth"])).any(), (name, "no sample ON a threshold")
    if premise.get("seams"):
        along_row, along_col = tangent_variants(res, kw.get("max_rel_depth", 0.01))
        valid = res["valid"]
        rows, cols = np.mgrid[0:H, 0:W]
        col_seam = np.isin(cols % 64, (63, 0)) & (cols > 0) & (cols < W - 1)
        row_seam = np.isin(rows % 4, (3, 0)) & (rows > 0) & (rows < H - 1)
        for v in (0, 1, 2, 3):   # (the one-tile image has no seam inside it)
            assert (valid & col_seam & (along_row == v)).any() or not col_seam.any(), (name, "row tangent variant %d on a column seam" % v)
            assert (valid & row_seam & (along_col == v)).any() or not row_seam.any(), (name, "column tangent variant %d on a row seam" % v)
        for v in (0, 1):    # at the last column / row the upper neighbour lies outside the image
            assert (valid & (cols == W - 1) & (along_row == v)).any() and (valid & (rows == H - 1) & (along_col == v)).any(), (name, "border", v)
        for v in (0, 2):    # (the one-tile image gives its first row away: that is its empty row)
            assert (valid & (cols == 0) & (along_row == v)).any() and ((valid & (rows == 0) & (along_col == v)).any() or H < 40), (name, "border", v)
        for v in (0, 1, 2, 3):
            assert (valid & (along_row == v)).any() and (valid & (along_col == v)).any(), (name, "variant", v)
        ntx = -(-W // 64)
        seg = np.array([[keep[r, 64 * b:64 * b + 64].sum() for b in range(ntx)] for r in range(H)])
        assert (seg == 0).any() and (seg.sum(1) == 0).any(), (name, "an empty segment and an empty row")
        assert (seg == 64).any() or H < 40, (name, "a full segment")   # (the one-tile image's are in its all_kept case)
        lone = valid & (along_row == 0) & (along_col == 0)
        assert lone.any() and not keep[lone].any()


# ---- TSDF cases: the rotated set ----------------------------------------------------------------------------------------------------------
def pairs(slots):
    return [(s, FRAME_OF[s]) for s in slots]


def tsdf_snapshots(st, mats, G, mirror=am):
    """the mirror's volume (am.Volume: the TSDF fields and the appearance cells) after each prefix of TSDF_LIST in LENGTHS, then after
    TSDF_LIST_COST under MAX_COST and TSDF_LIST_ZERO under max_cost = 0 on top -> ({key: (sum, count, cells)}, the final volume)"""
    origin, h = cube(G)
    vol = mirror.Volume(G, origin, h, 4 * h)
    wmap = mirror.tm.wmap
    maps = {s: wmap(st["depths"][s], None, mats[s]) for s in range(DEPTH_CAP)}
    snaps, done = {}, 0
    for n in LENGTHS:
        vol.integrate_frames(maps, mats, st["frames"], pairs(TSDF_LIST[done:n]))
        done = n
        snaps[n] = (vol.sum.copy(), vol.count.copy(), vol.cells.copy())
    for key, slots, mc in (("cost", TSDF_LIST_COST, MAX_COST), ("zero", TSDF_LIST_ZERO, f32(0.0))):
        maps_c = {s: wmap(st["depths"][s], st["costs"][s], mats[s], mc) for s in slots}
        vol.integrate_frames(maps_c, mats, st["frames"], pairs(slots))
        snaps[key] = (vol.sum.copy(), vol.count.copy(), vol.cells.copy())
    return snaps, vol


# ---- TSDF ties ----------------------------------------------------------------------------------------------------------------------------
def project_nodes(vol, P, W, H):
    """DESIGN.md section 12 rules 2 and 3 as tests/tsdf_mirror.py's Volume.integrate states them -> (qw, u, v, fc, fr, hit), each [G, G, G]"""
    x, y, z = vol.x[None, None, :], vol.y[None, :, None], vol.z[:, None, None]
    P = np.asarray(P, f32)
    halfW, halfH = f32(W) * f32(0.5), f32(H) * f32(0.5)
    with np.errstate(all="ignore"):
        q = [P[r, 0] * x + ((P[r, 1] * y + P[r, 2] * z) + P[r, 3]) for r in (0, 1, 3)]
        qx, qy, qw = (np.broadcast_to(a, (vol.G,) * 3).astype(f32) for a in q)
        inv = f32(1.0) / qw
        u = (qx * inv + f32(1.0)) * halfW - f32(0.5)
        v = (f32(1.0) - qy * inv) * halfH - f32(0.5)
        fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        hit = (qw > f32(0.0)) & (fc >= f32(0.0)) & (fc < f32(W)) & (fr >= f32(0.0)) & (fr < f32(H))
    return qw, u, v, fc, fr, hit


T_TIES = [f32(-1.0), down(-1.0), f32(1.0), down(1.0)]   # updated with -1; not updated; counted, no vote; counted and voted
BAND_W, BAND_H, BAND_G = 67, 45, 50
BAND_ORIGIN = np.array([-2.7, -2.7, -6.2], f32)
BAND_H_NODE = f32(5.4 / 49)
BAND_TAU = f32(2.0)                                     # a power of two: inv_tau and (wd - qw) inv_tau are exact
BAND_LIST = [0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0]   # 19 entries: LENGTHS' prefixes


def band_cameras():
    """near = 0.5: t = 1 - 2^-24 needs qw below 2 (its ulp 2^-23 or finer), t = -1 - 2^-23 needs wd below 4"""
    return [synth.camera_at((0.013, -0.021, 0.0371), BAND_W, BAND_H, near=0.5),   # (off the origin: qw = -z + c_z takes every low bit)
            looking(BAND_W, BAND_H, 9.0, -7.0, 65.0, near=0.5)]


def band_volume(mirror=am):
    return mirror.Volume(BAND_G, BAND_ORIGIN, BAND_H_NODE, BAND_TAU)


def band_ties(mats, per_tie=24):
    """depth maps of band_cameras() (the scene's exact maps) in which, for chosen nodes of the band volume, the pixel the node lands on holds
    a depth whose w (tsdf_mirror.wmap's arithmetic with `mats`) puts the node's t exactly on each of T_TIES; found by trying the floats
    around the closed-form depth.  -> (depths, placed [camera][tie] counts, nodes [camera] -> list of ((k, j, i), tie index))"""
    vol = band_volume()
    cams = band_cameras()
    rng = np.random.Generator(np.random.PCG64(0xBA9D))
    W, H = BAND_W, BAND_H
    depths, placed, nodes = [], [], []
    for s, cam in enumerate(cams):
        P, Pi = (np.asarray(m, f32) for m in mats[s][:2])
        d = exact_depth(cam, W, H)
        qw, _, _, fc, fr, hit = project_nodes(vol, P, W, H)
        taken = np.zeros((H, W), bool)
        count = [0] * len(T_TIES)
        mine = []
        b = Pi[3].astype(np.float64)
        for flat in rng.permutation(np.nonzero(hit.ravel())[0]):
            if min(count) >= per_tie:
                break
            r, c = int(fr.ravel()[flat]), int(fc.ravel()[flat])
            if taken[r, c]:
                continue
            q = qw.ravel()[flat]
            ties = [k for k in np.argsort(count) if count[k] < per_tie]
            xn, yn = fm.pixel_xn(c, W), fm.pixel_yn(r, H)
            for k in ties:
                with np.errstate(all="ignore"):
                    wd0 = float(q) + float(T_TIES[k]) * float(BAND_TAU)
                    if not wd0 > 0.5:
                        continue
                    z0 = f32((1.0 / wd0 - (b[0] * float(xn) + b[1] * float(yn) + b[3])) / b[2])   # w = 1 / (P^-1 (xn, yn, z, 1)).w
                    if not (-0.99 < z0 < 0.99):
                        continue
                    cand = (np.array(z0, f32).view(np.int32) + np.arange(-300, 301, dtype=np.int32)).view(f32)
                    t = (_wmap_at(P, Pi, xn, yn, cand) - q) * vol.inv_tau
                ok = np.nonzero(t == T_TIES[k])[0]
                if len(ok):
                    d[r, c] = cand[ok[0]]
                    taken[r, c] = True
                    count[k] += 1
                    mine.append((np.unravel_index(flat, hit.shape), int(k)))
                    break
        depths.append(d)
        placed.append(count)
        nodes.append(mine)
    return depths, placed, nodes


def _wmap_at(P, Pi, xn, yn, z):
    """tsdf_mirror.wmap's value at one pixel centre for an array of stored depths"""
    with np.errstate(all="ignore"):
        X = fm._unproject(Pi, f32(xn), f32(yn), np.asarray(z, f32))
        w = fm._prow(P, 3, X)
        return np.where(fm._valid(np.asarray(z, f32), None, np.inf, f32) & (w > f32(0.0)), w, f32(np.nan)).astype(f32)


# ---- TSDF pixel rounding --------------------------------------------------------------------------------------------------------------------
# 64 x 4 with fovx = 1: P[0][0] = 2 and P[1][1] = 32 exactly, so for the camera at the origin a node (x, y, z) has u + 0.5 = 32 + 64 x / w and
# v + 0.5 = 2 - 64 y / w without a rounding wherever 1 / w is exact.  With h = 1/16 and nodes on the multiples of h the layer z = -4 has
# u + 0.5 = 32 + i': every integer, so every node of that layer sits ON a pixel seam (floor(u + 0.5) and round-half-even part at the odd ones),
# one node is on the optical axis, x = 2 lands ON fc = W (outside), x = -2 on fc = 0 (inside)
ROUND_W, ROUND_H, ROUND_G = 64, 4, 65
ROUND_ORIGIN = np.array([-2.0, -2.0, -6.0], f32)
ROUND_H_NODE = f32(1.0 / 16)
ROUND_TAU = f32(0.25)
ROUND_LIST = [0, 1, 2, 1, 0, 2, 2, 0, 1, 1, 2, 0, 0, 2, 1, 2, 1, 0, 2]  # 19 entries: LENGTHS' prefixes
ON_A_NODE, TURNED_ON_A_NODE = 1, 2


def round_cameras():
    """the camera at the origin; one ON the node (0.25, -0.5, -3) (that node's qw is exactly 0, and half the volume is behind it); a turned
    and rolled one on the node (-0.5, 0.25, -2.5)"""
    W, H = ROUND_W, ROUND_H
    return [synth.camera_at((0.0, 0.0, 0.0), W, H, fovx=1.0, near=1.0, far=8.0),
            synth.camera_at((0.25, -0.5, -3.0), W, H, fovx=1.0, near=0.25, far=8.0),
            synth.camera_at((-0.5, 0.25, -2.5), W, H, fovx=1.0, near=0.25, far=8.0, rot=rotation(25.0, -20.0, 70.0))]


def round_depths():
    return [exact_depth(c, ROUND_W, ROUND_H, FLOOR) for c in round_cameras()]


def round_volume(mirror=am):
    return mirror.Volume(ROUND_G, ROUND_ORIGIN, ROUND_H_NODE, ROUND_TAU)


def crafted_frames(n, W, H, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return {s: rng.integers(0, 256, (H, W), dtype=np.uint8) for s in range(n)}


def integrate_crafted(vol, depths, mats, frames, slots, mirror=am):
    """the mirror's integrate_frames of crafted maps, frame slot = depth slot"""
    maps = {s: mirror.tm.wmap(depths[s], None, mats[s]) for s in set(slots)}
    return vol.integrate_frames(maps, mats, frames, [(s, s) for s in slots])


def crafted_snapshots(vol, depths, mats, frames, slots, mirror=am):
    """the mirror's volume after each prefix of `slots` in LENGTHS -> {n: (sum, count, cells)}"""
    maps = {s: mirror.tm.wmap(depths[s], None, mats[s]) for s in set(slots)}
    snaps, done = {}, 0
    for n in LENGTHS:
        vol.integrate_frames(maps, mats, frames, [(s, s) for s in slots[done:n]])
        done = n
        snaps[n] = (vol.sum.copy(), vol.count.copy(), vol.cells.copy())
    return snaps
