"""Crafted meshes, cameras and frames for the rasteriser (csrc/raster.hip vs oracle/raster_oracle.c vs tests/raster_mirror.py), each a named
case.  tests/test_raster_cases_cpu.py validates the cases and the oracle against the mirrors on any machine; tests/test_raster_cases_gpu.py
runs the kernels on them.  Geometry is written in PIXEL units (u, v): pixel (col, row) has its centre at (col + 0.5, row + 0.5), NDC
x = 2 u / W - 1, y = 1 - 2 v / H -- so "on a pixel centre", "on a pixel corner" and "on the 15 / 16 seam" can be read off the numbers.

A  fill rule and watertightness      exact mirror; power-of-two frames, dyadic cameras
B  depth range, ties, degenerates    exact mirror (orthographic: zn = z)
C  camera-plane crossings            float64 classifier
D  binning                           oracle, both bin modes
E  shadow pass, texture, mip chain   oracle"""
import functools
import itertools

import numpy as np

from mvs_amd import synth

f32 = np.float32
BIN = 16            # csrc/raster.hip: one face bin per 16 x 16 raster tile
BIN_MAXCOVER = 4    # a face whose box touches more bins goes to the shared list
BIN_MIN_FACES = 16384

# ---- cameras -----------------------------------------------------------------------------------------------------------------------------
ORTHO = np.eye(4, dtype=f32)                                                                    # clip = (x, y, z, 1): zn = z
PERSP = np.array([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, -1.25, -2.5], [0, 0, -1, 0]], f32)         # w = -z, zn = 1.25 - 2.5 / w
CAMS = {"ortho": ORTHO, "persp": PERSP}
# eight depth levels per camera, nearest first: z of the orthographic camera, w of the perspective one (dyadic; zn = -0.75 ... 0.9375)
LEVELS = {"ortho": [k / 8.0 - 0.5 for k in range(8)], "persp": [1.25, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0]}
# |f32 z - exact z| per shape under the perspective camera, where 1 / det need not be a power of two (every orthographic case is exact): 4 x the
# largest difference the CPU oracle shows over the shape's frames and vertex orders -- 7.947285973752827e-08 on the fans and the grid,
# 3.9736429868764134e-08 on ndc_edge, 0 on diag_quad and slivers (the plane's coefficients times a rounded 1 / det)
Z_TOL_PERSP = {"diag_quad": 0.0, "slivers": 0.0, "fan_centres": 4 * 7.947285973752827e-08, "fan_corners": 4 * 7.947285973752827e-08,
               "grid_hv": 4 * 7.947285973752827e-08, "ndc_edge": 4 * 3.9736429868764134e-08}


def z_tol(name):
    shape, cam, _ = name.split("-")
    return 0.0 if cam == "ortho" else Z_TOL_PERSP[shape]


PERMS = list(itertools.permutations(range(3)))                                                  # three keep the winding, three flip it


def place(cam, u, v, d, W, H):
    """the world vertex (x, y, z, 1) that camera `cam` puts at pixel coordinates (u, v) with depth parameter d (ortho: z, persp: w)"""
    x, y = 2.0 * u / W - 1.0, 1.0 - 2.0 * v / H
    return [x, y, d, 1.0] if cam == "ortho" else [x * d, y * d / 2.0, -d, 1.0]


def mesh_of(cam, W, H, tris, exact=True):
    """tris: a list of faces, each three (u, v, d) -> (verts4, faces3) with unshared vertices; exact: every coordinate must be an f32 value"""
    verts = np.array([place(cam, u, v, d, W, H) for t in tris for (u, v, d) in t], np.float64)
    v32 = verts.astype(f32)
    assert not exact or np.array_equal(v32.astype(np.float64)[np.isfinite(verts)], verts[np.isfinite(verts)]), "a crafted vertex is no f32 value"
    return v32, np.arange(len(v32), dtype=np.int32).reshape(-1, 3)


def permuted(faces, which):
    """vertex order `which` (0..5 of PERMS) for every face, or "mixed": face i takes order i mod 6"""
    faces = np.asarray(faces)
    if which == "mixed":
        return np.stack([faces[i][list(PERMS[i % 6])] for i in range(len(faces))]).astype(np.int32)
    return faces[:, list(PERMS[which])].astype(np.int32)


def _case(name, cam, W, H, tris, exact=True, **kw):
    verts, faces = mesh_of(cam, W, H, tris, exact)
    return dict(name=name, W=W, H=H, cam=CAMS[cam], verts=verts, faces=faces, **kw)


def _quad(u0, v0, u1, v1, d0, d1=None, flip=False):
    """two faces of the rectangle [u0, u1] x [v0, v1] at depths d0 / d1, split by the main or (flip) the other diagonal"""
    d1 = d0 if d1 is None else d1
    p = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
    if flip:
        return [[p[0] + (d0,), p[1] + (d0,), p[3] + (d0,)], [p[1] + (d1,), p[2] + (d1,), p[3] + (d1,)]]
    return [[p[0] + (d0,), p[1] + (d0,), p[2] + (d0,)], [p[0] + (d1,), p[2] + (d1,), p[3] + (d1,)]]


# ---- A: fill rule and watertightness ---------------------------------------------------------------------------------------------------------
def _fan(lv, r):
    c = (31.5, 15.5)
    rim = [(c[0] + r * dx, c[1] + r * dy) for dx, dy in [(-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0)]]
    tris = []
    for i in range(8):
        p, q = rim[i], rim[(i + 1) % 8]
        if i & 1:
            p, q = q, p                     # mixed windings
        tris.append([c + (lv[i],), p + (lv[i],), q + (lv[i],)])
    return tris


def _a_shapes(cam, W, H):
    lv = LEVELS[cam]
    shapes = {
        # the diagonal runs through the pixel centres (8 + k, 4 + k)
        "diag_quad": _quad(8.5, 4.5, 24.5, 20.5, lv[1], lv[2]),
        # centre vertex on a pixel centre; rim vertices on centres (r = 8) and on pixel corners / edge midpoints (r = 8.5)
        "fan_centres": _fan(lv, 8.0),
        "fan_corners": _fan(lv, 8.5),
        # 2 x 2 quads whose shared edges lie on the centre column 20 and the centre row 14: the a == 0 branch of the tie rule
        "grid_hv": (_quad(10.5, 6.5, 20.5, 14.5, lv[0], lv[1]) + _quad(20.5, 6.5, 30.5, 14.5, lv[2], lv[3], flip=True) +
                    _quad(10.5, 14.5, 20.5, 22.5, lv[4], lv[5], flip=True) + _quad(20.5, 14.5, 30.5, 22.5, lv[6], lv[7])),
        # narrower than a pixel: the first holds no pixel centre, the second exactly one, (20, 8)
        "slivers": [[(10.125, 5.125, lv[0]), (10.375, 5.125, lv[0]), (10.25, 20.875, lv[0])],
                    [(12.0, 8.25, lv[1]), (21.0, 8.25, lv[1]), (21.0, 8.53125, lv[1])]],
        # vertices exactly on NDC +-1: the screen split along its diagonal, a face that is mostly off-screen over the bottom-left corner, and
        # thin faces along the top row and the last column
        "ndc_edge": [[(0, H, lv[2]), (W, H, lv[2]), (0, 0, lv[2])], [(W, 0, lv[3]), (0, 0, lv[3]), (W, H, lv[3])],
                     [(-W / 2, 1.5 * H, lv[0]), (0.75 * W, 1.5 * H, lv[0]), (-W / 2, 0.25 * H, lv[0])],
                     [(0, 0, lv[1]), (W, 0, lv[1]), (W / 2, 0.75, lv[1])], [(W, 0, lv[1]), (W, H, lv[1]), (W - 0.75, H / 2, lv[1])]],
    }
    return shapes


A_NAMES = ["diag_quad", "fan_centres", "fan_corners", "grid_hv", "slivers", "ndc_edge"]
A_CASES = ["%s-%s-%dx%d" % (s, cam, W, H) for s in A_NAMES for cam in ("ortho", "persp") for (W, H) in ((64, 32), (128, 64))]
A_ORDERS = [0, 1, 2, 3, 4, 5, "mixed"]


@functools.lru_cache(maxsize=None)
def a_case(name):
    shape, cam, size = name.split("-")
    W, H = (int(s) for s in size.split("x"))
    return _case(name, cam, W, H, _a_shapes(cam, W, H)[shape], shape=shape)


# ---- box slack: edges one ulp beyond a pixel centre in frames that are no power of two --------------------------------------------------------------
# With 1 / W rounded, ((xn(col) + 1) W - 1) / 2 need not give back col: it can come out a hair below, and a box cut there without its pixel of slack
# drops the column.  Face k of "columns" has its right edge one f32 ulp right of the centre of column k, face k of "rows" its bottom edge one ulp
# below the centre of row k.  The other two vertices are chosen so that the f32 edge function of that edge is EXACT in sign (one vertex coordinate
# 0, the edge's length a power of two: e = fma(+-0.5, xn, 0.5 xmax) is 0.5 (xmax - xn) rounded once), so the pixel is inside by the contract's own
# arithmetic, not by luck.  Faces k' > k cover the pixel too, farther away: z = k / 512 - 0.5 names the face that drew it.
# (Frames in which the round trip happens to be exact for every column, 333 x 211 for one, pin nothing and are not listed.)
ULP_CASES = [("columns", 100, 30), ("rows", 30, 100)]


def pixel_centres(W, H):
    """the f32 NDC pixel centres of the contract: fma(2 col + 1, 1 / W, -1), fma(-(2 row + 1), 1 / H, 1) (the product is exact in float64)"""
    inv_w, inv_h = np.float64(f32(1) / f32(W)), np.float64(f32(1) / f32(H))
    return ((2.0 * np.arange(W) + 1.0) * inv_w - 1.0).astype(f32), (1.0 - (2.0 * np.arange(H) + 1.0) * inv_h).astype(f32)


@functools.lru_cache(maxsize=None)
def ulp_case(kind, W, H):
    xn, yn = pixel_centres(W, H)
    verts = []
    if kind == "columns":
        for k, x in enumerate(np.nextafter(xn, f32(2))):
            verts += [[x, 0, k / 512.0 - 0.5, 1], [x, 0.5, k / 512.0 - 0.5, 1], [-3, 0, k / 512.0 - 0.5, 1]]
        band = ((yn > 0.05) & (yn < 0.4))[:, None] & np.ones(W, bool)[None, :]           # clear of the faces' other edges
        expected = np.broadcast_to(np.arange(W) / 512.0 - 0.5, (H, W))
    else:
        for k, y in enumerate(np.nextafter(yn, f32(-2))):
            verts += [[0, y, k / 512.0 - 0.5, 1], [0.5, y, k / 512.0 - 0.5, 1], [0, 3, k / 512.0 - 0.5, 1]]
        band = np.ones(H, bool)[:, None] & ((xn > 0.05) & (xn < 0.4))[None, :]
        expected = np.broadcast_to((np.arange(H) / 512.0 - 0.5)[:, None], (H, W))
    verts = np.array(verts, f32)
    return dict(name="ulp_%s_%dx%d" % (kind, W, H), W=W, H=H, cam=ORTHO, verts=verts, faces=np.arange(len(verts), dtype=np.int32).reshape(-1, 3),
                band=band, expected=expected)


# ---- B: depth range, ties, degenerate faces (orthographic, 64 x 32: zn = z) ------------------------------------------------------------------
STEP = 2.0 ** -10                 # one dyadic step beyond a depth limit
NAN, INF = float("nan"), float("inf")


def _b_tris():
    good = _quad(4.5, 4.5, 40.5, 24.5, 0.5)                                                       # faces 0, 1
    return {
        # four columns of quads: zn = -1 is kept; zn = +1 equals the clear depth and is never drawn; a face one step in front of the near limit
        # is rejected and shows the face behind it; a face one step behind the far limit is rejected and the face listed after it is drawn
        "zn_limits": (_quad(2.5, 4.5, 14.5, 20.5, -1.0) + _quad(16.5, 4.5, 28.5, 20.5, 1.0) +
                      _quad(30.5, 4.5, 42.5, 20.5, -1.0 - STEP) + _quad(30.5, 4.5, 42.5, 20.5, 0.5) +
                      _quad(44.5, 4.5, 58.5, 20.5, 1.0 + STEP) + _quad(44.5, 4.5, 58.5, 20.5, 0.5)),
        # a quad (rows 0-15) and two slanted faces.  z = (u - 10.5) / 16 - 1 on the first: zn = -1 exactly on the centres of column 10, which are kept; columns < 10 show the quad
        # behind.  z = (u - 8.5) / 16 on the third: zn = +1 exactly on column 24, where (equal to the clear depth) nothing is drawn
        "near_far_cut": (_quad(0.5, 0.5, 64.5, 16.5, 0.75) +
                         [[(2.5, 2.5, -1.5), (34.5, 2.5, 0.5), (2.5, 18.5, -1.5)], [(40.5, 20.5, 2.0), (8.5, 20.5, 0.0), (40.5, 28.5, 2.0)]]),
        # the same face three times, coplanar overlapping faces listed before and after, a nearer face in between
        "duplicates": (_quad(8.5, 4.5, 40.5, 20.5, 0.25) + _quad(8.5, 4.5, 40.5, 20.5, 0.25) + [[(2.5, 2.5, 0.25), (60.5, 2.5, 0.25), (2.5, 30.5, 0.25)]] +
                       _quad(16.5, 8.5, 24.5, 12.5, 0.0) + _quad(8.5, 4.5, 40.5, 20.5, 0.25, flip=True) +
                       [[(60.5, 30.5, 0.25), (2.5, 30.5, 0.25), (60.5, 2.5, 0.25)]]),
        # handled inputs between good faces: zero area (collinear), a repeated vertex, NaN and Inf coordinates -- all in front of the good ones
        "degenerate": (good + [[(8.5, 8.5, 0.0), (16.5, 12.5, 0.0), (24.5, 16.5, 0.0)], [(8.5, 8.5, 0.0), (8.5, 8.5, 0.0), (30.5, 20.5, 0.0)],
                               [(8.5, 8.5, 0.0), (NAN, 20.5, 0.0), (30.5, 8.5, 0.0)], [(8.5, 8.5, 0.0), (30.5, 20.5, INF), (30.5, 8.5, 0.0)],
                               [(INF, 8.5, 0.0), (8.5, -INF, 0.0), (30.5, 8.5, NAN)], [(-INF, 8.5, 0.0), (8.5, 20.5, 0.0), (30.5, 8.5, 0.0)]] +
                       [[(20.5, 2.5, 0.25), (50.5, 2.5, 0.25), (50.5, 28.5, 0.25)]]),
    }


B_CASES = ["zn_limits", "near_far_cut", "duplicates", "degenerate"]
DEGENERATE_GOOD = [0, 1, 8]        # the faces of "degenerate" that may draw
# a projector for the cases rendered with the orthographic camera: a shifted, slightly zoomed copy of it (every pixel in frame, unoccluded)
ORTHO_PROJECTOR = np.array([[0.875, 0, 0, 0.0625], [0, 0.875, 0, -0.03125], [0, 0, 1, 0], [0, 0, 0, 1]], f32)


def noise_frame(W, H, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def b_case(name):
    return _case(name, "ortho", 64, 32, _b_tris()[name], prj=ORTHO_PROJECTOR, frame=noise_frame(64, 32))


# ---- ties: equal depths whose owner changes the bytes of projected() -----------------------------------------------------------------------------
# A flat quad F at z = 0.25 and two quads slanted in x, z = 0.25 + (u - centre) / 32, that meet F's depth EXACTLY on the centres of column 16
# (S_a, listed before F) and of column 32 (S_b, listed after F); every face has a power-of-two det, so the f32 depths are equal bit for bit.  Both
# faces put the same point of space at a tied pixel, so the level-0 texel is the same whoever owns it -- but the mip level comes from the OWNER's
# finite differences, and the projector below shears z into its x (nx = 3 x + 4 z - 0.5): a pixel step moves u by 3 texels on F, by 7 on a slanted
# face, so the two owners blend different mip levels of a noise frame.  The projector's z row is zero: its depth is 0 everywhere and nothing is in
# shadow, so a render of one group of faces alone shows what that group gives at the tied pixels.  F's box touches 6 bins (the shared list), the
# slanted quads' 4 (the tiles' own lists); "tie_batches" adds 300 small faces behind everything in the bin of column 16-31, 150 listed before F and
# 150 after, so that the tied faces also sit in different batches of 256 candidates, binned or not.
TIE_PROJECTOR = np.array([[3, 0, 4, -0.5], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], f32)
TIE_CASES = ["tie_slant", "tie_batches"]
TIE_ROWS = slice(5, 21)                     # the rows of the quads, 4.5 < v <= 20.5
TIE_COLUMNS = {16: ("S_a", "F"), 32: ("F", "S_b")}     # tied column -> (the group listed first, which owns it; the group listed later)


@functools.lru_cache(maxsize=None)
def tie_case(name):
    W, H = 64, 32
    s_a = _quad(8.5, 4.5, 24.5, 20.5, 0.0)
    s_b = _quad(24.5, 4.5, 40.5, 20.5, 0.0, flip=True)
    for quad, centre in ((s_a, 16.5), (s_b, 32.5)):
        for t in quad:
            t[:] = [(u, v, 0.25 + (u - centre) / 32.0) for (u, v, _) in t]
    flat = _quad(8.5, 4.5, 40.5, 20.5, 0.25)
    rng = np.random.default_rng(5)
    fill = _small_faces(rng, 300, 17.5, 1.5, 30.5, 14.5, 0.5, 0.9) if name == "tie_batches" else []
    tris = s_a + fill[:150] + flat + fill[150:] + s_b
    n = len(fill) // 2
    groups = {"S_a": [0, 1], "F": [2 + n, 3 + n], "S_b": [4 + 2 * n, 5 + 2 * n]}
    return _case(name, "ortho", W, H, tris, exact=False, prj=TIE_PROJECTOR, frame=noise_frame(W, H, 11), groups=groups)


# ---- C: faces across the camera plane (camera at the origin looking along -z: w = -z) -----------------------------------------------------------
C_SIZES = [(64, 48), (333, 211)]
_C_FACES = {
    "one_behind": ([[-50, -1, -40], [50, -1, -40], [0, -1, 30]], 0.5),
    "two_behind": ([[0, -1, -40], [-50, -1, 30], [50, -1, 30]], 0.5),
    "on_w0": ([[-50, -1, -40], [50, -1, -40], [0, -1, 0]], 0.5),               # the third vertex has w == 0 exactly
    "all_behind": ([[-50, -1, 5], [50, -1, 10], [0, 3, 30]], 0.5),             # draws nothing
    "corner": ([[-1.2, -0.8, -3], [-8, 1, 2], [1, -7, 2]], 0.5),                # what is in front shows in the bottom-left corner only
    "whole_screen": ([[-100, -100, -5], [100, -100, -5], [0, 300, 10]], 0.5),  # crosses w = 0 far above the frustum
    "ground_strip": ([[-50, -1, -40], [50, -1, -40], [0, -1, 30]], 0.001),     # the face cameras' near plane (heuristic.cpp:193-247)
}
# the classifier's eps per shape (default 1e-4).  With near = 0.001, zn = 1.0000333 - 0.002 / w: everything farther than w = 15 is within 1e-4 of
# the far limit, the strip reaches w = 40, and 1e-5 (w < 44) is still a hundred times the f32 rounding of zn near 1
C_EPS = {"ground_strip": 1e-5}
C_CASES = ["%s-%dx%d" % (n, W, H) for n in _C_FACES for (W, H) in C_SIZES]


@functools.lru_cache(maxsize=None)
def c_case(name):
    shape, size = name.split("-")
    W, H = (int(s) for s in size.split("x"))
    pts, near = _C_FACES[shape]
    verts = np.concatenate([np.array(pts, f32), np.ones((3, 1), f32)], 1)
    cam = synth.camera_at([0, 0, 0], W, H, near=near, far=60.0)
    assert cam[3].tolist() == [0, 0, -1, 0]
    return dict(name=name, shape=shape, W=W, H=H, cam=cam, verts=verts, faces=np.array([[0, 1, 2]], np.int32), eps=C_EPS.get(shape, 1e-4))


# ---- D: binning ----------------------------------------------------------------------------------------------------------------------------
def face_boxes(case):
    """the bounding boxes of the contract (one pixel of slack, truncation, clamped to the frame) of faces in front of the camera, restated in
    float64 -> (F, 4) x0, y0, x1, y1.  Only the crafted binning cases use it, to show that their faces cover the bins they are meant to."""
    from raster_mirror import soup_of
    W, H = case["W"], case["H"]
    v = soup_of(case["verts"], case["faces"]).astype(np.float64).reshape(-1, 3, 3)
    m = case["cam"].astype(np.float64)
    clip = np.einsum("kj,fij->fik", m[:, :3], v) + m[:, 3]
    assert (clip[..., 3] > 0).all()
    nx, ny = clip[..., 0] / clip[..., 3], clip[..., 1] / clip[..., 3]
    x0 = np.clip(np.trunc(((nx.min(1) + 1) * W - 1) / 2 - 1), 0, W)
    x1 = np.clip(np.trunc(((nx.max(1) + 1) * W - 1) / 2 + 1), -1, W - 1)
    y0 = np.clip(np.trunc(((1 - ny.max(1)) * H - 1) / 2 - 1), 0, H)
    y1 = np.clip(np.trunc(((1 - ny.min(1)) * H - 1) / 2 + 1), -1, H - 1)
    return np.stack([x0, y0, x1, y1], 1).astype(int)


def bins_covered(case):
    """(F, 2): how many bin columns and rows each face's box touches"""
    b = face_boxes(case)
    return np.stack([b[:, 2] // BIN - b[:, 0] // BIN + 1, b[:, 3] // BIN - b[:, 1] // BIN + 1], 1)


def _tri_box(bx0, by0, bx1, by1, z):
    """a right triangle whose box is exactly the bins bx0..bx1 x by0..by1: one pixel more on any side would touch the next bin"""
    u0, u1, v0, v1 = BIN * bx0 + 1.75, BIN * (bx1 + 1) - 0.75, BIN * by0 + 1.75, BIN * (by1 + 1) - 0.75
    return [(u0, v0, z), (u1, v0, z), (u0, v1, z)]


MAXCOVER_BINS = [(2, 2), (4, 1), (1, 4), (5, 1), (3, 2), (2, 3), (8, 6)]     # bins touched by the faces of "maxcover", columns x rows


def _small_faces(rng, n, u0, v0, u1, v1, z0, z1):
    """n small triangles inside [u0, u1] x [v0, v1] at n distinct depths, shuffled so that face order and depth order differ"""
    zs = rng.permutation(np.linspace(z0, z1, n))
    tris = []
    for z in zs:
        c = rng.uniform([u0 + 3, v0 + 3], [u1 - 3, v1 - 3])
        p = c + rng.uniform(-3, 3, (3, 2))
        tris.append([(float(np.round(q[0] * 8) / 8), float(np.round(q[1] * 8) / 8), float(f32(z))) for q in p])
    return tris


def _large_faces(rng, n, W, H, z0, z1):
    zs = rng.permutation(np.linspace(z0, z1, n))
    tris = []
    for i, z in enumerate(zs):
        j = float(i % 7)
        t = [(-j, -3.0 + j, float(f32(z))), (2.0 * W + j, -2.0, float(f32(z))), (-4.0, 2.0 * H - j, float(f32(z)))]
        tris.append(t if i & 1 else [(W + 4.0 - u, H + 3.0 - v, z) for (u, v, z) in t])
    return tris


def _grid_mesh(nx, ny, drop=0):
    """nx x ny cells over NDC [-0.9375, 0.9375]^2, two faces each, z a smooth function of the vertex; `drop` faces left out at the end"""
    xs, ys = np.linspace(-0.9375, 0.9375, nx + 1), np.linspace(-0.9375, 0.9375, ny + 1)
    X, Y = np.meshgrid(xs, ys)
    Z = 0.25 * np.sin(3.0 * X) * np.cos(2.0 * Y)
    verts = np.stack([X.ravel(), Y.ravel(), Z.ravel(), np.ones(X.size)], 1).astype(f32)
    idx = np.arange(X.size).reshape(ny + 1, nx + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([b, d, c], 1)], 1).reshape(-1, 3).astype(np.int32)
    return verts, faces[:len(faces) - drop]


def _soup_scene(W, H, seed):
    rng = np.random.default_rng(seed)
    return _small_faces(rng, 60, -2, -2, W + 2, H + 2, -0.5, 0.5) + _large_faces(rng, 3, W, H, 0.6, 0.7)


D_CASES = ["maxcover", "seam", "small300", "small300_large5", "large300", "empty_bins", "behind", "ragged_333x211", "ragged_17x17", "single_8x8"]
D_SWITCH = ["grid_16384", "grid_16383"]     # the default switch to binning at BIN_MIN_FACES faces


@functools.lru_cache(maxsize=None)
def d_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = {}
    if name == "maxcover":
        W, H = 128, 96
        spots = [(0, 0), (2, 0), (7, 1), (1, 5), (2, 2), (5, 1), (0, 0)]
        tris = [_tri_box(bx, by, bx + nx - 1, by + ny - 1, -0.5 + 0.125 * i) for i, ((nx, ny), (bx, by)) in enumerate(zip(MAXCOVER_BINS, spots))]
    elif name == "seam":
        # rectangles whose edges lie on the pixel boundary 16.0 between the tiles, on the centres 15.5 / 16.5 next to it, and across it
        W, H = 64, 48
        tris = (_quad(4.5, 4.5, 16.0, 16.0, -0.25) + _quad(16.0, 16.0, 28.5, 31.5, -0.125) + _quad(15.5, 20.5, 16.5, 40.5, 0.0) +
                _quad(30.5, 15.5, 50.5, 16.5, 0.125) + _quad(31.0, 31.0, 33.0, 33.0, 0.25) + _quad(40.25, 2.5, 47.75, 15.75, 0.375))
    elif name in ("small300", "small300_large5", "large300"):
        W, H = 64, 48
        small = _small_faces(rng, 300, 17.5, 17.5, 30.5, 30.5, -0.5, 0.25)      # every box inside the tile of bin (1, 1)
        if name == "small300":
            tris = small
        elif name == "small300_large5":
            large = _large_faces(rng, 5, W, H, -0.25, 0.5)
            large[3] = large[1]                                                  # equal faces: the lower id wins, whichever list it came from
            tris = small[:100] + large[:2] + small[100:250] + large[2:4] + small[250:] + [small[7]] + large[4:]
        else:
            tris = _large_faces(rng, 300, W, H, -0.5, 0.5)
            tris[290] = tris[3]
            tris[17] = tris[260]
    elif name == "empty_bins":
        W, H = 128, 96
        tris = _small_faces(rng, 12, 100, 70, 127, 95, -0.5, 0.5)
    elif name == "behind":
        W, H = 64, 48
        verts, faces = _grid_mesh(8, 8)
        verts[:, 2] += 4.0                                                       # z > 0: behind a camera that looks along -z
        return dict(name=name, W=W, H=H, cam=synth.camera_at([0, 0, 0], W, H, near=0.5, far=60.0), verts=verts, faces=faces,
                    prj=synth.camera_at([0.2, 0, 0], W, H, near=0.5, far=60.0), frame=noise_frame(W, H))
    else:
        W, H = (int(s) for s in name.split("_")[1].split("x"))
        tris = _soup_scene(W, H, W)
    return _case(name, "ortho", W, H, tris, exact=False, prj=ORTHO_PROJECTOR, frame=noise_frame(W, H), **kw)


@functools.lru_cache(maxsize=None)
def d_switch_case(name):
    W, H = 160, 96
    verts, faces = _grid_mesh(128, 64, drop=BIN_MIN_FACES - int(name.split("_")[1]))
    return dict(name=name, W=W, H=H, cam=ORTHO, verts=verts, faces=faces, prj=ORTHO_PROJECTOR, frame=noise_frame(W, H))


# ---- E: shadow pass, projector limits, texture wrap, mip chain -----------------------------------------------------------------------------------
SHADOW_SIZES = [(3, 5), (17, 6), (255, 4), (257, 3)]


@functools.lru_cache(maxsize=None)
def shadow_case(W, H):
    """the occluder scene of test_raster_cpu.py::test_shadow_masks_occluded_surface"""
    far = np.array([[-4, -4, -6, 1], [4, -4, -6, 1], [4, 4, -6, 1], [-4, 4, -6, 1]], f32)
    near = np.array([[-0.4, -0.4, -3, 1], [0.4, -0.4, -3, 1], [0.4, 0.4, -3, 1], [-0.4, 0.4, -3, 1]], f32)
    return dict(name="shadow_%dx%d" % (W, H), W=W, H=H, verts=np.concatenate([far, near]),
                faces=np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32), cam=synth.camera_at([0, 0, 0], W, H),
                prj=synth.camera_at([1.5, 0, 0], W, H), frame=noise_frame(W, H))


def _flat_screen():
    """the whole screen of the orthographic camera at z = 0, four faces around the centre"""
    v = np.array([[-1, -1, 0, 1], [1, -1, 0, 1], [1, 1, 0, 1], [-1, 1, 0, 1], [0, 0, 0, 1]], f32)
    return v, np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)


ONE_BELOW = float(np.nextafter(f32(1), f32(0)))       # the largest f32 below 1
# projectors that put EVERY point at one constant NDC x or y: exactly on the limit (masked: the inequality is strict) or one ulp inside it, where
# the texture coordinate rounds to the frame's edge and the bilinear fetch reads the wrap padding
LIMIT_CASES = [(axis, sign, on) for axis in (0, 1) for sign in (-1.0, 1.0) for on in (True, False)]


def limit_case(axis, sign, on):
    W, H = 64, 32
    verts, faces = _flat_screen()
    prj = np.array(ORTHO_PROJECTOR)
    prj[axis] = [0, 0, 0, sign * (1.0 if on else ONE_BELOW)]
    return dict(name="limit", W=W, H=H, cam=ORTHO, verts=verts, faces=faces, prj=prj, frame=noise_frame(W, H))


def zoom_projector(zx, zy, cx=0.0, cy=0.0):
    """an orthographic projector that sees [cx - 1 / zx, cx + 1 / zx] x [cy - 1 / zy, cy + 1 / zy] of the screen plane: a main-view pixel covers
    zx x zy texels of its frame, so rho = max(zx, zy) exactly (up to f32 rounding of the finite differences)"""
    return np.array([[zx, 0, 0, -zx * cx], [0, zy, 0, -zy * cy], [0, 0, 1, 0], [0, 0, 0, 1]], f32)


def mip_levels(W, H):
    n = 0
    while W > 1 or H > 1:
        W, H, n = max(1, W >> 1), max(1, H >> 1), n + 1
    return n


# (W, H, zoom x, zoom y): levels 0-1, 1-2, 2-3 ... of frames where one axis reaches 1 early, where level 1 is 64 (all in the one-workgroup tail)
# or 65 texels wide (one more mip_reduce launch), odd sizes, and a zoom beyond the last level (its y centre on a pixel centre, so a row is in frame)
MIP_CASES = [(256, 4, 1.5, 1.5), (256, 4, 3.0, 1.0), (256, 4, 24.0, 1.0), (5, 300, 1.5, 1.5), (5, 300, 1.0, 6.0), (5, 300, 1.0, 48.0),
             (128, 128, 1.5, 1.5), (128, 128, 3.0, 3.0), (130, 130, 1.5, 1.5), (130, 130, 3.0, 3.0), (37, 23, 1.5, 2.5), (37, 23, 5.0, 3.0),
             (256, 4, 1.0, 600.0), (5, 300, 1.0, 600.0), (37, 23, 1.0, 80.0)]


def mip_case(W, H, zx, zy):
    verts, faces = _flat_screen()
    cy = 1.0 - (2 * (H // 2) + 1.0) / H      # the centre of row H // 2
    return dict(name="mip", W=W, H=H, cam=ORTHO, verts=verts, faces=faces, prj=zoom_projector(zx, zy, 0.0, cy), frame=noise_frame(W, H),
                levels=mip_levels(W, H), rho=max(zx, zy))
