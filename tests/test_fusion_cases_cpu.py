"""The crafted fusion and TSDF cases of tests/fusion_cases.py without a GPU: every case's premise holds in the mirrors; the mirrors are right
on general cameras (against the closed form of the scene and their own float64 path), not merely self-consistent; and every entry of a table of
small perturbations of the mirrors' text -- a summation order, a coefficient, an inclusive comparison, a rounding -- changes the expected
bytes of a named case, so tests/test_fusion_cases_gpu.py would fail on a kernel that is wrong in that way."""
import functools
import sys
import types

import numpy as np
import pytest

import appearance_mirror as am
import fuse_mirror as fm
import fusion_cases as fc
import tsdf_mirror as tm

f32 = np.float32
EPS = float(np.finfo(f32).eps)


@functools.lru_cache(maxsize=None)
def _mats(W, H):
    st = fc.store(W, H)
    return {s: fc.mats32(st["cams"][s]) for s in range(fc.DEPTH_CAP)}


@functools.lru_cache(maxsize=None)
def _band():
    mats = {s: fc.mats32(c) for s, c in enumerate(fc.band_cameras())}
    depths, placed, nodes = fc.band_ties(mats)
    return mats, depths, placed, nodes, fc.crafted_frames(2, fc.BAND_W, fc.BAND_H, 0xBA9D)


@functools.lru_cache(maxsize=None)
def _round():
    return {s: fc.mats32(c) for s, c in enumerate(fc.round_cameras())}, fc.round_depths(), fc.crafted_frames(3, fc.ROUND_W, fc.ROUND_H, 0x90D)


# ---- premises ---------------------------------------------------------------------------------------------------------------------------
def test_rotated_cameras_have_every_coefficient():
    """rows x, y, w of P and the 14 entries of P^-1 a projective camera can have: all non-zero for each general camera; the axis-parallel one
    keeps its zeros"""
    for size in fc.SIZES:
        mats = _mats(*size)
        for s in fc.VOTING:
            P, Pi, C = mats[s]
            assert all(P[r, c] != 0 for r, c in fc.P_COEFFS) and all(Pi[r, c] != 0 for r, c in fc.PI_COEFFS), (size, s)
            assert all(C[:3] != 0)
        P, Pi, _ = mats[fc.AXIS]
        assert sum(P[r, c] == 0 for r, c in fc.P_COEFFS) == 9 and sum(Pi[r, c] == 0 for r, c in fc.PI_COEFFS) == 8
        rolled = mats[fc.ROLLED][0]
        assert abs(rolled[0, 1]) > abs(rolled[0, 0]) * 1.5   # a roll of 75 degrees: row x is mostly the world's y


@pytest.mark.parametrize("case", fc.FUSE_CASES, ids=[c[0] for c in fc.FUSE_CASES])
def test_fusion_case_premise(case):
    mats = _mats(*case[1])
    res = fc.fuse_expected(case, mats)
    fc.check_fuse_premise(case, res, mats)
    if case[5].get("half"):   # some of AXIS' pixel centres land exactly half way between two of HALF's pixels: the two roundings part there
        st = fc.store(*case[1])
        X = [res["X"][..., a] for a in range(3)]
        P = mats[fc.HALF][0]
        with np.errstate(all="ignore"):
            u = (fm._prow(P, 0, X) / fm._prow(P, 3, X) + f32(1.0)) * (f32(case[1][0]) * f32(0.5)) - f32(0.5)
        assert (np.floor(u + f32(0.5)) != np.rint(u)).sum() >= 3
        assert st["depths"][fc.HALF].shape == u.shape


def test_depth_rule_ties_are_in_the_maps():
    for size in fc.SIZES:
        st = fc.store(*size)
        d, cost = st["depths"][fc.TIES], st["costs"]
        for z in fc.Z_TIES:
            assert ((d == z) | ((d != d) & (z != z))).sum() >= 9
        valid = fm._valid(d, None, np.inf, f32)
        assert valid[0:3, 12:15].all() and valid[0:3, 20:23].all() and not valid[0:3, 4:7].any() and not valid[0:3, 28:31].any()
        for c in cost:
            for v in fc.COST_VALUES:
                assert (c == v).sum() >= 4
            assert (np.signbit(c) & (c == 0)).any()


@pytest.mark.parametrize("size", fc.TSDF_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("G", fc.GRIDS)
def test_rotated_tsdf_premise(G, size):
    """every prefix adds updates; the two lists under a cost threshold add fewer than they would without; votes are fewer than updates; and
    tsdf_mirror's plain integration gives the appearance mirror's TSDF fields"""
    st, mats = fc.store(*size), _mats(*size)
    snaps, vol = fc.tsdf_snapshots(st, mats, G)
    last = 0
    for key in fc.LENGTHS + ["cost", "zero"]:
        total = int(snaps[key][1].sum())
        assert total > last
        last = total
    votes, _ = am.split(vol.cells)
    assert (vol.count > 0).mean() > 0.2 and (votes > 0).mean() > 0.05 and (vol.count > votes).any() and vol.count.max() >= 20
    plain = tm.Volume(G, *fc.cube(G), 4 * fc.cube(G)[1])
    maps = {s: tm.wmap(st["depths"][s], None, mats[s]) for s in range(fc.DEPTH_CAP)}
    plain.integrate(maps, mats, fc.TSDF_LIST)
    assert plain.sum.tobytes() == snaps[19][0].tobytes() and np.array_equal(plain.count, snaps[19][1])
    # max_cost = 0 admits the zeros of either sign and the negative denormal only
    w0 = tm.wmap(st["depths"][0], st["costs"][0], mats[0], f32(0.0))
    c0 = st["costs"][0]
    assert np.array_equal(w0 == w0, (c0 == 0) | (c0 == -fc.TINY)) and 0.3 < (w0 == w0).mean() < 0.5


def test_band_ties_premise():
    """nodes sit on each of the four values of t, for both cameras, and the mirror treats them as rule 4 and rule B say"""
    mats, depths, placed, nodes, frames = _band()
    assert all(n >= 8 for cam in placed for n in cam), placed
    for s in (0, 1):
        vol = fc.integrate_crafted(fc.band_volume(), depths, mats, frames, [s])
        votes, _ = am.split(vol.cells)
        seen = [0, 0, 0, 0]
        for node, k in nodes[s]:
            expect = [(f32(-1.0), 1, 1), (f32(0.0), 0, 0), (f32(1.0), 1, 0), (fc.T_TIES[3], 1, 1)][k]
            assert (vol.sum[node], vol.count[node], votes[node]) == expect, (s, node, k)
            seen[k] += 1
        assert min(seen) >= 8
        assert 0.05 < (vol.count > 0).mean() < 0.5


def test_pixel_rounding_premise():
    mats, depths, frames = _round()
    vol = fc.round_volume()
    W, H = fc.ROUND_W, fc.ROUND_H
    for s in range(3):
        qw, u, v, col, row, hit = fc.project_nodes(vol, mats[s][0], W, H)
        front = qw > 0
        with np.errstate(all="ignore"):
            for name, out in (("left", col < 0), ("right", col >= W), ("top", row < 0), ("bottom", row >= H)):
                assert (front & out).sum() >= 100, (s, name)
            assert hit.sum() >= 1000 and (front & (col == W)).any() and (hit & (col == 0)).any() and (front & (row == H)).any() and (hit & (row == 0)).any()
            if s == 0:   # the camera at the origin: nodes ON the optical axis and ON the seams; the two roundings part at the odd seams
                assert (hit & (u == f32(W / 2 - 0.5)) & (v == f32(H / 2 - 0.5))).any()
                assert (hit & (np.rint(u) != col)).sum() >= 50 and (hit & (np.rint(v) != row)).sum() >= 50
            else:
                assert (~front).sum() >= 10000
            if s == fc.ON_A_NODE:
                assert (qw == 0).any()
    snaps = fc.crafted_snapshots(fc.round_volume(), depths, mats, frames, fc.ROUND_LIST)
    votes, _ = am.split(snaps[19][2])
    assert (snaps[19][1] > 0).sum() >= 3000 and (votes > 0).sum() >= 1000 and snaps[19][1].max() >= 8
    assert all(snaps[a][1].sum() < snaps[b][1].sum() for a, b in zip(fc.LENGTHS, fc.LENGTHS[1:]))


# ---- the mirrors are right on general cameras ---------------------------------------------------------------------------------------------
def _angle(a, b):
    return np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))


def test_fusion_mirror_on_the_analytic_scene():
    """Exact maps at 131 x 67; the rolled camera, the wide one and the one with its own near / far each as the reference against the other
    seven, min_consistent 2.  The float64 path gives the figures; the float32 path is bounded against it.

    Points: a fused point averages back-projections that lie on the primitives up to the stored depth's one rounding (eps / 2 |z|, times
    dw/dz = w^2 (far - near) / (2 far near) < 2 w: at most eps w), so the float64 rows are off a plane by that and inside the ball by a chord's
    sag l^2 / 2r at the most (l the longest tangent).  The float32 rows must lie within 16 eps w of the float64 rows (a back-projection is
    four sums of four terms of the size of w and a division, and dw/dz z / w is about 3) wherever both paths keep the pixel and count the same
    votes, and the keep masks must agree on 99.5 % of the pixels.  Normals: unit, on the camera's side of the surface, within 4 B / l of
    the float64 normal (B the bound on a point, l the shortest tangent); the float64 normals follow the closed form on the planes up to the
    stored depths' roundings (4 eps w / l) and on the ball up to a chord's turn (2 l / r).

    Measured (reference ROLLED / WIDE / DEEP): float64 rows off the planes 2.3e-8 / 3.1e-8 / 2.8e-8 (eps w: 4.3e-7), inside the ball
    5.1e-4 / 6.0e-4 / 7.5e-4 (sag: 2.3e-3 / 3.3e-3 / 2.9e-3); float32 against float64 rows 5.9e-7 / 6.7e-7 / 6.2e-7 (bound 7.1e-6 / 6.8e-6 /
    7.8e-6); keep masks equal; float32 against float64 normals 0.028 / 0.027 / 0.029 degrees (bound 0.095 / 0.077 / 0.11); float64 normals
    against the closed form: planes 6.6e-5 / 6.0e-5 / 6.3e-5 degrees (bound 0.006 / 0.005 / 0.007), ball at most 5.1 / 6.5 / 5.4 degrees at
    the limb (bound 16 / 19 / 17), median 0.18 / 0.28 / 0.16"""
    size = fc.SIZES[0]
    W, H = size
    st = fc.store(*size)
    depths = dict(enumerate(st["depths"]))
    for ref in (fc.ROLLED, fc.WIDE, fc.DEEP):
        nbrs = [s for s in range(fc.NCAM) if s != ref]
        mats64 = {s: fm.slot_matrices(st["cams"][s]) for s in range(fc.NCAM)}
        r32 = fm.fuse(depths, {}, _mats(*size), ref, nbrs, min_consistent=2)
        r64 = fm.fuse(depths, {}, mats64, ref, nbrs, min_consistent=2, dtype=np.float64)
        print("reference %d: keep masks agree on %.5f" % (ref, (r32["keep"] == r64["keep"]).mean()))
        assert (r32["keep"] == r64["keep"]).mean() >= 0.995
        both = r32["keep"] & r64["keep"] & (r32["agree"] == r64["agree"])
        assert both.sum() > 0.5 * W * H
        idx32 = np.cumsum(r32["keep"].ravel()) - 1
        idx64 = np.cumsum(r64["keep"].ravel()) - 1
        p32 = r32["rows"][idx32[both.ravel()]].astype(np.float64)
        p64 = r64["rows"][idx64[both.ravel()]]
        depth = r64["w"][both]
        # the float64 rows against the closed form
        dist, normal, which = fc.scene_distance(p64[:, :3].T)
        flat, ball = which != 2, which == 2
        assert flat.sum() > 1000 and ball.sum() > 50
        X = r64["X"]
        same = lambda a, b: np.abs(r64["w"][a] - r64["w"][b]) / r64["w"][b] <= 0.01   # noqa: E731
        right, below = (slice(None), slice(1, None)), (slice(1, None), slice(None))
        left, above = (slice(None), slice(None, -1)), (slice(None, -1), slice(None))
        lengths = np.concatenate([np.linalg.norm(X[right] - X[left], axis=-1)[same(right, left)], np.linalg.norm(X[below] - X[above], axis=-1)[same(below, above)]])
        sag = lengths.max() ** 2 / (2.0 * fc.BALL.r)   # the agreeing samples lie within a pixel of the reference's, on the ball
        stored = EPS * depth.max()                     # a stored depth's one rounding, eps / 2 |z|, times dw/dz = w^2 (far - near) / (2 far near) < 2 w
        print("reference %d: float64 rows off the planes by %.2g, off the ball by %.2g (a pixel's sag: %.2g)" % (ref, dist[flat].max(), dist[ball].max(), sag))
        assert dist[flat].max() <= stored and dist[ball].max() <= sag + stored
        # the float32 rows against the float64 rows
        B = 16.0 * EPS * depth
        off = np.linalg.norm(p32[:, :3] - p64[:, :3], axis=1)
        print("   float32 rows off the float64 rows by %.2g at the most (bound %.2g)" % (off.max(), B.max()))
        assert np.all(off <= B) and np.all(p32[:, 3] == 1.0)
        # normals
        n32, n64 = p32[:, 4:7], p64[:, 4:7]
        assert np.abs(np.linalg.norm(n32, axis=1) - 1.0).max() <= 4 * EPS
        C = mats64[ref][2][:3]
        assert np.all(((C - p64[:, :3]) * n64).sum(1) > 0) and np.all(((C - p32[:, :3]) * n32).sum(1) > 0)
        bound = np.degrees(4.0 * B.max() / lengths.min())
        ang = _angle(n32, n64)
        print("   float32 normals off the float64 normals by %.2g degrees at the most (bound %.2g)" % (ang.max(), bound))
        assert ang.max() <= bound
        own = fc.scene_distance(X[both].T)   # the reference pixel's own surface point (the normal is the reference map's alone)
        toward = np.where(((C - X[both]) * own[1].T).sum(1, keepdims=True) > 0, own[1].T, -own[1].T)   # the ball's inner side faces the other way
        a64 = _angle(n64, toward)
        # away from the step and the silhouettes: all four neighbours on the pixel's own primitive
        pad = np.pad(fc.scene_distance(X.transpose(2, 0, 1))[2], 1, constant_values=-1)
        inner = ((pad[1:-1, :-2] == pad[1:-1, 1:-1]) & (pad[1:-1, 2:] == pad[1:-1, 1:-1]) & (pad[:-2, 1:-1] == pad[1:-1, 1:-1]) & (pad[2:, 1:-1] == pad[1:-1, 1:-1]))[both]
        on_flat, on_ball = inner & (own[2] != 2), inner & (own[2] == 2)
        print("   float64 normals off the closed form: planes %.2g degrees, ball %.2g (median %.2g)" % (a64[on_flat].max(), a64[on_ball].max(), np.median(a64[on_ball])))
        assert a64[on_flat].max() <= np.degrees(4.0 * stored / lengths.min())
        turn = np.degrees(2.0 * lengths.max() / fc.BALL.r)   # a chord's turn: its length over the radius, twice for two tangents
        print("   (bounds: planes %.2g, ball %.2g degrees)" % (np.degrees(4.0 * stored / lengths.min()), turn))
        assert a64[on_ball].max() <= turn


def test_tsdf_mirror_meshes_the_rotated_maps_onto_the_scene():
    """The exact maps of the rotated set at 131 x 67 (all but CUT, which sees through the occluder and so contradicts the others) into G = 65
    over the cube (h = 0.053, truncation 4 h), meshed at min_observations 1.  tests/test_tsdf_cpu.py's bounds for the height field (median
    0.1 h, 99th percentile 0.5 h) are asserted for the vertices farther than the truncation from the occluder's rim and from the ball, where
    clamped votes from in front of a step meet the ones from behind it.
    Measured: 4599 vertices, 3474 of them away from the rims: median 0.0072 h, 99th percentile 0.043 h; all vertices: median 0.0079 h"""
    size = fc.SIZES[0]
    st, mats = fc.store(*size), _mats(*size)
    G = 65
    origin, h = fc.cube(G)
    maps = {s: tm.wmap(st["depths"][s], None, mats[s]) for s in range(fc.CUT)}   # (CUT sees through the occluder: it contradicts the others)
    vol = tm.Volume(G, origin, h, 4 * h).integrate(maps, mats, range(fc.CUT))
    v, f = vol.surface(1)
    assert len(v) > 2000 and len(f) > 4000
    p = v[:, :3].astype(np.float64).T
    d = fc.scene_distance(p)[0] / float(h)
    tau = 4.0 * float(h)
    rim = (np.abs(np.abs(p[0] - 0.1) - 0.35) < tau) | (np.abs(np.abs(p[1] + 0.05) - 0.3) < tau)
    rim &= (np.abs(p[0] - 0.1) < 0.35 + tau) & (np.abs(p[1] + 0.05) < 0.3 + tau)
    rim |= np.linalg.norm(p - fc.BALL.c[:, None], axis=0) < fc.BALL.r + tau
    far = ~rim
    print("rotated maps, mirror: %d vertices (%d away from the rims): median %.4f h, 99th percentile %.4f h; all: median %.4f h"
          % (len(v), far.sum(), np.median(d[far]), np.percentile(d[far], 99), np.median(d)))
    assert far.sum() > 0.5 * len(v)
    assert np.median(d[far]) <= 0.1 and np.percentile(d[far], 99) <= 0.5


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------
MIRRORS = ("fuse_mirror", "tsdf_mirror", "appearance_mirror")


def _perturbed(subs):
    """copies of the three mirrors, each compiled from its file's text after the substitutions {module: [(old, new)]}; a later copy imports
    the earlier copies.  Every `old` must occur, so a table entry cannot rot away unseen"""
    saved = {n: sys.modules[n] for n in MIRRORS}
    mods = []
    try:
        for name in MIRRORS:
            with open(saved[name].__file__) as fh:
                src = fh.read()
            for old, new in subs.get(name, []):
                assert src.count(old) >= 1, (name, old)
                src = src.replace(old, new)
            mod = types.ModuleType(name)
            mod.__file__ = saved[name].__file__
            sys.modules[name] = mod
            exec(compile(src, mod.__file__, "exec"), mod.__dict__)
            mods.append(mod)
    finally:
        sys.modules.update(saved)
    return mods


FUSE_BY_NAME = {c[0]: c for c in fc.FUSE_CASES}


def _case_bytes(name, mods):
    """the bytes tests/test_fusion_cases_gpu.py compares for a case, from the given copies of the mirrors"""
    fm2, tm2, am2 = mods
    if name in FUSE_BY_NAME:
        case = FUSE_BY_NAME[name]
        res = fc.fuse_expected(case, _mats(*case[1]), mirror=fm2)
        return res["keep"].tobytes() + res["rows"].tobytes()
    size = fc.TSDF_SIZES[1]
    if name in ("tsdf_rotated", "shade_rolled"):
        snaps, vol = fc.tsdf_snapshots(fc.store(*size), _mats(*size), 16, mirror=am2)
        if name == "shade_rolled":
            return am2.shade(vol, _mats(*size)[fc.ROLLED], fc.store(*size)["depths"][fc.ROLLED]).tobytes()
        return b"".join(a.tobytes() for key in snaps for a in snaps[key])
    if name == "tsdf_band":
        mats, depths, _, _, frames = _band()
        vol = fc.integrate_crafted(fc.band_volume(am2), depths, mats, frames, fc.BAND_LIST[:3], mirror=am2)
    else:
        assert name == "tsdf_round", name
        mats, depths, frames = _round()
        vol = fc.integrate_crafted(fc.round_volume(am2), depths, mats, frames, fc.ROUND_LIST[:9], mirror=am2)
    return vol.sum.tobytes() + vol.count.tobytes() + vol.cells.tobytes()


def _both(old, new):
    """the integration's text, which tsdf_mirror and appearance_mirror both state"""
    return {"tsdf_mirror": [(old, new)], "appearance_mirror": [(old, new)]}


UNPROJECT = "((Pi[i, 0] * xn + Pi[i, 1] * yn) + Pi[i, 2] * z) + Pi[i, 3]"
PROW = "((P[i, 0] * X[0] + P[i, 1] * X[1]) + P[i, 2] * X[2]) + P[i, 3]"
NODE = "P[r, 0] * x + ((P[r, 1] * y + P[r, 2] * z) + P[r, 3])"
ROUND_FUSE = "np.floor(u + t(0.5)), np.floor(v + t(0.5))"
ROUND_TSDF = "np.floor(u + f32(0.5)), np.floor(v + f32(0.5))"
VOTE = "a = vj & (sw > t(0.0)) & (d2 <= reproj2) & (rel <= max_rel)"

# (what is wrong, {mirror: [(text, replacement)]}, the case that sees it).  Not in the table, because no input can show them: `w > 0` and
# `qw > 0` against `>=` (at w = 0 the division that follows gives no finite pixel either way), and the order of the sum whose sign decides the
# normal's flip (a depth map holds no surface edge-on to its own rays, so that sum is never within a rounding of zero)
PERTURBATIONS = [
    # summation orders
    ("unproject sums like the node projection", {"fuse_mirror": [(UNPROJECT, "Pi[i, 0] * xn + ((Pi[i, 1] * yn + Pi[i, 2] * z) + Pi[i, 3])")]}, "turn2_all_131x67"),
    ("prow sums like the node projection, in the w-maps", {"fuse_mirror": [(PROW, "P[i, 0] * X[0] + ((P[i, 1] * X[1] + P[i, 2] * X[2]) + P[i, 3])")]}, "tsdf_rotated"),
    ("prow sums like the node projection, in the fusion", {"fuse_mirror": [(PROW, "P[i, 0] * X[0] + ((P[i, 1] * X[1] + P[i, 2] * X[2]) + P[i, 3])")]}, "thresholds_131x67"),
    ("the node projection sums like prow", _both(NODE, "((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3]"), "tsdf_rotated"),
    ("the normal's length sums from the right", {"fuse_mirror": [("(nx * nx + ny * ny) + nz * nz", "nx * nx + (ny * ny + nz * nz)")]}, "turn2_all_131x67"),
    # coefficients: two neighbours swapped in one row, or one dropped
    ("P^-1 row 0: coefficients 1 and 2 swapped", {"fuse_mirror": [(UNPROJECT, "((Pi[i, 0] * xn + Pi[i, 2 if i == 0 else 1] * yn) + Pi[i, 1 if i == 0 else 2] * z) + Pi[i, 3]")]}, "turn1_all_131x67"),
    ("P^-1 row 1: coefficients 0 and 1 swapped", {"fuse_mirror": [(UNPROJECT, "((Pi[i, 1 if i == 1 else 0] * xn + Pi[i, 0 if i == 1 else 1] * yn) + Pi[i, 2] * z) + Pi[i, 3]")]}, "turn3_cost_131x67"),
    ("P^-1 row 2: coefficient 0 dropped", {"fuse_mirror": [(UNPROJECT, "(((0 if i == 2 else Pi[i, 0]) * xn + Pi[i, 1] * yn) + Pi[i, 2] * z) + Pi[i, 3]")]}, "turn5_all_67x45"),
    ("P^-1 row 3: coefficients 2 and 3 swapped", {"fuse_mirror": [(UNPROJECT, "((Pi[i, 0] * xn + Pi[i, 1] * yn) + Pi[i, 3 if i == 3 else 2] * z) + Pi[i, 2 if i == 3 else 3]")]}, "tsdf_rotated"),
    ("P row x: coefficients 1 and 2 swapped, in the fusion", {"fuse_mirror": [(PROW, "((P[i, 0] * X[0] + P[i, 2 if i == 0 else 1] * X[1]) + P[i, 1 if i == 0 else 2] * X[2]) + P[i, 3]")]}, "turn4_all_131x67"),
    ("P row y: coefficient 3 dropped, in the fusion", {"fuse_mirror": [(PROW, "((P[i, 0] * X[0] + P[i, 1] * X[1]) + P[i, 2] * X[2]) + (0 if i == 1 else P[i, 3])")]}, "turn2_all_64x4"),
    ("P row w: coefficients 0 and 1 swapped, in the w-maps", {"fuse_mirror": [(PROW, "((P[i, 1 if i == 3 else 0] * X[0] + P[i, 0 if i == 3 else 1] * X[1]) + P[i, 2] * X[2]) + P[i, 3]")]}, "tsdf_rotated"),
    ("P row x: coefficients 1 and 2 swapped, in the node projection", _both(NODE, "P[r, 0] * x + ((P[r, 2 if r == 0 else 1] * y + P[r, 1 if r == 0 else 2] * z) + P[r, 3])"), "tsdf_rotated"),
    ("P row y: coefficient 0 dropped, in the node projection", _both(NODE, "(0 if r == 1 else P[r, 0]) * x + ((P[r, 1] * y + P[r, 2] * z) + P[r, 3])"), "tsdf_band"),
    ("P row w: coefficients 0 and 1 swapped, in the node projection", _both(NODE, "P[r, 1 if r == 3 else 0] * x + ((P[r, 0 if r == 3 else 1] * y + P[r, 2] * z) + P[r, 3])"), "tsdf_rotated"),
    ("rows y and w exchanged in the integration's arguments", _both("for r in (0, 1, 3)]", "for r in (0, 3, 1)]"), "tsdf_round"),
    # inclusive and exclusive comparisons
    ("z >= -1 is valid", {"fuse_mirror": [("ok = (z > t(-1.0))", "ok = (z >= t(-1.0))")]}, "ties_reference_67x45"),
    ("z >= -1 is valid, in a TSDF slot", {"fuse_mirror": [("ok = (z > t(-1.0))", "ok = (z >= t(-1.0))")]}, "tsdf_rotated"),
    ("z <= 1 is valid", {"fuse_mirror": [("& (z < t(1.0))", "& (z <= t(1.0))")]}, "ties_reference_64x4"),
    ("z <= 1 is valid, in a TSDF slot", {"fuse_mirror": [("& (z < t(1.0))", "& (z <= t(1.0))")]}, "tsdf_rotated"),
    ("cost < max_cost", {"fuse_mirror": [("ok &= cost <= t(max_cost)", "ok &= cost < t(max_cost)")]}, "turn0_cost_64x4"),
    ("cost < max_cost at max_cost = 0", {"fuse_mirror": [("ok &= cost <= t(max_cost)", "ok &= cost < t(max_cost)")]}, "cost_zero_67x45"),
    ("cost < max_cost, in a TSDF slot", {"fuse_mirror": [("ok &= cost <= t(max_cost)", "ok &= cost < t(max_cost)")]}, "tsdf_rotated"),
    ("same surface: < max_rel_depth", {"fuse_mirror": [("/ c[3] <= max_rel)", "/ c[3] < max_rel)")]}, "surface_tie_131x67"),
    ("same surface: < max_rel_depth, one tile", {"fuse_mirror": [("/ c[3] <= max_rel)", "/ c[3] < max_rel)")]}, "surface_tie_64x4"),
    ("du^2 + dv^2 < max_reproj_px^2", {"fuse_mirror": [(VOTE, VOTE.replace("d2 <= reproj2", "d2 < reproj2"))]}, "thresholds_131x67"),
    ("|sw - w| / w < max_rel_depth", {"fuse_mirror": [(VOTE, VOTE.replace("rel <= max_rel", "rel < max_rel"))]}, "thresholds_131x67"),
    ("agree > min_consistent", {"fuse_mirror": [("(agree >= min_consistent)", "(agree > min_consistent)")]}, "thresholds_67x45"),
    ("fc <= W is inside, in the fusion", {"fuse_mirror": [("(fc < t(W))", "(fc <= t(W))")]}, "turn0_all_131x67"),
    ("fr <= H is inside, in the fusion", {"fuse_mirror": [("(fr < t(H))", "(fr <= t(H))")]}, "turn2_cost_131x67"),
    ("fc > 0 is inside, in the fusion", {"fuse_mirror": [("(fc >= t(0.0))", "(fc > t(0.0))")]}, "turn0_all_131x67"),
    ("fc <= W is inside, in the integration", _both("(fc < f32(W))", "(fc <= f32(W))"), "tsdf_round"),
    ("fr > 0 is inside, in the integration", _both("(fr >= f32(0.0))", "(fr > f32(0.0))"), "tsdf_round"),
    ("t > -1 updates", _both("(t >= f32(-1.0))", "(t > f32(-1.0))"), "tsdf_band"),
    ("t >= -1 - 2^-23 updates", _both("(t >= f32(-1.0))", "(t >= f32(-1.0000001))"), "tsdf_band"),
    ("t <= 1 votes", {"appearance_mirror": [("& (t < f32(1.0))", "& (t <= f32(1.0))")]}, "tsdf_band"),
    ("t < 1 - 2^-24 votes", {"appearance_mirror": [("& (t < f32(1.0))", "& (t < f32(0.99999994))")]}, "tsdf_band"),
    # roundings
    ("round half to even, in the fusion", {"fuse_mirror": [(ROUND_FUSE, "np.rint(u), np.rint(v)")]}, "half_pixel_131x67"),
    ("round half to even, in the integration", _both(ROUND_TSDF, "np.rint(u), np.rint(v)"), "tsdf_round"),
    ("the shaded grey truncates", {"appearance_mirror": [("np.floor(value + f32(0.5))", "np.floor(value)")]}, "shade_rolled"),
    # the normal
    ("the one-sided tangents exchanged", {"fuse_mirror": [("np.where(uh, hi[k] - c[k], c[k] - lo[k])", "np.where(uh, c[k] - lo[k], hi[k] - c[k])")]}, "seams_alone_131x67"),
    ("the one-sided tangents exchanged, one tile", {"fuse_mirror": [("np.where(uh, hi[k] - c[k], c[k] - lo[k])", "np.where(uh, c[k] - lo[k], hi[k] - c[k])")]}, "seams_alone_64x4"),
    ("a one-sided tangent where both neighbours are usable", {"fuse_mirror": [("np.where(ul & uh, hi[k] - lo[k],", "np.where(ul & uh & False, hi[k] - lo[k],")]}, "seams_votes_67x45"),
    ("the normal's flip omitted", {"fuse_mirror": [("np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)", "nx, ny, nz")]}, "turn3_all_131x67"),
    ("the normal always flipped", {"fuse_mirror": [("np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)", "-nx, -ny, -nz")]}, "turn6_all_131x67"),
]


@functools.lru_cache(maxsize=None)
def _true_bytes(name):
    return _case_bytes(name, (fm, tm, am))


@pytest.mark.parametrize("what,subs,case", PERTURBATIONS, ids=[p[0] for p in PERTURBATIONS])
def test_a_wrong_mirror_changes_a_case(what, subs, case):
    """a mirror that is wrong in this way expects other bytes of the named case (or leaves the image or the volume: an index error)"""
    try:
        wrong = _case_bytes(case, _perturbed(subs))
    except IndexError:
        return
    assert wrong != _true_bytes(case), "%s: no byte of %s changes" % (what, case)


def test_the_copies_are_the_mirrors():
    """without a substitution the copies give the mirrors' bytes"""
    for case in ("turn2_all_64x4", "tsdf_band"):
        assert _case_bytes(case, _perturbed({})) == _true_bytes(case)
