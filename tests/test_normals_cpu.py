"""DESIGN.md section 31 on the mirror (tests/normals_mirror.py): rule N1 against the analytic normals of planes seen by general cameras, the
float32 path against the float64 path, the clauses no device input reaches, the crafted fusion cases' premises and identities, the table of
one-line errors that each change a named case's bytes, and what the slope normals buy on section 25's exposure scene (measured)."""
import functools
import types

import numpy as np
import pytest

import fuse_mirror as fm
import fuse_sequence_mirror as sm
import fusion_cases as fc
import normals_cases as nc
import normals_mirror as nm
from mvs_amd import synth

f32 = np.float32
PLANES = (("BACK", fc.BACK), ("FLOOR", fc.FLOOR[0]))

# Rule N1's float64 path against the analytic normal.  The inputs carry relative errors of a few eps = 2^-53 (the inverse of a matrix of
# condition below 50, the slopes' quotients); every step of N1 adds a few eps relative to |m|, and m's entries come from sums without
# cancellation beyond a factor |z| + |a| + |b| + |d| < 10 over |m| > 0.1: an angle below 1e3 eps ~ 1e-13.  1e-9 leaves four decades.
N1_F64_BOUND = 1e-9
# The float32 path against the float64 path over the 54 (size, camera, plane) cases below: the largest angle measured is 5.81e-8 rad (the
# rolled camera, BACK, 131 x 67) and no pixel's flip differs; asserted with a margin of 2 x.  It bounds the mirror, not the device: the
# device equals the float32 path bit for bit.
N1_F32_MEASURED, N1_F32_FLIPS_MEASURED = 5.81e-8, 0


def _mats(W, H):
    return {s: fc.mats32(c) for s, c in enumerate(fc.store(W, H)["cams"])}


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arcsin(np.clip(np.linalg.norm(np.cross(a, b), axis=-1), 0.0, 1.0)), (a * b).sum(-1)


def reversed_depth_camera(W, H):
    """NDC depth falls with the distance (near and far exchanged): the one kind of camera for which rule N1's flip is not taken"""
    return np.ascontiguousarray(fc.looking(W, H, -4.0, 7.0, 40.0, near=synth.FAR, far=synth.NEAR), f32)


def _raw_m(z, gx, gy, P, W, H):
    """rule N1's m of pixel (0, 0) in float64, before the flip"""
    xn, yn = 1.0 / W - 1.0, 1.0 - 1.0 / H
    a, b = -gx[0, 0] * (W * 0.5), gy[0, 0] * (H * 0.5)
    return np.array([a, b, 1.0, -((z[0, 0] + a * xn) + b * yn)]) @ P


# ---- rule N1 ------------------------------------------------------------------------------------------------------------------------------------
def test_rule_n1_returns_the_planes_normal_on_the_cameras_side():
    worst64, worst32, flips, total, flipped = 0.0, 0.0, 0, 0, {}
    for W, H in fc.SIZES:
        for ci, cam in enumerate(fc.cameras(W, H) + [reversed_depth_camera(W, H)]):
            P, _, C = fm.slot_matrices(cam)
            for pname, plane in PLANES:
                z, gx, gy = nc.plane_hypotheses(cam, W, H, plane)
                ok = (z > -1.0) & (z < 1.0)
                assert ok.sum() > 100, (W, H, ci, pname)
                n64 = nm.hypothesis_normals(z, gx, gy, P, C, np.float64)
                want = np.sign(plane.n @ C[:3] - plane.d) * plane.n
                angle, dot = _angle(n64[ok], want)
                assert (dot > 0).all() and angle.max() <= N1_F64_BOUND, (W, H, ci, pname, angle.max())
                assert not n64[~ok].any()
                worst64 = max(worst64, angle.max())
                flipped[ci] = bool(_raw_m(z, gx, gy, P, W, H)[:3] @ want < 0)   # was the flip taken?
                n32 = nm.hypothesis_normals(z.astype(f32), gx.astype(f32), gy.astype(f32), np.asarray(P, f32), np.asarray(C, f32))
                assert n32.dtype == f32 and nm.usable(n32[ok]).all() and not n32[~ok].any()
                a32, d32 = _angle(n32[ok], n64[ok])
                worst32 = max(worst32, a32.max())
                flips += int((d32 < 0).sum())
                total += int(ok.sum())
    print("rule N1, float64 path against the analytic normal: %.3g rad; float32 against float64: %.3g rad, %d of %d flips differ" % (worst64, worst32, flips, total))
    assert worst32 <= 2.0 * N1_F32_MEASURED and flips <= 2 * N1_F32_FLIPS_MEASURED
    # m . (C, 1) is P's z row at the centre whatever the slopes are (rows x and y vanish there): negative for every camera whose NDC depth
    # grows with the distance, the mirrored one included -- rule N1 does not depend on the image's handedness as rule 5's cross product
    # does.  The camera with near and far exchanged takes the other branch
    assert all(flipped[ci] for ci in range(fc.NCAM)) and not flipped[fc.NCAM], flipped


def _one(z, gx, gy, P, C, t=f32):
    return nm.hypothesis_normals(np.full((1, 1), z, t), np.full((1, 1), gx, t), np.full((1, 1), gy, t), P, C, t)[0, 0]


def test_clauses_the_device_entry_cannot_reach():
    """a camera whose centre lies ON a pixel's plane, a length that overflows, NaN slopes, and each of Z_TIES as z"""
    W = H = 1   # the one pixel's centre is (0, 0)
    P = np.eye(4, dtype=f32)
    # m = (0, 0, 1, -z): m . (C, 1) = C_z - z.  C ON the plane: no flip (the test is `< 0`); on either side of it: the two signs
    assert _one(0.25, 0.0, 0.0, P, (0.0, 0.0, 0.25)).tolist() == [0.0, 0.0, 1.0]
    assert _one(0.25, 0.0, 0.0, P, (0.0, 0.0, 0.5)).tolist() == [0.0, 0.0, 1.0]
    assert _one(0.25, 0.0, 0.0, P, (0.0, 0.0, 0.0)).tolist() == [-0.0, -0.0, -1.0]
    # slopes whose squares overflow: an infinite length gives zeros; just below, a unit normal
    big = f32(6e19)   # a = -big / 2: its square is above the largest float32
    assert _one(0.0, big, 0.0, P, (0, 0, 0)).tolist() == [0.0, 0.0, 0.0]
    assert nm.usable(_one(0.0, f32(1e18), 0.0, P, (0, 0, 9)))
    for gx, gy in ((np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (np.inf, -np.inf)):
        assert _one(0.0, gx, gy, P, (0, 0, 0)).tolist() == [0.0, 0.0, 0.0], (gx, gy)
    # a singular "camera" with no plane left: length 0
    assert _one(0.0, 0.0, 0.0, np.zeros((4, 4), f32), (0, 0, 0)).tolist() == [0.0, 0.0, 0.0]
    for k, z in enumerate(fc.Z_TIES):
        n = _one(z, 0.01, -0.02, fc.cameras(8, 8)[fc.ROLLED], fc.mats32(fc.cameras(8, 8)[fc.ROLLED])[2])
        assert bool(nm.usable(n)) == (k in (1, 2)) and (k in (1, 2) or n.tolist() == [0.0, 0.0, 0.0]), (k, z, n)


def test_usable_is_open_at_both_bounds():
    n = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, -1.0], [0.0, 0.0, 0.0], [np.nan, 0, 1], [0, np.inf, 0], [0.6, 0.0, 0.8], [0.5, 0.5, 0.001], [1.0, 0.0, -0.999]], f32)
    assert nm.usable(n).tolist() == [False, False, False, False, False, True, True, True]


# ---- the fusion cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nc.CASES, ids=[c[0] for c in nc.CASES])
def test_case_holds_what_it_is_for(case):
    nc.check_premise(case, _mats(*case[1]))


@pytest.mark.parametrize("case", nc.CASES, ids=[c[0] for c in nc.CASES])
def test_identities(case):
    """no plane and no test: mvs_fuse_depth_masked's bytes; planes of zeros: the same; with min_support = 0 as well: mvs_fuse_depth's"""
    name, size, ref, nbrs, kinds, kw, _, _ = case
    mats = _mats(*size)
    d, c, s, n = nc.case_inputs(case)
    plain = dict(kw)
    min_support = plain.pop("min_support", 0)
    masked = sm.fuse_masked(d, c, s, mats, ref, nbrs, min_support=min_support, **plain)
    zeros = {slot: np.zeros(size[::-1] + (3,), f32) for slot in kinds}
    for planes, cos in (({}, nc.NO_TEST), (zeros, nc.NO_TEST), (zeros, 0.5), ({}, 1.0)):
        res = nc.expected(case, mats, min_normal_cos=cos, normals=planes)
        assert res["keep"].tobytes() == masked["keep"].tobytes() and res["rows"].tobytes() == masked["rows"].tobytes(), (name, cos)
    plainest = fm.fuse(d, c, mats, ref, list(nbrs), **plain)
    res = nc.expected(case, mats, min_normal_cos=nc.NO_TEST, normals={}, min_support=0)
    assert res["rows"].tobytes() == plainest["rows"].tobytes() and res["keep"].tobytes() == plainest["keep"].tobytes(), name
    assert nc.expected(case, mats)["rows"].tobytes() != masked["rows"].tobytes(), (name, "the planes change nothing")


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------------------
def _perturbed(subs):
    """a copy of the mirror compiled from its file's text after the substitutions [(old, new)]; every `old` must occur"""
    with open(nm.__file__) as fh:
        src = fh.read()
    for old, new in subs:
        assert src.count(old) >= 1, old
        src = src.replace(old, new)
    mod = types.ModuleType("normals_mirror")
    mod.__file__ = nm.__file__
    exec(compile(src, mod.__file__, "exec"), mod.__dict__)
    return mod


def n1_inputs(name):
    """rule N1's own cases: the store's map of a camera with the scene's slopes, perturbed -> (z, gx, gy, P, C)"""
    slot = {"n1_rolled": fc.ROLLED, "n1_mirrored": fc.MIRRORED, "n1_ties": fc.TIES}[name]
    W, H = fc.SIZES[2]
    st = fc.store(W, H)
    gx, gy = (np.nan_to_num(g, nan=0.01) for g in nc.surface_slopes(st["cams"][slot], st["depths"][slot]))   # (finite beside the z ties)
    rng = np.random.Generator(np.random.PCG64(31 + slot))
    P, _, C = fc.mats32(st["cams"][slot])
    return st["depths"][slot], (gx * (1.0 + 0.3 * rng.random((H, W)))).astype(f32), (gy * (1.0 - 0.3 * rng.random((H, W)))).astype(f32), P, C


def _case_bytes(name, mod):
    if name.startswith("n1_"):
        return mod.hypothesis_normals(*n1_inputs(name)).tobytes()
    case = nc.BY_NAME[name]
    res = nc.expected(case, _mats(*case[1]), mirror=mod)
    return res["keep"].tobytes() + res["rows"].tobytes()


M_K = "((a * P[0, k] + b * P[1, k]) + P[2, k]) + d * P[3, k]"
PERTURBATIONS = [
    ("a and b exchanged", [(M_K, "((b * P[0, k] + a * P[1, k]) + P[2, k]) + d * P[3, k]")], "n1_rolled"),
    ("b's sign", [("b = gy * halfH", "b = -gy * halfH")], "n1_rolled"),
    ("a's sign", [("a = -gx * halfW", "a = gx * halfW")], "n1_mirrored"),
    ("d P[3][k] dropped", [(M_K, "((a * P[0, k] + b * P[1, k]) + P[2, k])")], "n1_rolled"),
    ("the sum order of m_k", [(M_K, "(a * P[0, k] + (b * P[1, k] + P[2, k])) + d * P[3, k]")], "n1_rolled"),
    ("the sum order of d", [("d = -((z + a * xn) + b * yn)", "d = -(z + (a * xn + b * yn))")], "n1_rolled"),
    ("the length sums from the right", [("ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])", "ln = np.sqrt(m[0] * m[0] + (m[1] * m[1] + m[2] * m[2]))")], "n1_rolled"),
    ("rule N1's flip omitted", [("n = [np.where(flip, -v, v) for v in n]", "n = list(n)")], "n1_rolled"),
    ("rule N1's flip inverted, mirrored camera", [("n = [np.where(flip, -v, v) for v in n]", "n = [np.where(flip, v, -v) for v in n]")], "n1_mirrored"),
    ("the side test leaves m3 out", [("+ m[2] * C[2]) + m[3] < t(0.0)", "+ m[2] * C[2]) < t(0.0)")], "n1_rolled"),
    ("z = -1 holds a hypothesis", [("ok = (z > t(-1.0)) & (z < t(1.0)) & (ln", "ok = (z >= t(-1.0)) & (z < t(1.0)) & (ln")], "n1_ties"),
    ("z = 1 holds a hypothesis", [("ok = (z > t(-1.0)) & (z < t(1.0)) & (ln", "ok = (z > t(-1.0)) & (z <= t(1.0)) & (ln")], "n1_ties"),
    ("> for >= in rule 3n", [("(dot >= min_cos)", "(dot > min_cos)")], "cos_mid_131x67"),
    ("> for >= in rule 3n, odd size", [("(dot >= min_cos)", "(dot > min_cos)")], "cos_mid_67x45"),
    ("a voter's normal added before its test", [("add = a & both", "add = rule3 & both")], "cos_mid_67x45"),
    ("a voter's normal added though the reference has none", [("both = ur & usable(nj, t)", "both = usable(nj, t)")], "holes_131x67"),
    ("the test applied to a voter without a usable normal", [("a = rule3 & (~both | (dot >= min_cos))", "a = rule3 & (dot >= min_cos)")], "holes_67x45"),
    ("the voter's normal read at the reference's pixel", [("nj = np.asarray(normals[j], t)[rj, cj]", "nj = np.asarray(normals[j], t)")], "cos_mid_67x45"),
    ("rule 5n's flip omitted", [("snx, sny, snz = toward_camera(ax / la, ay / la, az / la)", "snx, sny, snz = ax / la, ay / la, az / la")], "away_67x45"),
    ("rule 5n's length sums from the right", [("la = np.sqrt((ax * ax + ay * ay) + az * az)", "la = np.sqrt(ax * ax + (ay * ay + az * az))")], "cos_mid_131x67"),
    ("the tangent rule applied beside a usable normal", [("has_normal = ok & np.where(ur, summed_ok, tangent_ok)", "has_normal = ok & np.where(ur, summed_ok, tangent_ok) & tangent_ok")], "keepset_alone_64x4"),
    ("zeros treated as usable", [("(s > t(0.5))", "(s >= t(0.0))")], "holes_131x67"),
    ("a squared length of 0.5 is usable", [("(s > t(0.5))", "(s >= t(0.5))")], "holes_67x45"),
    ("a squared length of 2 is usable", [("(s < t(2.0))", "(s <= t(2.0))")], "holes_131x67"),
    ("rule 1s left out", [("depths = sm.masked(depths, supports, min_support)", "depths = dict(depths)")], "support_64x4"),
]


@functools.lru_cache(maxsize=None)
def _true_bytes(name):
    return _case_bytes(name, nm)


@pytest.mark.parametrize("what,subs,case", PERTURBATIONS, ids=[p[0] for p in PERTURBATIONS])
def test_a_wrong_mirror_changes_a_case(what, subs, case):
    """a mirror that is wrong in this way expects other bytes of the named case (or leaves the image: an index error)"""
    try:
        wrong = _case_bytes(case, _perturbed(subs))
    except IndexError:
        return
    assert wrong != _true_bytes(case), "%s: no byte of %s changes" % (what, case)


def test_the_copy_is_the_mirror():
    for case in ("n1_rolled", "cos_mid_64x4"):
        assert _case_bytes(case, _perturbed([])) == _true_bytes(case)


# ---- what it buys ---------------------------------------------------------------------------------------------------------------------------------
def scene_normal(X):
    """unit normal of synth.Scene's height field z = h(x, y) at the points X [N, 3]: (-h_x, -h_y, 1) normalised"""
    x, y = X[:, 0].astype(np.float64), X[:, 1].astype(np.float64)
    hx = -0.4 * 1.3 * np.cos(1.3 * x + 0.7) * np.cos(1.1 * y - 0.2)
    hy = 0.4 * 1.1 * np.sin(1.3 * x + 0.7) * np.sin(1.1 * y - 0.2)
    n = np.stack([-hx, -hy, np.ones_like(hx)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def test_slope_normals_against_tangent_normals_on_the_exposure_scene(oracle):
    """section 25's exposure scene at 96 x 64, 16 planes refined and section 25's recipe (3 iterations, 3 random candidates, ZNCC r = 3)
    through the propagation's mirror; the main view fused alone.  Measured: rule 5's tangent normals median
    20.22 deg, 90th percentile 39.13 deg, 5724 rows; rule N1's slope normals through rule 5n 16.92 deg, 28.24 deg, 6144 rows.  Only the
    direction is asserted: 29 % of the pixels still hold the zero slopes they started with, and both figures are far from the 0.006 deg of
    the tangent rule on the analytic map."""
    import propagate_cases as pc
    import propagate_mirror as pm
    W, H = 96, 64
    views, truth, start = pc.exposure_start(W, H)
    coarse = 2.0 / 16
    state = pm.State(pm.Scene(oracle, *views), start, pc.ZNCC, 3, pc.KEEP_ALL).run(3, 0.5 * coarse, 0.125 * coarse, 3, 0)
    mats = {0: fc.mats32(views[0])}
    depths = {0: np.asarray(state.z, f32)}
    normals = {0: nm.hypothesis_normals(state.z, state.gx, state.gy, mats[0][0], mats[0][2])}

    def figures(rows):
        cos = np.abs((rows[:, 4:7].astype(np.float64) * scene_normal(rows[:, :3])).sum(-1))
        angle = np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))
        return float(np.median(angle)), float(np.percentile(angle, 90)), len(rows)

    old = figures(sm.fuse_masked(depths, {}, {}, mats, 0, [], min_consistent=0)["rows"])
    new = figures(nm.fuse_normals(depths, {}, {}, normals, mats, 0, [], min_consistent=0)["rows"])
    print("exposure scene %d x %d, angle to the analytic normal: tangent normals median %.2f deg, p90 %.2f deg, %d rows; slope normals median %.2f deg, p90 %.2f deg, %d rows; "
          "zero slopes at %.0f %% of the pixels" % ((W, H) + old + new + (100.0 * float((np.asarray(state.gx) == 0).mean()),)))
    assert new[0] < old[0] and new[1] < old[1] and new[2] >= old[2]
