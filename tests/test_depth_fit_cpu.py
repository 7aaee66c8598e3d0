"""DESIGN.md section 32 on the mirror (tests/depth_fit_mirror.py): the array path against the pixel-at-a-time path on the crafted maps, what
each crafted case is for, the table of one-line errors that each change a named case's bytes, the float64 path on exact affine maps
against a bound worked out below, the float32 path against the float64 path and numpy's least squares, and the direction of what the fit
buys: against the propagation's central differences on degraded maps of a smooth scene, and of the depth gate beside a depth step."""
import functools
import types

import numpy as np
import pytest

import depth_fit_cases as fc
import depth_fit_mirror as fm
import propagate_mirror as pm
from mvs_amd import synth

f32 = np.float32
INF = float("inf")
EPS = 2.0 ** -53
# The float32 path against the float64 path on random member masks of the +- 1/2-step map (test_float32_path_...): the worst differences
# of the rule's prototype on slopes of about 4e-3, asserted with a margin of 4 x because the masks are random and the worst case is a
# tail (this module's masks give 1.19e-8 and 3.57e-8).  They bound the mirror, not the device: the device equals the float32 path bit for bit.
F32_SLOPE_MEASURED, F32_C_MEASURED = 2.2e-8, 3.1e-8


def _pixels(shape):
    """every pixel of a small map; of a larger one the two outer rings, the tile seams' neighbours and every fifth pixel"""
    H, W = shape
    rows, cols = np.mgrid[0:H, 0:W]
    if H * W <= 200:
        keep = np.ones(shape, bool)
    else:
        keep = (rows < 2) | (rows >= H - 2) | (cols < 2) | (cols >= W - 2) | ((rows + 3 * cols) % 5 == 0)
        keep |= (np.abs(cols - 31.5) < 2) | (np.abs(rows - 7.5) < 2)
    return np.argwhere(keep)


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c.name)
def test_the_two_statements_agree(case):
    ref = fc.reference(case)
    for row, col in _pixels(case.depth.shape):
        got = fm.brute_pixel(case.depth, row, col, case.radius, case.tau, case.max_step, case.min_members, case.guide)
        want = tuple(a[row, col] for a in ref[:5])
        for g, w, name in zip(got[:4], want[:4], ("z", "gx", "gy", "zfit")):
            assert f32(g).view(np.uint32) == f32(w).view(np.uint32), "%s: %s at (%d, %d): %r, the array path has %r" % (case.name, name, row, col, g, w)
        assert got[4] == want[4], "%s: members at (%d, %d)" % (case.name, row, col)


def test_cases_hold_what_they_are_for():
    ref = lambda name: fc.reference(fc.by_name(name))
    sizes = {c.depth.shape[::-1] for c in fc.cases()}
    assert {(9, 5), (32, 8), (33, 8), (31, 8), (32, 9), (32, 7), (64, 16)} <= sizes
    for r in fc.RADII:                                          # borders and corners are fitted from asymmetric windows
        res = ref("plain_r%d" % r)
        assert all((edge > 0).any() for edge in (res.members[0], res.members[-1], res.members[:, 0], res.members[:, -1])) and res.report[1] > 300
        assert (ref("gated_r%d" % r).members != res.members).any()
    for name in ("collinear_row", "collinear_column", "collinear_diagonal"):
        res = ref(name)
        assert res.report == [117, 0, 0 if name != "collinear_diagonal" else res.report[2], res.report[3]] and res.report[3] >= 100, (name, res.report)
        assert (res.D == 0).all() and not res.gx.any() and not res.members.any()
    full = ref("full_r4")
    assert (full.D == fc.FULL_D).sum() == (19 - 8) * (13 - 8) == full.report[1] and full.report[2] == 19 * 13 - full.report[1]
    assert (full.members == 81).sum() == full.report[1] and ref("full_r4_min80").report[1] == full.report[1]
    D = np.concatenate([ref(n).D.ravel() for n in ("plain_r4", "full_r4_min80", "seams_no_gate")])
    assert ((D > 2 ** 24) & (D.astype(f32).astype(np.int64) != D)).any(), "no D of these cases needs the rounded conversion"
    for k in (3, 6, 9):
        hit, miss = ref("count_%d_of_%d" % (k, k)), ref("count_%d_of_%d" % (k, k + 1))
        assert hit.members[4, 4] == k and miss.members[4, 4] == 0 and miss.report[2] >= 1 and miss.gx[4, 4] == 0
    on, tau_below, step_below = ref("gate_on"), ref("gate_tau_below"), ref("gate_step_below")
    assert on.members[5, 5] == 6 and tau_below.members[5, 5] == 4 and step_below.members[5, 5] == 5
    assert ref("gate_step0").members[5, 5] == 0 and ref("gate_step_inf").members[5, 5] > ref("gate_tau0").members[5, 5]
    for name, sign in (("range_above", 1.0), ("range_below", -1.0)):
        res = ref(name)
        assert res.members[0, 0] == 4 and res.c[0, 0] == f32(sign * 0.5) and res.z[0, 0] == f32(sign * 0.5) and res.zfit[0, 0] == res.z[0, 0]
    for name, sign in (("range_line_above", 1.0), ("range_line_below", -1.0)):
        res = ref(name)
        assert (res.members > 0).all() and (sign * (res.z[:, 0] + res.c[:, 0]) > 1.1).all() and (res.zfit[:, 0] == res.z[:, 0]).all()
        assert (res.zfit[:, 1:] != res.z[:, 1:]).all()
    assert ref("all_invalid").report == [0, 0, 0, 0] and ref("one_valid").report == [1, 0, 1, 0]
    vals = ref("values_r1")
    assert vals.z[1, 0].view(np.uint32) == 0 and np.signbit(fc.by_name("values_r1").depth[1, 0])   # -0.0 is read as +0.0


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------
def _perturbed(subs):
    """a copy of the mirror compiled from its file's text after the substitutions [(old, new)]; every `old` must occur"""
    with open(fm.__file__) as fh:
        src = fh.read()
    for old, new in subs:
        assert src.count(old) >= 1, old
        src = src.replace(old, new)
    mod = types.ModuleType("depth_fit_mirror")
    mod.__file__ = fm.__file__
    exec(compile(src, mod.__file__, "exec"), mod.__dict__)
    return mod


def _case_bytes(name, mod):
    res = fc.run(fc.by_name(name), mod)
    return b"".join(a.tobytes() for a in res[:5]) + repr(res.report).encode()


C_SUM = "c = ((A00 * St + A01 * Sxt) + A02 * Syt) / Df"
PERTURBATIONS = [
    ("dc and dr exchanged", [("Sxt + t_(dc) * t", "Sxt + t_(dr) * t"), ("Syt + t_(dr) * t", "Syt + t_(dc) * t")], "plain_r2"),
    ("dc and dr exchanged in the moments", [("Sx += m * dc", "Sx += m * dr"), ("Sy += m * dr", "Sy += m * dc")], "size_9x5"),
    ("a cofactor's sign", [("A01 = Sy * Sxy - Sx * Syy", "A01 = Sx * Syy - Sy * Sxy")], "plain_r2"),
    ("another cofactor's sign", [("A12 = Sx * Sy - n * Sxy", "A12 = n * Sxy - Sx * Sy")], "plain_r3"),
    ("D without the Sy A02 term", [("D = n * A00 + Sx * A01 + Sy * A02", "D = n * A00 + Sx * A01")], "size_31x8"),
    ("> for >= at min_members", [("fitted = ok & (n >= min_members)", "fitted = ok & (n > min_members)")], "count_3_of_3"),
    ("> for >= at min_members, a full window", [("fitted = ok & (n >= min_members)", "fitted = ok & (n > min_members)")], "full_r4"),
    ("< for <= at max_step", [("(np.abs(gate_t) <= step)", "(np.abs(gate_t) < step)")], "gate_on"),
    ("the depth gate left out", [("& (np.abs(gate_t) <= step)", "")], "gate_step_below"),
    ("collinear members fitted", [("& (D != 0)\n", "\n")], "collinear_diagonal"),
    ("the sum order of c", [(C_SUM, "c = (A00 * St + (A01 * Sxt + A02 * Syt)) / Df")], "plain_r4"),
    ("the sum order of gx", [("gx = ((A01 * St + A11 * Sxt) + A12 * Syt) / Df", "gx = (A01 * St + (A11 * Sxt + A12 * Syt)) / Df")], "plain_r4"),
    ("the window walked backwards", [("for dr, dc in offsets(radius):", "for dr, dc in reversed(offsets(radius)):")], "plain_r4"),
    ("the window walked column by column", [("for dr, dc in offsets(radius):", "for dc, dr in offsets(radius):")], "plain_r3"),
    ("t not differenced against the centre", [("t = gate_t if t_ is f32 else", "t = q if t_ is f32 else")], "plain_r3"),
    ("the products not rounded before they are added", [("Sxt + t_(dc) * t, Sxt).astype(t_)", "(Sxt.astype(np.float64) + np.float64(dc) * t.astype(np.float64)).astype(t_), Sxt).astype(t_)")], "plain_r4"),
    ("-0.0 not read as +0.0", [("z = np.where(ok, vt, BACKGROUND_DEPTH)", "z = np.where(ok, np.asarray(depth, t_), BACKGROUND_DEPTH)")], "values_r1"),
    ("members written for pixels that are not fitted", [("members = np.where(fitted, n, 0)", "members = n")], "count_3_of_4"),
    ("slopes written for pixels that are not fitted", [("gx = np.where(fitted, gx, t_(0.0))", "gx = np.where(ok, gx, t_(0.0))")], "count_6_of_7"),
    ("zfit not range-checked", [("fitted & (moved > t_(-1.0)) & (moved < t_(1.0))", "fitted")], "range_line_above"),
    ("zfit not range-checked below", [("fitted & (moved > t_(-1.0)) & (moved < t_(1.0))", "fitted & (moved < t_(1.0))")], "range_line_below"),
    ("zfit = 1 admitted", [("(moved < t_(1.0))", "(moved <= t_(1.0))")], "range_above"),
    ("zfit = -1 admitted", [("(moved > t_(-1.0))", "(moved >= t_(-1.0))")], "range_below"),
    ("the report's refusals exchanged", [("int((ok & (n < min_members)).sum()), int((ok & (n >= min_members) & (D == 0)).sum())",
                                         "int((ok & (n >= min_members) & (D == 0)).sum()), int((ok & (n < min_members)).sum())")], "collinear_row"),
]


@functools.lru_cache(maxsize=None)
def _true_bytes(name):
    return _case_bytes(name, fm)


@pytest.mark.parametrize("what,subs,case", PERTURBATIONS, ids=[p[0] for p in PERTURBATIONS])
def test_a_wrong_mirror_changes_a_case(what, subs, case):
    """a mirror that is wrong in this way expects other bytes of the named case (or trips the mirror's own range assertion)"""
    try:
        wrong = _case_bytes(case, _perturbed(subs))
    except AssertionError:
        return
    assert wrong != _true_bytes(case), "%s: no byte of %s changes" % (what, case)


def test_the_copy_is_the_mirror_and_the_guide_gate_decides_its_cases():
    for case in ("plain_r2", "gate_on"):
        assert _case_bytes(case, _perturbed([])) == _true_bytes(case)
    assert _true_bytes("gate_on") != _true_bytes("gate_tau_below")      # the guide difference at tau and at tau + 1 (section 23's rule 2)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def _punched(z, share, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.where(rng.random(z.shape) < share, z, np.nan)


@pytest.mark.parametrize("radius", fc.RADII)
def test_float64_path_returns_an_exact_affine_map(radius):
    """z = z0 + a col + b row evaluated in float64, under random member masks (holes), borders included: every fitted pixel gets (a, b)
    and c = 0 up to the bound below.
    The bound, per pixel.  The map's values carry one rounding each, |z| < 1: every t = z(q) - z(p) is off the affine value by at most
    2 eps, eps = 2^-53.  St, Sxt, Syt are sums of n <= 81 products |d t| <= 4 T (T = the largest |t| of the window), each product and
    each partial sum rounded once: their error is below n (n 4 T + 4 * 2) eps, the data's error included.  With exact data the normal
    equations return (0, a, b) exactly; the three errors enter c, gx, gy through one row of the adjugate each, |Aij| <= 291 600, three
    products and two sums of magnitudes below 3 * 291 600 * n * 4 T, rounded once each, and one division by D: in all
    |error| <= 3 * 291 600 * (n (4 n T + 8) + 5 * 4 n T) eps / D, and a factor 2 for the second-order terms."""
    W, H, z0, a, b = 41, 23, -0.31, 0.0043, -0.0027
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    exact = z0 + a * cols + b * rows
    worst = 0.0
    for share in (1.0, 0.6, 0.25, 0.1):
        z = _punched(exact, share, 320 + radius)
        res = fm.fit(z, radius, 255, INF, 3, None, np.float64)
        fitted = res.members > 0
        assert fitted.sum() > 5, (share, fitted.sum())
        n, T = res.members.astype(np.float64), 4.0 * (abs(a) + abs(b)) * 2
        bound = 2 * 3 * 291600 * (n * (4 * n * T + 8) + 20 * n * T) * EPS / np.maximum(res.D, 1)
        for got, want, name in ((res.gx, a, "gx"), (res.gy, b, "gy"), (res.c, 0.0, "c")):
            err = np.abs(got - want)[fitted]
            assert (err <= bound[fitted]).all(), "%s, share %g: error %.3g against the bound %.3g" % (name, share, err.max(), bound[fitted][np.argmax(err)])
            worst = max(worst, err.max())
    print("radius %d: the float64 path is within %.3g of the affine map's slopes and c = 0" % (radius, worst))
    assert worst < 1e-12


@functools.lru_cache(maxsize=None)
def _smooth_maps():
    """synth.make_views(96, 64, 4)'s exact depth, and the degraded maps of DESIGN.md section 32: rounded to the steps of a 48-plane table,
    and with uniform noise of +- 1/2 and +- 1/4 step"""
    W, H = 96, 64
    truth = np.asarray(synth.make_views(W, H, 4)[4], np.float64)
    step = 2.0 / 48
    rng = np.random.Generator(np.random.PCG64(3200))
    noise = rng.uniform(-0.5, 0.5, (H, W))
    return truth, {"rounded": (np.round((truth + 1.0) / step) * step - 1.0).astype(f32), "half": (truth + step * noise).astype(f32),
                   "quarter": (truth + 0.5 * step * noise).astype(f32)}


def test_float32_path_against_the_float64_path_and_least_squares():
    """random member masks (holes) of the +- 1/2-step map, every radius, member shares 1.0 / 0.6 / 0.25 / 0.1, frame borders included.
    The bound is asserted at min_members = 6, the call's default; measured there: slopes 1.19e-8, c 3.57e-8.  At min_members = 3 the worst
    pixels are planes through exactly three noisy pixels (D = 1): their slopes are up to 0.10, 25 times the surface's 4e-3 the bound is
    stated for, the rounding of t = z(q) - z(p) and of the sums scales with them, and the worst slope difference measured is 9.3e-8 (c
    3.57e-8).  The slope figure at 3 is printed with its size relative to the slope; the bound on c holds there too and is asserted."""
    z = _smooth_maps()[1]["half"]
    worst_lstsq, checked, worst = 0.0, 0, {}
    for min_members in (6, 3):
        worst_slope = worst_c = worst_rel = 0.0
        for radius in fc.RADII:
            for share in (1.0, 0.6, 0.25, 0.1):
                zm = _punched(z, share, 3210 + 10 * radius + int(10 * share)).astype(f32)
                a, b = fm.fit(zm, radius, 255, INF, min_members, None, f32), fm.fit(zm, radius, 255, INF, min_members, None, np.float64)
                fitted = a.members > 0
                assert (a.members == b.members).all()
                if not fitted.any():                             # (radius 1 at a share of 0.1 leaves no window six members)
                    assert radius == 1 and share == 0.1 and min_members == 6
                    continue
                err = np.maximum(np.abs(a.gx.astype(np.float64) - b.gx), np.abs(a.gy.astype(np.float64) - b.gy))[fitted]
                worst_slope = max(worst_slope, err.max())
                worst_rel = max(worst_rel, (err / np.maximum(np.abs(b.gx), np.abs(b.gy))[fitted]).max())
                worst_c = max(worst_c, np.abs(a.c.astype(np.float64) - b.c)[fitted].max())
                for row, col in np.argwhere(fitted)[::97]:       # the float64 path is numpy's least squares
                    sol = fm.lstsq_pixel(zm, row, col, radius)
                    worst_lstsq = max(worst_lstsq, abs(sol[0] - b.c[row, col]), abs(sol[1] - b.gx[row, col]), abs(sol[2] - b.gy[row, col]))
                    checked += 1
        worst[min_members] = (worst_slope, worst_c, worst_rel)
        print("min_members %d, float32 path against float64 path: worst slope difference %.3g (relative to the slope %.3g), worst c difference %.3g"
              % (min_members, worst_slope, worst_rel, worst_c))
    print("float64 path against lstsq at %d pixels: %.3g" % (checked, worst_lstsq))
    assert checked > 400 and worst_lstsq < 1e-12
    assert worst[6][0] <= 4 * F32_SLOPE_MEASURED and worst[6][1] <= 4 * F32_C_MEASURED
    assert worst[3][1] <= 4 * F32_C_MEASURED


def _ndc_angle(gx, gy, ex, ey, W, H):
    """degrees between the NDC plane normals (-gx W/2, gy H/2, 1) of estimated and exact slopes"""
    a = np.stack([-np.asarray(gx, np.float64) * W / 2, np.asarray(gy, np.float64) * H / 2, np.ones(np.shape(gx))], -1)
    b = np.stack([-np.asarray(ex, np.float64) * W / 2, np.asarray(ey, np.float64) * H / 2, np.ones(np.shape(ex))], -1)
    cos = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))


def test_the_fit_beats_central_differences_on_degraded_maps():
    """The NDC proxy, not rule N1's world normals: the angle between the NDC plane normals of estimated and exact slopes, a border of 2
    pixels left out; the exact slopes are the central differences of the exact float64 map (the scene is smooth: their own error is of
    second order).  Measured medians (DESIGN.md section 32 has the table): the fit at radius 4 against MVS_PROPAGATE_SLOPES' seed rule."""
    W, H = 96, 64
    truth, maps = _smooth_maps()
    ey, ex = np.gradient(truth)
    inner = (slice(2, H - 2), slice(2, W - 2))
    for name in ("rounded", "half", "quarter"):
        _, sx, sy = pm.seed_maps(maps[name], slopes=True)
        row = [float(np.median(_ndc_angle(sx, sy, ex, ey, W, H)[inner])), float(np.percentile(_ndc_angle(sx, sy, ex, ey, W, H)[inner], 90))]
        errs = [float(np.median(np.abs(maps[name].astype(np.float64) - truth)))]
        for radius in (2, 4):
            res = fm.fit(maps[name], radius, 255, INF, 6)
            ang = _ndc_angle(res.gx, res.gy, ex, ey, W, H)[inner]
            row += [float(np.median(ang)), float(np.percentile(ang, 90))]
        errs.append(float(np.median(np.abs(res.zfit.astype(np.float64) - truth))))
        print("%-8s central differences %.1f / %.1f deg, fit r = 2 %.1f / %.1f deg, fit r = 4 %.1f / %.1f deg (median / p90); median depth error %.4f -> %.4f"
              % ((name,) + tuple(row) + tuple(errs)))
        if name != "quarter":                                    # the two maps the bound is set for
            assert row[4] <= 0.5 * row[0], (name, row)


def test_the_depth_gate_keeps_the_plane_off_a_step():
    """two slanted planes (0.002 and 0.02 per pixel along the columns, 0.003 along the rows) with a step of 0.5 between columns 47 and 48,
    noise of +- 1/2 step of a 48-plane table, radius 4: within 4 pixels of the step, on either side, the fit gated at 4 steps is at most a
    quarter of the ungated fit's median angle (the NDC proxy, exact slopes analytic)"""
    W, H, step = 96, 64, 2.0 / 48
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    right = cols >= 48
    exact = np.where(right, -0.9 + 0.002 * 48 + 0.5 + 0.02 * (cols - 48), -0.9 + 0.002 * cols) + 0.003 * rows
    ex, ey = np.where(right, 0.02, 0.002), np.full((H, W), 0.003)
    z = (exact + step * np.random.Generator(np.random.PCG64(3220)).uniform(-0.5, 0.5, (H, W))).astype(f32)
    plain, gated = fm.fit(z, 4, 255, INF, 6), fm.fit(z, 4, 255, f32(4 * step), 6)
    sides = {"0.002": (cols >= 44) & (cols < 48), "0.02": (cols >= 48) & (cols < 52), "elsewhere": (np.abs(cols - 47.5) > 8)}
    med = {k: (float(np.median(_ndc_angle(plain.gx, plain.gy, ex, ey, W, H)[m])), float(np.median(_ndc_angle(gated.gx, gated.gy, ex, ey, W, H)[m]))) for k, m in sides.items()}
    print("step scene, median angle ungated / gated at 4 steps: " + ", ".join("%s %.1f / %.1f deg" % ((k,) + v) for k, v in med.items()))
    assert (gated.members > 0).all()
    for k in ("0.002", "0.02"):
        assert med[k][1] <= 0.25 * med[k][0], (k, med[k])
