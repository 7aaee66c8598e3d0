"""Inputs shared by tests/test_normals_cpu.py (which checks each case's premise on the mirror) and tests/test_normals_gpu.py (which compares
the device with the mirror bit for bit), DESIGN.md section 31: the exact slopes of the crafted store's scene (tests/fusion_cases.py) for
cameras of any orientation, the normal planes made from them by rule N1, and the fusion cases with their premises.

A slope pair (gx, gy) is the change of NDC depth per pixel along a row and down a column, as the propagation holds it.  The tangent plane of
the scene at the point a pixel sees is n . X = n . X0 in the world; its row vector (n, -n . X0) times P^-1 is the same plane in NDC, and
dividing by the z coefficient gives a x + b y + z + d = 0 with gx = -a / (W / 2), gy = b / (H / 2).  All in float64, rounded once.
"""
import functools

import numpy as np

import fuse_mirror as fm
import fusion_cases as fc
import normals_mirror as nm

f32 = np.float32
NO_TEST = float("-inf")


def plane_hypotheses(cam, W, H, plane):
    """float64 (z, gx, gy) [H, W] of the unbounded world plane `plane` (fusion_cases.Plane) at the pixel centres of `cam`: a plane is affine
    in NDC, so the slopes are exact differences of z"""
    Pi = np.linalg.inv(np.asarray(cam, np.float64).reshape(4, 4))
    q = np.concatenate([plane.n, [-plane.d]]) @ Pi
    rows, cols = np.mgrid[0:H, 0:W]
    xn = (2.0 * cols + 1.0) / W - 1.0
    yn = 1.0 - (2.0 * rows + 1.0) / H
    z = -(q[0] * xn + q[1] * yn + q[3]) / q[2]
    gx = np.full((H, W), -(q[0] / q[2]) * (2.0 / W))
    gy = np.full((H, W), (q[1] / q[2]) * (2.0 / H))
    return z, gx, gy


def surface_slopes(cam, depth, prims=fc.SCENE):
    """float64 (gx, gy) [H, W] of the tangent plane of the scene at the point each pixel of `depth` (NDC, `cam`) sees; NaN where the depth
    is not inside (-1, 1)"""
    H, W = depth.shape
    P = np.asarray(cam, np.float64).reshape(4, 4)
    Pi = np.linalg.inv(P)
    rows, cols = np.mgrid[0:H, 0:W]
    xn = (2.0 * cols + 1.0) / W - 1.0
    yn = 1.0 - (2.0 * rows + 1.0) / H
    z = np.asarray(depth, np.float64)
    ok = (z > -1.0) & (z < 1.0)
    zz = np.where(ok, z, 0.0)
    h = np.einsum("ij,j...->i...", Pi, np.stack([xn, yn, zz, np.ones((H, W))]))
    X = h[:3] / h[3]
    n = fc.scene_distance(X, prims)[1]
    m = np.concatenate([n, -(n * X).sum(0)[None]])
    q = np.einsum("k...,kj->j...", m, Pi)
    with np.errstate(all="ignore"):
        gx = -(q[0] / q[2]) * (2.0 / W)
        gy = (q[1] / q[2]) * (2.0 / H)
    return np.where(ok, gx, np.nan), np.where(ok, gy, np.nan)


def hole_mask(W, H):
    """fusion_cases.punch_seams' holes as two masks (the 1.0 holes, the NaN holes): across the 64-column and 4-row seams, in the corners,
    around an isolated pixel, a whole segment and a whole row"""
    d = fc.punch_seams(np.zeros((H, W), f32))
    return d == f32(1.0), np.isnan(d)


def punch_normals(plane):
    """unusable values in a normal plane at hole_mask's pixels: zeros, NaN, an infinity, and vectors whose squared length is exactly 0.5
    and exactly 2 -- ON both bounds of the usable test, outside it"""
    out = np.array(plane, f32)
    H, W = out.shape[:2]
    ones, nans = hole_mask(W, H)
    rows, cols = np.mgrid[0:H, 0:W]
    out[ones & (rows % 2 == 0)] = f32(0.0)
    out[ones & (rows % 2 == 1)] = (f32(0.5), f32(0.5), f32(0.0))
    out[nans & (cols % 3 == 0)] = f32(np.nan)
    out[nans & (cols % 3 == 1)] = (f32(0.0), f32(np.inf), f32(0.0))
    out[nans & (cols % 3 == 2)] = (f32(1.0), f32(0.0), f32(-1.0))
    return out


SLOPE_NOISE = 0.6   # a slope is multiplied by 1 + SLOPE_NOISE u, u uniform in (-1, 1), and moved by SLOPE_SHIFT u' of a pixel's depth step
SLOPE_SHIFT = 2e-3


@functools.lru_cache(maxsize=None)
def planes(W, H):
    """-> {kind: [slot] -> [H, W, 3] f32} for every slot of fusion_cases.store(W, H): `exact` is rule N1 (the mirror's float32 path) on the
    scene's exact slopes at the stored depths, `noisy` the same on perturbed slopes, `holey` / `noisy_holey` those with punch_normals'
    holes, `away` the exact normals turned away from the camera (as a caller's own planes may be: rule 5n turns the row's back); and
    `support` [slot] -> [H, W] u8 planes with values 0 .. 4"""
    st = fc.store(W, H)
    rng = np.random.Generator(np.random.PCG64(0x2031 + 1000 * W + H))
    out = {"exact": [], "noisy": [], "holey": [], "noisy_holey": [], "away": [], "support": []}
    for s in range(fc.DEPTH_CAP):
        cam, depth = st["cams"][s], st["depths"][s]
        P, _, C = fc.mats32(cam)
        gx, gy = surface_slopes(cam, depth)
        exact = nm.hypothesis_normals(depth, gx.astype(f32), gy.astype(f32), P, C)
        nx = gx * (1.0 + SLOPE_NOISE * (2.0 * rng.random((H, W)) - 1.0)) + SLOPE_SHIFT * (2.0 * rng.random((H, W)) - 1.0)
        ny = gy * (1.0 + SLOPE_NOISE * (2.0 * rng.random((H, W)) - 1.0)) + SLOPE_SHIFT * (2.0 * rng.random((H, W)) - 1.0)
        noisy = nm.hypothesis_normals(depth, nx.astype(f32), ny.astype(f32), P, C)
        out["exact"].append(exact)
        out["noisy"].append(noisy)
        out["holey"].append(punch_normals(exact))
        out["noisy_holey"].append(punch_normals(noisy))
        out["away"].append(np.where(exact == f32(0.0), f32(0.0), -exact))
        out["support"].append(rng.integers(0, 5, (H, W), dtype=np.uint8))
    for kind in out.values():
        for a in kind:
            a.setflags(write=False)
    return out


def _cases():
    """(name, (W, H), reference slot, neighbour slots, {slot: kind of its normal plane} (a slot not named has none), parameters,
    min_normal_cos (a number, or "mid": the mirror's own median dot product), premise)"""
    cases = []
    T, R, Wd, D, S, M = fc.TILTED, fc.ROLLED, fc.WIDE, fc.DEEP, fc.SHIFTED, fc.MIRRORED
    for size in fc.SIZES:
        tag = "%dx%d" % size
        every = {s: "exact" for s in range(fc.DEPTH_CAP)}
        cases.append(("keepset_votes_" + tag, size, fc.HOLEY_AXIS, [T, R, Wd], every, dict(min_consistent=1), NO_TEST, dict(keepset=True)))
        cases.append(("keepset_alone_" + tag, size, fc.HOLEY_ROLLED, [], every, dict(min_consistent=0), NO_TEST, dict(keepset=True)))
        # the normal test decides: noisy planes on the reference and three voters, one voter without a plane, one with holes
        n0, n1, n2, n3, n4 = fc.NOISY
        cases.append(("cos_mid_" + tag, size, R, fc.NOISY, {R: "noisy", n0: "noisy", n1: "noisy", n3: "noisy_holey", n4: "noisy"},
                      dict(min_consistent=2, max_reproj_px=fc.MID_REPROJ, max_rel_depth=fc.MID_REL), "mid", dict(mid=True, at_min=True, mixed=True)))
        # unusable normals on both sides of the seams, in the reference's plane (over a whole depth map: rule 5 serves there) and the voters'
        cases.append(("holes_" + tag, size, fc.AXIS, [T, R, Wd], {fc.AXIS: "noisy_holey", T: "noisy_holey", R: "holey", Wd: "noisy"},
                      dict(min_consistent=1), "mid", dict(mid=True, holes=True)))
        # planes that face away from their cameras: the flip of rule 5n is taken
        cases.append(("away_" + tag, size, R, [T, Wd, S], {s: "away" for s in (R, T, Wd, S)}, dict(min_consistent=1), 0.9, dict(away=True)))
        # rule 1s beside rules 3n / 5n, under a finite max_cost
        cases.append(("support_" + tag, size, T, [fc.AXIS, R, Wd, D, S, M], {T: "noisy", fc.AXIS: "noisy", R: "exact", D: "noisy_holey", M: "noisy"},
                      dict(min_consistent=1, min_support=2, max_cost=float(fc.MAX_COST)), "mid", dict(mid=True)))
    return cases


CASES = _cases()
BY_NAME = {c[0]: c for c in CASES}


def case_inputs(case):
    """-> (depths, costs, supports, normals) dicts of the case's store"""
    _, size, _, _, kinds, _, _, _ = case
    st, pl = fc.store(*size), planes(*size)
    return (dict(enumerate(st["depths"])), dict(enumerate(st["costs"])), dict(enumerate(pl["support"])), {s: pl[k][s] for s, k in kinds.items()})


def min_cos_of(case, mats, mirror=nm):
    """the case's min_normal_cos: its number, or the median of the mirror's own dot products over the voters that pass rule 3 with both
    normals usable at valid pixels -- one voter sits ON the `>=`, about half on either side"""
    _, _, ref, nbrs, _, kw, cos, _ = case
    if cos != "mid":
        return float(cos)
    d, c, s, n = case_inputs(case)
    res = nm.fuse_normals(d, c, s, n, mats, ref, list(nbrs), min_normal_cos=NO_TEST, **kw)
    dots = np.concatenate([dot[sel & res["valid"]] for sel, dot in res["dots"]])
    return float(np.sort(dots)[len(dots) // 2])


def expected(case, mats, mirror=nm, min_normal_cos=None, normals=None, **over):
    """the mirror's result of a case; mats: slot -> (P, P^-1, centre)"""
    _, _, ref, nbrs, _, kw, _, _ = case
    d, c, s, n = case_inputs(case)
    cos = min_cos_of(case, mats) if min_normal_cos is None else min_normal_cos
    return mirror.fuse_normals(d, c, s, n if normals is None else normals, mats, ref, list(nbrs), min_normal_cos=cos, **dict(kw, **over))


def per_pixel_rows(res):
    """the rows of a mirror result scattered back to [H, W, 7] (zeros where no row)"""
    out = np.zeros(res["keep"].shape + (7,), f32)
    out[res["keep"]] = res["rows"]
    return out


def check_premise(case, mats):
    """what the case is for, asserted on the mirror with the given matrices -> the mirror's result"""
    import fuse_sequence_mirror as sm
    name, (W, H), ref, nbrs, kinds, kw, _, premise = case
    mc = f32(min_cos_of(case, mats))
    res = expected(case, mats)
    off = expected(case, mats, min_normal_cos=NO_TEST)
    d, c, s, n = case_inputs(case)
    plain = dict(kw)
    min_support = plain.pop("min_support", 0)
    masked = sm.fuse_masked(d, c, s, mats, ref, nbrs, min_support=min_support, **plain)
    m = kw["min_consistent"]
    rows, cols = np.mgrid[0:H, 0:W]
    # rule 5n against rule 5, with the normal test off: nothing is lost, the points are the same, and pixels without a tangent appear
    assert not (masked["keep"] & ~off["keep"]).any(), name
    assert per_pixel_rows(off)[masked["keep"]][:, :4].tobytes() == masked["rows"][:, :4].tobytes(), name
    fresh = off["keep"] & ~masked["keep"]
    assert (fresh <= (off["valid"] & ~off["tangent_ok"] & off["ref_usable"])).all(), name
    if premise.get("keepset"):
        assert fresh.any(), name
        for b in range(64, W if m == 0 else min(W, 65), 64):   # (the voters do not see the reference's last columns)
            assert fresh[:, b - 1].any() and fresh[:, b].any(), (name, "no new pixel beside the column seam at", b)
        for b in (4, 64):
            if b < H:
                assert fresh[b - 1].any() and fresh[b].any(), (name, "no new pixel beside the row seam at", b)
        along_row, along_col = fc.tangent_variants(off, kw.get("max_rel_depth", 0.01))
        lone = off["valid"] & (along_row == 0) & (along_col == 0)
        assert lone.any() and (m > 0 or fresh[lone].all()), (name, "an isolated pixel")
        assert (fresh & lone).any(), (name, "an isolated pixel is kept")
    if premise.get("mid"):
        dots = np.concatenate([dot[sel & res["valid"]] for sel, dot in res["dots"]])
        share = float((dots >= mc).mean())
        assert len(dots) >= 20 and 0.1 <= share <= 0.9 and (dots == mc).any(), (name, len(dots), share)
        assert (res["agree"] != off["agree"]).any(), name
    if premise.get("at_min"):   # caused by the normal test alone
        hn = res["has_normal"]
        assert (hn & (res["agree"] == m) & (off["agree"] > m)).any() and (hn & (res["agree"] == m - 1) & (off["agree"] >= m)).any(), name
    if premise.get("mixed"):
        assert any(j not in kinds for j in nbrs) and any(j in kinds for j in nbrs), name
        j = [k for k, v in enumerate(nbrs) if v not in kinds][0]
        assert not res["dots"][j][0].any() and (res["tests"][j][0] & res["keep"]).any(), (name, "a voter without a plane votes at kept pixels")
    if premise.get("holes"):
        bad = off["valid"] & ~off["ref_usable"]
        assert bad.any() and (bad & off["keep"]).any() and (bad & ~off["keep"]).any(), name
        for b in range(64, W, 64):
            assert bad[:, b - 1].any() and bad[:, b].any(), (name, "no unusable normal beside the column seam at", b)
        for b in (4, 64):
            if b < H:
                assert bad[b - 1].any() and bad[b].any(), (name, "no unusable normal beside the row seam at", b)
        reached = sum(int((t[0] & off["ref_usable"]).sum()) for t in off["tests"])
        assert sum(int(sel.sum()) for sel, _ in off["dots"]) < reached, (name, "no voter with an unusable normal")
    if premise.get("away"):
        k = res["keep"] & res["ref_usable"]
        stored = np.asarray(n[ref])[k].astype(np.float64)
        assert k.sum() > 20 and ((res["normal"][k].astype(np.float64) * stored).sum(-1) < 0).all(), (name, "rule 5n turns the rows toward the camera")
    return res
