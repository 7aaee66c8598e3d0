"""The crafted rasteriser cases of tests/raster_cases.py on the CPU: the oracle (oracle/raster_oracle.c) against the two box-free mirrors of
tests/raster_mirror.py, and the premise of every case -- that it puts a value ON the decision it is named after.  The oracle walks the same
bounding boxes as the kernel, so "kernel == oracle" (tests/test_raster_cases_gpu.py) proves nothing about boxes, tie rule or depth limits; this
file is where the oracle earns its place as the kernel's reference.  A wrong tie rule, a box without its pixel of slack or GL_LEQUAL in the oracle
makes tests here fail."""
import numpy as np
import pytest

import raster_cases as rc
import raster_mirror as rm
import scenes
from mvs_amd import synth

f32 = np.float32
AMBIGUOUS_CAP = 0.02


def _soup(case, faces=None):
    return rm.soup_of(case["verts"], case["faces"] if faces is None else faces)


def _exact(case, faces=None):
    return rm.exact_render(_soup(case, faces), case["cam"], case["W"], case["H"])


def _assert_oracle_is_exact(oracle, case, faces, owner, zn, tol):
    """coverage equal, z within tol of the exact value (tol == 0: bit for bit)"""
    d = oracle.depth(_soup(case, faces), case["cam"], case["W"], case["H"])
    drawn = (owner >= 0) & (zn != 1.0)
    bad = (d != f32(1.0)) != drawn
    assert not bad.any(), "%s: coverage differs from the exact mirror at %s" % (case["name"], np.argwhere(bad)[:4].tolist())
    err = np.abs(d.astype(np.float64) - zn)
    print("%s: max |z - exact| = %.3g" % (case["name"], err.max()))
    assert err.max() <= tol, "%s: z off by %g at %s" % (case["name"], err.max(), np.argwhere(err > tol)[:4].tolist())
    return d


def _rect_pixels(W, H, u0, v0, u1, v1):
    """the pixels of a watertight patch over the rectangle [u0, u1] x [v0, v1] under the tie rule: an edge through pixel centres belongs to the
    face on its right (a > 0) or, if horizontal, to the face above it (b > 0; y points up) -- left and bottom edges in, right and top edges out"""
    cu, cv = np.arange(W) + 0.5, np.arange(H) + 0.5
    return ((cv > v0) & (cv <= v1))[:, None] & ((cu >= u0) & (cu < u1))[None, :]


_A_RECT = {"diag_quad": (8.5, 4.5, 24.5, 20.5), "fan_centres": (23.5, 7.5, 39.5, 23.5), "fan_corners": (23.0, 7.0, 40.0, 24.0),
           "grid_hv": (10.5, 6.5, 30.5, 22.5)}


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.A_CASES)
def test_fill_rule_case(oracle, name):
    """exact mirror == oracle in all six vertex orders (both windings) and a mixed one; the owner map does not depend on the order, every pixel
    of a watertight patch has exactly one owner, and the patch covers exactly the pixels the tie rule gives it"""
    case = rc.a_case(name)
    W, H = case["W"], case["H"]
    owner, zn, hits = _exact(case)
    tol = rc.z_tol(name)
    for order in rc.A_ORDERS:
        faces = rc.permuted(case["faces"], order)
        o2, z2, h2 = _exact(case, faces)
        assert np.array_equal(o2, owner) and np.array_equal(z2, zn) and np.array_equal(h2, hits), "order %s changes the exact render" % (order,)
        _assert_oracle_is_exact(oracle, case, faces, owner, zn, tol)
    shape = case["shape"]
    if shape in _A_RECT:
        assert np.array_equal(hits, _rect_pixels(W, H, *_A_RECT[shape]).astype(hits.dtype)), "not watertight, or not the tie rule's pixels"
        assert len(np.unique(owner[owner >= 0])) == len(case["faces"])          # every face owns some pixel
    elif shape == "slivers":
        assert hits.sum() == 1 and owner[8, 20] == 1
    else:
        assert (owner >= 0).all() and (hits[:, 0] >= 1).all() and (hits[0] >= 1).all()
        assert owner[H - 1, 0] == 2 and owner[0, W // 2] == 3 and owner[H // 2, W - 1] == 4 and owner[0, 0] == 0 and owner[H - 1, W - 1] == 1
        assert (owner[0] == 3).sum() >= W // 4 and (owner[:, W - 1] == 4).sum() >= H // 4


@pytest.mark.parametrize("kind,W,H", rc.ULP_CASES)
def test_edge_one_ulp_past_a_pixel_centre(oracle, kind, W, H):
    """the pixel an edge clears by one ulp is drawn by that face: a box without its pixel of slack loses columns 49, 52, 53, 58, 59 of the 100-wide
    frame.  z is constant per face and the faces are 1 / 512 apart; 1e-5 allows for the f32 plane (za, zb of the order of an ulp, zc = z to an ulp)"""
    case = rc.ulp_case(kind, W, H)
    xn, yn = rc.pixel_centres(W, H)
    assert all(oracle.lib.orc_pixel_xn(c, W) == xn[c] for c in range(W)) and all(oracle.lib.orc_pixel_yn(r, H) == yn[r] for r in range(H))
    d = oracle.depth(_soup(case), case["cam"], W, H)
    bad = (np.abs(d - case["expected"]) > 1e-5) & case["band"]
    assert case["band"].sum() >= 500 and not bad.any(), "pixels lost at %s" % np.argwhere(bad)[:5].tolist()


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.B_CASES)
def test_depth_rule_case(oracle, name):
    case = rc.b_case(name)
    W, H = case["W"], case["H"]
    owner, zn, hits = _exact(case)
    d = _assert_oracle_is_exact(oracle, case, None, owner, zn, 0.0)
    soup = _soup(case)
    p = oracle.projected(soup, case["cam"], case["frame"], case["prj"])
    assert np.array_equal(p[..., 1] == 255, owner >= 0)                        # the projector sees every drawn pixel
    if name == "zn_limits":
        assert (d[5:20, 3:14] == -1.0).all() and (owner[5:20, 3:14] >= 0).all()                    # zn == -1 is kept
        assert (d[5:20, 17:28] == 1.0).all() and (hits[5:20, 17:28] == 1).all() and (owner[5:20, 17:28] == -1).all()   # zn == +1: a fragment, never drawn
        assert (d[5:20, 31:42] == 0.5).all() and (hits[5:20, 31:42] == 1).all()                    # one step beyond: no fragment at all
        assert (d[5:20, 45:58] == 0.5).all() and (hits[5:20, 45:58] == 1).all()
    elif name == "near_far_cut":
        assert d[5, 10] == -1.0 and owner[5, 10] == 2 and d[5, 9] == 0.75 and d[5, 11] == -0.9375   # cut along column 10, the column kept
        assert d[22, 23] == 0.9375 and owner[22, 23] == 3 and hits[22, 24] == 1 and owner[22, 24] == -1 and hits[22, 25] == 0
    elif name == "duplicates":
        assert hits.max() == 5                                             # three copies of the quad, a large face, the nearer face
        tied = hits > 1
        assert tied.sum() > 400 and np.isin(owner[9:13, 16:24], (5, 6)).all()   # the nearer face in between wins where it is
        assert set(np.unique(owner)) == {-1, 0, 1, 4, 5, 6, 9}                 # of equal faces the first listed owns the pixel
    elif name == "degenerate":
        good = case["faces"][rc.DEGENERATE_GOOD]
        assert set(np.unique(owner)) == {-1, 0, 1, 8}
        d_good = oracle.depth(_soup(case, good), case["cam"], W, H)
        assert d.tobytes() == d_good.tobytes()
        assert p.tobytes() == oracle.projected(_soup(case, good), case["cam"], case["frame"], case["prj"]).tobytes()


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------
def _assert_classified(oracle, case, what):
    W, H = case["W"], case["H"]
    soup = _soup(case)
    sure, possible = rm.classify(soup, case["cam"], W, H, case.get("eps", 1e-4))
    cov = oracle.depth(soup, case["cam"], W, H) != f32(1.0)
    ambiguous = float((possible & ~sure).mean())
    print("%s: covered %.4f, surely covered %.4f, ambiguous %.4f" % (what, cov.mean(), sure.mean(), ambiguous))
    assert ambiguous <= AMBIGUOUS_CAP
    assert not (sure & ~cov).any(), "%s: %d pixels surely inside a face are not covered" % (what, (sure & ~cov).sum())
    assert not (cov & ~possible).any(), "%s: %d pixels impossible for every face are covered" % (what, (cov & ~possible).sum())
    return cov


@pytest.mark.parametrize("name", rc.C_CASES)
def test_camera_plane_case(oracle, name):
    case = rc.c_case(name)
    W, H = case["W"], case["H"]
    cov = _assert_classified(oracle, case, name)
    w = case["cam"].astype(np.float64) @ case["verts"].astype(np.float64).T
    behind = int((w[3] <= 0).sum())
    shape = case["shape"]
    assert behind == {"one_behind": 1, "two_behind": 2, "on_w0": 1, "all_behind": 3, "corner": 2, "whole_screen": 1, "ground_strip": 1}[shape]
    if shape == "on_w0":
        assert w[3, 2] == 0.0
    if shape == "all_behind":
        assert not cov.any()
    elif shape == "whole_screen":
        assert cov.all()
    elif shape == "corner":
        assert cov[H - 1, 0] and 0 < cov.mean() < 0.02 and not cov[:H // 2].any() and not cov[:, W // 2:].any()
    else:
        assert 0.3 < cov.mean() < 0.6 and not cov[:H // 2 - 2].any() and cov[H - 1].all()


@pytest.mark.parametrize("W,H,n", [(64, 48, 12), (333, 211, 24)])
def test_classifier_on_a_height_field(oracle, W, H, n):
    """the classifier on a general mesh (242 and 1 058 faces): its ambiguous share stays under the cap there too"""
    verts, faces = scenes.heightfield_mesh(n)
    case = dict(name="heightfield", W=W, H=H, verts=verts, faces=faces, cam=synth.camera_at([0.02, -0.01, 0.0], W, H))
    assert _assert_classified(oracle, case, "height field %d" % n).all()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def test_binning_cases_reach_their_boundaries():
    assert rc.bins_covered(rc.d_case("maxcover")).tolist() == [list(b) for b in rc.MAXCOVER_BINS]
    assert sorted(nx * ny for nx, ny in rc.MAXCOVER_BINS)[:5] == [4, 4, 4, 5, 6] and rc.BIN_MAXCOVER == 4
    box = rc.face_boxes(rc.d_case("small300"))
    assert len(box) == 300 and box[:, :2].min() >= 16 and box[:, 2:].max() <= 31                  # one bin, more than one batch of 256
    both = rc.d_case("small300_large5")
    cover = rc.bins_covered(both).prod(1)
    assert len(cover) == 306 and (cover > rc.BIN_MAXCOVER).sum() == 5 and (cover == 1).sum() == 301
    n_small = int((cover == 1).sum())
    assert n_small > 256 and n_small % 256 + 5 <= 256                          # the bin's second batch of 256 candidates runs on into the shared list
    assert (rc.bins_covered(rc.d_case("large300")).prod(1) == 12).all()        # 64 x 48: every bin of the frame
    seam = rc.face_boxes(rc.d_case("seam"))
    assert (seam[:, 2] // rc.BIN > seam[:, 0] // rc.BIN).any()
    assert len(rc.d_switch_case("grid_16384")["faces"]) == rc.BIN_MIN_FACES and len(rc.d_switch_case("grid_16383")["faces"]) == rc.BIN_MIN_FACES - 1
    for name, bins in (("ragged_333x211", 21 * 14), ("ragged_17x17", 4), ("single_8x8", 1)):
        c = rc.d_case(name)
        assert -(-c["W"] // rc.BIN) * -(-c["H"] // rc.BIN) == bins


@pytest.mark.parametrize("name", rc.D_CASES)
def test_binning_case_against_the_classifier(oracle, name):
    """a side check of the oracle on the binning scenes, not a validation of their coverage: small faces are mostly edge, so few pixels are sure
    (the share is printed) and no ambiguity cap is asked; what these scenes are for is the comparison of the bin modes on the GPU"""
    case = rc.d_case(name)
    soup = _soup(case)
    sure, possible = rm.classify(soup, case["cam"], case["W"], case["H"])
    cov = oracle.depth(soup, case["cam"], case["W"], case["H"]) != f32(1.0)
    print("%s: covered %.4f, surely covered %.4f, ambiguous %.4f" % (name, cov.mean(), sure.mean(), (possible & ~sure).mean()))
    assert not (sure & ~cov).any() and not (cov & ~possible).any()
    assert cov.any() == (name != "behind")


# ---- ties ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.TIE_CASES)
def test_tie_case_names_its_owner(oracle, name):
    """the depths tie exactly (the exact mirror counts two fragments and hands the pixel to whichever face is listed first), and the oracle's
    projected() shows the owner: at the tied pixels it equals the render of the first-listed group alone, which differs from the later group's in
    more than half of them; with the face list reversed the depth map is the same and the tied pixels are the other group's"""
    case = rc.tie_case(name)
    W, H, rows, groups = case["W"], case["H"], rc.TIE_ROWS, case["groups"]
    soup = _soup(case)
    nf = len(soup)
    owner, _, hits = rm.exact_render(soup, case["cam"], W, H)
    owner_rev = nf - 1 - rm.exact_render(soup[::-1].copy(), case["cam"], W, H)[0]
    render = lambda sp: oracle.projected(sp, case["cam"], case["frame"], case["prj"])
    full, rev = render(soup), render(soup[::-1].copy())
    assert oracle.depth(soup, case["cam"], W, H).tobytes() == oracle.depth(soup[::-1].copy(), case["cam"], W, H).tobytes()
    for col, (first, later) in rc.TIE_COLUMNS.items():
        assert (hits[rows, col] == 2).all() and np.isin(owner[rows, col], groups[first]).all() and np.isin(owner_rev[rows, col], groups[later]).all()
        a, b = render(soup[groups[first]]), render(soup[groups[later]])
        assert (full[rows, col, 1] == 255).all() and (a[rows, col, 1] == 255).all() and (b[rows, col, 1] == 255).all()
        differ = int((a[rows, col, 0] != b[rows, col, 0]).sum())
        print("%s column %d: the two owners give different bytes in %d of 16 pixels" % (name, col, differ))
        assert differ > 8
        assert np.array_equal(full[rows, col], a[rows, col]) and np.array_equal(rev[rows, col], b[rows, col])
    cover = rc.bins_covered(case).prod(1)
    assert (cover[groups["F"]] == 6).all() and (cover[groups["S_a"] + groups["S_b"]] == 4).all()   # shared list vs the tiles' own lists
    if name == "tie_batches":
        box = rc.face_boxes(case)[[i for i in range(nf) if cover[i] == 1]]
        assert len(box) == 300 and box[:, 0].min() >= 16 and box[:, 2].max() <= 31 and box[:, 3].max() <= 15       # all in the bin of columns 16-31
        assert max(groups["F"]) < 256 <= min(groups["S_b"])                                                         # different batches, unbinned


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,sign,on", rc.LIMIT_CASES)
def test_projector_limit_is_strict(oracle, axis, sign, on):
    """projector NDC exactly +-1 is out of frame; one ulp inside is in frame, and its texture coordinate lands on the frame's edge"""
    case = rc.limit_case(axis, sign, on)
    out = oracle.projected(_soup(case), case["cam"], case["frame"], case["prj"])
    assert (out[..., 1] == (0 if on else 255)).all()
    if not on:
        assert len(np.unique(out[..., 0])) > 8                                  # texels, not a constant


@pytest.mark.parametrize("W,H,zx,zy", rc.MIP_CASES)
def test_mip_case_premise(oracle, W, H, zx, zy):
    """pixels are in frame, the mip chain changes them, and past the last level every one of them is the chain's single last texel"""
    case = rc.mip_case(W, H, zx, zy)
    soup = _soup(case)
    mip = oracle.projected(soup, case["cam"], case["frame"], case["prj"], mipmap=True)
    lv0 = oracle.projected(soup, case["cam"], case["frame"], case["prj"], mipmap=False)
    vis = mip[..., 1] == 255
    assert vis.sum() >= min(W, H) and np.array_equal(vis, lv0[..., 1] == 255)
    assert (mip[..., 0] != lv0[..., 0])[vis].any()
    chain = rm.mip_chain(case["frame"])
    assert len(chain) - 1 == case["levels"]
    if case["rho"] >= 2 ** case["levels"]:
        assert (mip[..., 0][vis] == chain[-1][0, 0]).all()


def test_mip_chain_shapes():
    """the frames of MIP_CASES take the branches they are named for: an axis at 1 before the other, level 1 of 64 and of 65 texels, odd parents"""
    shapes = {(W, H): [l.shape[::-1] for l in rm.mip_chain(rc.noise_frame(W, H))] for (W, H, _, _) in rc.MIP_CASES}
    assert shapes[(256, 4)][2:4] == [(64, 1), (32, 1)] and shapes[(5, 300)][2:4] == [(1, 75), (1, 37)]
    assert shapes[(128, 128)][1] == (64, 64) and shapes[(130, 130)][1:3] == [(65, 65), (32, 32)]
    assert shapes[(37, 23)][1:] == [(18, 11), (9, 5), (4, 2), (2, 1), (1, 1)]
