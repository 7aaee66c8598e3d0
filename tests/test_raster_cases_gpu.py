"""The rasteriser's kernels (csrc/raster.hip) on the crafted cases of tests/raster_cases.py: bit for bit against the CPU oracle, and against the
box-free mirrors of tests/raster_mirror.py that tests/test_raster_cases_cpu.py holds the oracle to.  Every case runs with MVS_RASTER_BINS=0 and =1
(the hooks are read when a Context is created, so the variable is set first); the binning cases also run under MVS_POISON_ALLOC=1 with a fresh
Context, where a read of an unwritten bin counter shows."""
import numpy as np
import pytest

import mvs_amd
import raster_cases as rc
import raster_mirror as rm

pytestmark = pytest.mark.gpu
f32 = np.float32
BINS = ["0", "1"]


def _context(monkeypatch, case, bins, poison=False, faces=None):
    if bins is None:
        monkeypatch.delenv("MVS_RASTER_BINS", raising=False)
    else:
        monkeypatch.setenv("MVS_RASTER_BINS", bins)
    if poison:
        monkeypatch.setenv("MVS_POISON_ALLOC", "1")
    else:
        monkeypatch.delenv("MVS_POISON_ALLOC", raising=False)
    ctx = mvs_amd.Context(case["W"], case["H"])
    ctx.load_mesh(case["verts"], case["faces"] if faces is None else faces)
    return ctx


def _same(got, ref, what):
    bad = got.view(np.uint8).reshape(got.shape[0], got.shape[1], -1) != ref.view(np.uint8).reshape(ref.shape[0], ref.shape[1], -1)
    assert not bad.any(), "%s: %d pixels differ from the oracle; first (row, col) %s: %s vs %s" % (
        what, int(bad.any(2).sum()), np.argwhere(bad.any(2))[0].tolist(), got[tuple(np.argwhere(bad.any(2))[0])], ref[tuple(np.argwhere(bad.any(2))[0])])


def _oracle_pair(oracle, case, faces=None, mipmap=True):
    soup = oracle.load_mesh(case["verts"], case["faces"] if faces is None else faces)
    depth = oracle.depth(soup, case["cam"], case["W"], case["H"])
    proj = oracle.projected(soup, case["cam"], case["frame"], case["prj"], mipmap=mipmap) if "prj" in case else None
    return depth, proj


def _assert_exact(case, depth, owner, zn, tol):
    drawn = (owner >= 0) & (zn != 1.0)
    bad = (depth != f32(1.0)) != drawn
    assert not bad.any(), "%s: coverage differs from the exact mirror at %s" % (case["name"], np.argwhere(bad)[:4].tolist())
    err = np.abs(depth.astype(np.float64) - zn)
    assert err.max() <= tol, "%s: z off by %g at %s" % (case["name"], err.max(), np.argwhere(err > tol)[:4].tolist())


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("name", rc.A_CASES)
def test_fill_rule_case(oracle, monkeypatch, name, bins):
    """every vertex order: depth == oracle bit for bit, coverage == the exact mirror's, z == the exact value (orthographic) or within the
    tolerance measured on the oracle (perspective: 1 / det is no power of two)"""
    case = rc.a_case(name)
    owner, zn, _ = rm.exact_render(rm.soup_of(case["verts"], case["faces"]), case["cam"], case["W"], case["H"])
    tol = rc.z_tol(name)
    with _context(monkeypatch, case, bins) as ctx:
        for order in rc.A_ORDERS:
            faces = rc.permuted(case["faces"], order)
            ctx.load_mesh(case["verts"], faces)
            got = ctx.depth(case["cam"])
            _same(got, _oracle_pair(oracle, case, faces)[0], "%s order %s" % (name, order))
            _assert_exact(case, got, owner, zn, tol)


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("kind,W,H", rc.ULP_CASES)
def test_edge_one_ulp_past_a_pixel_centre(oracle, monkeypatch, kind, W, H, bins):
    case = rc.ulp_case(kind, W, H)
    with _context(monkeypatch, case, bins) as ctx:
        got = ctx.depth(case["cam"])
    _same(got, _oracle_pair(oracle, case)[0], case["name"])
    bad = (np.abs(got - case["expected"]) > 1e-5) & case["band"]
    assert not bad.any(), "pixels lost at %s" % np.argwhere(bad)[:5].tolist()


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.B_CASES)
def test_depth_rule_case(oracle, monkeypatch, name):
    """depth == exact mirror == oracle, projected == oracle, byte for byte; the same on a second call and in both bin modes"""
    case = rc.b_case(name)
    owner, zn, _ = rm.exact_render(rm.soup_of(case["verts"], case["faces"]), case["cam"], case["W"], case["H"])
    d_ref, p_ref = _oracle_pair(oracle, case)
    seen = []
    for bins in BINS:
        with _context(monkeypatch, case, bins) as ctx:
            for call in range(2):
                d, p = ctx.depth(case["cam"]), ctx.projected(case["cam"], case["frame"], case["prj"])
                _same(d, d_ref, "%s bins %s call %d depth" % (name, bins, call))
                _same(p, p_ref, "%s bins %s call %d projected" % (name, bins, call))
                seen.append(d.tobytes() + p.tobytes())
            _assert_exact(case, d, owner, zn, 0.0)
            if name == "degenerate":
                ctx.load_mesh(case["verts"], case["faces"][rc.DEGENERATE_GOOD])
                assert ctx.depth(case["cam"]).tobytes() == d.tobytes()
                assert ctx.projected(case["cam"], case["frame"], case["prj"]).tobytes() == p.tobytes()
    assert len(set(seen)) == 1


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("name", rc.TIE_CASES)
def test_tie_goes_to_the_lower_face_id(oracle, monkeypatch, name, bins):
    """equal depths whose owner shows in projected() (the owner's own footprint picks the mip level): the tied faces come from the tile's list and
    the shared list, and from different batches of 256 candidates.  At the tied pixels the bytes are those of the first-listed group rendered alone"""
    case = rc.tie_case(name)
    d_ref, p_ref = _oracle_pair(oracle, case)
    with _context(monkeypatch, case, bins) as ctx:
        for call in range(2):
            _same(ctx.depth(case["cam"]), d_ref, "%s bins %s call %d depth" % (name, bins, call))
            p = ctx.projected(case["cam"], case["frame"], case["prj"])
            _same(p, p_ref, "%s bins %s call %d projected" % (name, bins, call))
    for col, (first, _) in rc.TIE_COLUMNS.items():
        alone = _oracle_pair(oracle, case, case["faces"][case["groups"][first]])[1]
        assert np.array_equal(p[rc.TIE_ROWS, col], alone[rc.TIE_ROWS, col])


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("name", rc.C_CASES)
def test_camera_plane_case(oracle, monkeypatch, name, bins):
    """the clipped box of a face across w = 0 loses no pixel: depth == oracle (whose box for such a face is the whole screen) bit for bit, every
    pixel surely inside the face is covered and none that is impossible"""
    case = rc.c_case(name)
    with _context(monkeypatch, case, bins) as ctx:
        got = ctx.depth(case["cam"])
    _same(got, _oracle_pair(oracle, case)[0], name)
    sure, possible = rm.classify(rm.soup_of(case["verts"], case["faces"]), case["cam"], case["W"], case["H"], case["eps"])
    cov = got != f32(1.0)
    assert not (sure & ~cov).any() and not (cov & ~possible).any()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def _render(ctx, case):
    return ctx.depth(case["cam"]), ctx.projected(case["cam"], case["frame"], case["prj"])


@pytest.mark.parametrize("poison", [False, True], ids=["", "poison"])
@pytest.mark.parametrize("name", rc.D_CASES)
def test_binning_case(oracle, monkeypatch, name, poison):
    """depth and projected: unbinned == binned == oracle, byte for byte; with poisoned allocations a fresh Context per mode"""
    case = rc.d_case(name)
    d_ref, p_ref = _oracle_pair(oracle, case)
    for bins in BINS:
        with _context(monkeypatch, case, bins, poison) as ctx:
            for call in range(1 if poison else 2):
                d, p = _render(ctx, case)
                _same(d, d_ref, "%s bins %s call %d depth" % (name, bins, call))
                _same(p, p_ref, "%s bins %s call %d projected" % (name, bins, call))
    if name == "behind":
        assert (d_ref == 1.0).all() and not p_ref.any()


@pytest.mark.parametrize("poison", [False, True], ids=["", "poison"])
@pytest.mark.parametrize("name", rc.D_SWITCH)
def test_default_switch_to_binning(oracle, monkeypatch, name, poison):
    """no hook set: 16 384 faces are binned, 16 383 are not; either way the bytes are those of both forced modes and of the oracle"""
    case = rc.d_switch_case(name)
    d_ref, p_ref = _oracle_pair(oracle, case)
    for bins in [None] + BINS:
        with _context(monkeypatch, case, bins, poison) as ctx:
            d, p = _render(ctx, case)
        _same(d, d_ref, "%s bins %s depth" % (name, bins))
        _same(p, p_ref, "%s bins %s projected" % (name, bins))


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(2, 5)] + rc.SHADOW_SIZES)
def test_shadow_pass_sizes(oracle, monkeypatch, W, H):
    """the occluder scene at widths of 2 (no interior column), 3, and around one and two blocks of the row-0 prefix minimum"""
    case = rc.shadow_case(W, H)
    d_ref, p_ref = _oracle_pair(oracle, case)
    for bins in BINS:
        with _context(monkeypatch, case, bins) as ctx:
            d, p = _render(ctx, case)
        _same(d, d_ref, "%s bins %s depth" % (case["name"], bins))
        _same(p, p_ref, "%s bins %s projected" % (case["name"], bins))


@pytest.mark.parametrize("axis,sign,on", rc.LIMIT_CASES)
def test_projector_limit_is_strict(oracle, monkeypatch, axis, sign, on):
    case = rc.limit_case(axis, sign, on)
    p_ref = _oracle_pair(oracle, case)[1]
    for bins in BINS:
        with _context(monkeypatch, case, bins) as ctx:
            p = ctx.projected(case["cam"], case["frame"], case["prj"])
        _same(p, p_ref, "limit axis %d sign %+g on %s bins %s" % (axis, sign, on, bins))
        assert (p[..., 1] == (0 if on else 255)).all()


@pytest.mark.parametrize("W,H,zx,zy", rc.MIP_CASES)
def test_mip_case(oracle, monkeypatch, W, H, zx, zy):
    """projected == oracle with the mip chain and with level 0 only, and again with the chain after the filter was switched back"""
    case = rc.mip_case(W, H, zx, zy)
    p_mip, p_lv0 = _oracle_pair(oracle, case)[1], _oracle_pair(oracle, case, mipmap=False)[1]
    what = "mip %dx%d zoom %g x %g" % (W, H, zx, zy)
    for bins in BINS:
        with _context(monkeypatch, case, bins) as ctx:
            _same(ctx.projected(case["cam"], case["frame"], case["prj"]), p_mip, what)
            ctx.set_texture_filter("level0")
            _same(ctx.projected(case["cam"], case["frame"], case["prj"]), p_lv0, what + " level0")
            ctx.set_texture_filter("mipmap")
            _same(ctx.projected(case["cam"], case["frame"], case["prj"]), p_mip, what + " again")
    if case["rho"] >= 2 ** case["levels"]:
        vis = p_mip[..., 1] == 255
        assert vis.any() and (p_mip[..., 0][vis] == rm.mip_chain(case["frame"])[-1][0, 0]).all()
