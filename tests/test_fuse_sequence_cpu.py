"""Support planes, masked fusion and sequence fusion without a GPU: the premises of tests/fuse_sequence_cases.py
asserted on the mirror's intermediates (tests/fuse_sequence_mirror.py), so that a green tests/test_fuse_sequence_gpu.py means something; the
identities the contract implies; a table of small errors applied to copies of the mirror's text, each of which must change a named case's
bytes; the quality of the sequence cloud against the concatenation of the per-view clouds on tests/test_fuse_cpu.py's ring; and the new
entry points' refusal of a null context through the library."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import cKDTree

import fuse_mirror as fm
import fuse_sequence_cases as sc
import fuse_sequence_mirror as sm
import fusion_cases as fc
import mvs_amd
from mvs_amd import synth
from test_fuse_cpu import _centres

f32 = np.float32
BIG = sc.SIZES[0]
MS = sc.MIN_SUPPORT


def _store(size):
    st = fc.store(*size)
    mats = {s: fc.mats32(st["cams"][s]) for s in range(fc.DEPTH_CAP)}
    return dict(enumerate(st["depths"])), dict(enumerate(st["costs"])), sc.supports(*size), mats


def _seq(size, order, min_support):
    return sc.expected(size, order, min_support, _store(size)[3], "host")


# ---- the planes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_planes_put_the_threshold_on_the_seams_and_the_borders(size):
    W, H = size
    planes = sc.planes(W, H)
    assert not planes[sc.ALL_ZERO].any() and (planes[sc.ALL_255] == 255).all()
    others = [p for s, p in enumerate(planes) if s not in (sc.ALL_ZERO, sc.ALL_255)]
    assert all(set(np.unique(p)) == {0, 1, 2, 3, 4} for p in others)
    on, below = [np.stack([p == v for p in others]).any(0) for v in (MS, MS - 1)]
    for name, region in (("left", np.s_[:, 0]), ("right", np.s_[:, W - 1]), ("top", np.s_[0, :]), ("bottom", np.s_[H - 1, :])):
        assert on[region].any() and below[region].any(), name
    if W > 64:   # both sides of the 64-column seam, in one row, on and one below the threshold
        assert (on[:, 63] & on[:, 64]).any() and (below[:, 63] & below[:, 64]).any()
    if H > 4:    # both sides of a 4-row seam, in one column
        assert (on[3] & on[4]).any() and (below[3] & below[4]).any()


# ---- the mask's three roles ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.MASKED_CASES, ids=[c[0] for c in sc.MASKED_CASES])
def test_the_mask_changes_the_keep_set_through_each_role(case):
    name, ref, nbrs, kw = case
    depths, costs, supports, mats = _store(BIG)
    plain = fm.fuse(depths, costs, mats, ref, nbrs, **kw)
    mask = sm.fuse_masked(depths, costs, supports, mats, ref, nbrs, min_support=MS, **kw)
    low = supports[ref] < MS
    as_reference = int((plain["keep"] & low).sum())
    assert as_reference > 0 and not (mask["keep"] & low).any()
    max_rel = kw.get("max_rel_depth", 0.01)
    tv_plain, tv_mask = fc.tangent_variants(plain, max_rel), fc.tangent_variants(mask, max_rel)
    variant = (tv_plain[0] != tv_mask[0]) | (tv_plain[1] != tv_mask[1])
    both = plain["keep"] & mask["keep"]
    differ = (plain["normal"].view(np.uint32) != mask["normal"].view(np.uint32)).any(-1)
    as_tangent = int((both & variant & differ).sum())
    lost_tangent = int((plain["keep"] & ~low & ~mask["has_normal"]).sum())
    print("%s: reference %d, tangent variant changed %d (normal lost %d)" % (name, as_reference, as_tangent, lost_tangent))
    assert as_tangent > 0 and lost_tangent > 0
    if nbrs:
        mc = kw["min_consistent"]
        as_voter = int((plain["keep"] & mask["has_normal"] & (mask["agree"] < mc)).sum())
        print("%s: voter %d" % (name, as_voter))
        assert as_voter > 0
    assert mask["rows"].tobytes() != plain["rows"].tobytes() and 0 < mask["keep"].sum() < plain["keep"].sum()


def test_min_support_sits_on_the_threshold():
    """support == MIN_SUPPORT is valid, MIN_SUPPORT - 1 is not: both occur at pixels the unmasked fusion keeps"""
    depths, costs, supports, mats = _store(BIG)
    _, ref, nbrs, kw = sc.MASKED_CASES[0]
    plain = fm.fuse(depths, costs, mats, ref, nbrs, **kw)
    mask = sm.fuse_masked(depths, costs, supports, mats, ref, nbrs, min_support=MS, **kw)
    on, below = plain["keep"] & (supports[ref] == MS), plain["keep"] & (supports[ref] == MS - 1)
    assert on.sum() > 20 and below.sum() > 20 and mask["keep"][on].any() and not mask["keep"][below].any()


# ---- the sequence's premises ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_support", [0, MS])
@pytest.mark.parametrize("order", sorted(sc.ORDERS))
@pytest.mark.parametrize("size", sc.SEQ_SIZES, ids=lambda s: "%dx%d" % s)
def test_sequence_premises(size, order, min_support):
    W, H = size
    e = _seq(size, order, min_support)
    per = e["per_ref"]
    assert e["total"] == e["counts"].sum() == len(e["rows"]) and e["total"] > W * H // 2
    # every reference after the first has claimed pixels that the rules alone would keep
    assert not per[0]["shadowed"].any() and all(p["shadowed"].sum() > W * H // 100 for p in per[1:]), [int(p["shadowed"].sum()) for p in per]
    # each reference's count is at most its independent count
    assert all(p["kept"].sum() <= p["res"]["keep"].sum() for p in per)
    tangent_neighbour = voter = 0
    for p in per:
        # a claimed pixel is a tangent neighbour of a kept pixel: the kept pixel's variant uses it
        row_var, col_var = fc.tangent_variants(p["res"], 0.01)
        sh = np.pad(p["shadowed"], 1)
        tangent_neighbour += int((p["kept"] & ((((row_var & 1) > 0) & sh[1:-1, :-2]) | (((row_var & 2) > 0) & sh[1:-1, 2:]) |
                                               (((col_var & 1) > 0) & sh[:-2, 1:-1]) | (((col_var & 2) > 0) & sh[2:, 1:-1]))).sum())
        # a claimed pixel is an agreeing voter of a kept pixel
        for k, j in enumerate(p["nbrs"]):
            rj, cj, _ = sm.vote_pixel(_store(size)[3][j][0], p["res"]["X"], W, H)
            voter += int((p["kept"] & p["agreed"][k] & (p["before"][j][rj, cj] != 0)).sum())
    print("claimed pixels as tangent neighbours of kept pixels: %d, as agreeing voters: %d" % (tangent_neighbour, voter))
    assert tangent_neighbour > 0 and voter > 0
    # some pixel is claimed by two references
    twice = 0
    for s in e["claims"]:
        writers = sum(p["wrote"][s].astype(np.int32) for p in per if s in p["wrote"])
        twice += int((np.asarray(writers) >= 2).sum())
    assert twice > 0
    # claims fall in both tiles either side of a seam
    planes = np.stack(list(e["claims"].values())) != 0
    assert (planes[:, 3] & planes[:, 4]).any()
    if W > 64:
        assert (planes[:, :, 63] & planes[:, :, 64]).any()
    # the slot that is only ever a neighbour is claimed too; a slot's plane holds nothing but 0 and 1
    assert e["claims"][fc.AXIS].any() and set(np.unique(planes.astype(np.uint8))) == {0, 1}


@pytest.mark.parametrize("min_support", [0, MS])
@pytest.mark.parametrize("size", sc.SEQ_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_two_orders_give_different_rows(size, min_support):
    a, b = _seq(size, "a", min_support), _seq(size, "b", min_support)
    assert a["rows"].tobytes() != b["rows"].tobytes() and a["total"] != b["total"]


def test_the_mask_changes_the_sequence():
    assert _seq(BIG, "a", 0)["rows"].tobytes() != _seq(BIG, "a", MS)["rows"].tobytes()


def test_the_one_tile_case_has_claims_too():
    e = _seq(sc.SIZES[1], "a", 0)
    assert e["total"] > 20 and sum(int(p["shadowed"].sum()) for p in e["per_ref"]) > 10


# ---- identities -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_identities(size):
    depths, costs, supports, mats = _store(size)
    ref = fc.WIDE
    nbrs = sc.NEIGHBOURS[ref]
    one = sm.fuse_sequence(depths, costs, supports, mats, [ref], [nbrs], min_support=MS, **sc.SEQ_KW)
    single = sm.fuse_masked(depths, costs, supports, mats, ref, [j for j in nbrs if j != -1], min_support=MS, **sc.SEQ_KW)
    assert one["rows"].tobytes() == single["rows"].tobytes() and one["total"] == single["keep"].sum() > 0
    zero = sm.fuse_sequence(depths, costs, supports, mats, [ref], [nbrs], min_support=0, **sc.SEQ_KW)
    plain = fm.fuse(depths, costs, mats, ref, [j for j in nbrs if j != -1], **sc.SEQ_KW)
    assert zero["rows"].tobytes() == plain["rows"].tobytes() and zero["rows"].tobytes() != one["rows"].tobytes()
    # max_rows cuts the rows, not the totals
    e = _seq(size, "a", 0) if size in sc.SEQ_SIZES else zero
    cut = sm.fuse_sequence(depths, costs, supports, mats, [ref], [nbrs], min_support=0, max_rows=3, **sc.SEQ_KW)
    assert len(cut["rows"]) == 3 and cut["total"] == zero["total"] and e["total"] == len(e["rows"])


# ---- small errors in the mirror's text must change a named case's bytes -------------------------------------------------------------------------
ERRORS = [
    ("claims written for dropped pixels", "sel = kept & agreed[k]", "sel = agreed[k]", 0),
    ("claims gating votes", "maps = md   #",
     "maps = {s: (np.where(claim[s] != 0, f32(1.0), md[s]).astype(f32) if s in claim and s != ref else md[s]) for s in md}   #", 0),
    ("claims gating tangents", "maps = md   #", "maps = {s: (np.where(claim[s] != 0, f32(1.0), md[s]).astype(f32) if s == ref else md[s]) for s in md}   #", 0),
    ("> for >= at min_support", "< min_support] = f32(1.0)", "<= min_support] = f32(1.0)", MS),
    ("claims not cleared between calls", "claim = {s: np.zeros((H, W), np.uint8) for s in slots}", "claim = {s: STALE.setdefault(s, np.zeros((H, W), np.uint8)) for s in slots}", 0),
    ("rows not in reference order", "rows = np.concatenate(rows) if rows", "rows = np.concatenate(rows[::-1]) if rows", 0),
]


@pytest.mark.parametrize("error", ERRORS, ids=[e[0] for e in ERRORS])
def test_a_small_error_changes_the_bytes(error):
    name, old, new, min_support = error
    text = open(sm.__file__).read()
    assert text.count(old) == 1, old
    wrong = {"__name__": "fuse_sequence_mirror_with_an_error", "STALE": {}}
    exec(compile(text.replace(old, new), sm.__file__, "exec"), wrong)
    depths, costs, supports, mats = _store(BIG)
    order = sc.ORDERS["a"]
    right = _seq(BIG, "a", min_support)
    got = wrong["fuse_sequence"](depths, costs, supports, mats, order, sc.lists(order), min_support=min_support, **sc.SEQ_KW)
    if "STALE" in new:   # the first call starts from zeroed planes either way; the second must not see the first one's claims
        assert got["rows"].tobytes() == right["rows"].tobytes()
        got = wrong["fuse_sequence"](depths, costs, supports, mats, order, sc.lists(order), min_support=min_support, **sc.SEQ_KW)
    assert got["rows"].tobytes() != right["rows"].tobytes(), name
    if "reference order" in name:
        assert np.array_equal(np.sort(got["rows"].view(np.uint32), axis=0), np.sort(right["rows"].view(np.uint32), axis=0))


# ---- quality: the ring of tests/test_fuse_cpu.py at 160 x 120, exact maps -----------------------------------------------------------------------
def test_the_sequence_cloud_loses_nothing_and_repeats_nothing():
    """min_consistent 2, 1 px, 0.01: the sequence cloud has fewer rows than the concatenation of the five per-view clouds, and every row of
    that concatenation lies within half the sequence cloud's median nearest-neighbour spacing of a sequence row"""
    W, H = 160, 120
    scene = synth.Scene()
    depths, mats = {}, {}
    for s, c in enumerate(_centres()):
        depths[s] = scene.render(c, W, H, want_depth=True)[1]
        mats[s] = tuple(np.asarray(m, f32) for m in fm.slot_matrices(synth.camera_at(c, W, H)))
    refs = list(range(5))
    lists = [[j for j in refs if j != i] for i in refs]
    kw = dict(min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01)
    each = [fm.fuse(depths, {}, mats, i, lists[i], **kw)["rows"] for i in refs]
    seq = sm.fuse_sequence(depths, {}, {}, mats, refs, lists, **kw)
    cat = np.concatenate(each)
    tree = cKDTree(seq["rows"][:, :3].astype(np.float64))
    spacing = float(np.median(tree.query(seq["rows"][:, :3].astype(np.float64), k=2)[0][:, 1]))
    dist = tree.query(cat[:, :3].astype(np.float64))[0]
    print("per-view clouds: %d rows in total (%s); sequence cloud: %d rows (%s); farthest per-view row from a sequence row %.4f, exactly 0 for %.1f %%; "
          "median nearest-neighbour spacing of the sequence cloud %.4f" %
          (len(cat), " / ".join(str(len(r)) for r in each), seq["total"], " / ".join(str(c) for c in seq["counts"]), dist.max(), 100.0 * (dist == 0).mean(), spacing))
    assert seq["total"] < len(cat)
    assert dist.max() <= 0.5 * spacing, (dist.max(), spacing)
    assert all(c <= len(r) for c, r in zip(seq["counts"], each))


# ---- the library without a device -------------------------------------------------------------------------------------------------------------
def test_new_entry_points_refuse_a_null_context():
    lib = mvs_amd.load_library()
    n, total = C.c_int(7), C.c_longlong(7)
    one = (C.c_int * 1)(0)
    plane = (C.c_uint8 * 4)()
    assert lib.mvs_depth_support_upload(None, 0, plane) == -1
    assert lib.mvs_depth_support_upload_device(None, 0, None) == -1
    assert lib.mvs_depth_support_fetch(None, 0, plane) == -1
    assert lib.mvs_depth_support_drop(None, 0) == -1
    assert lib.mvs_fuse_depth_masked(None, 0, 0, None, 0, 1.0, 0.01, float("inf"), 1, None, C.byref(n)) == -1
    assert lib.mvs_tsdf_integrate_masked(None, 1, one, None, float("inf"), 1) == -1
    assert lib.mvs_fuse_sequence(None, 1, one, 0, None, 0, 1.0, 0.01, float("inf"), 0, 0, None, None, C.byref(total)) == -1
    assert lib.mvs_fuse_sequence_points_device(None) is None
    assert b"null context" in lib.mvs_last_error(None)
