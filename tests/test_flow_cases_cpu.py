"""The crafted pairs of tests/flow_cases.py reach what they claim -- on the oracle alone, so that the bit-for-bit comparison of
tests/test_flow_cases_gpu.py can never pass on a case that no longer reaches its path."""
import numpy as np
import pytest

import flow_cases as fc

_refs = {}


def _ref(oracle, name):
    """the oracle's answer to a case, computed once"""
    if name not in _refs:
        _, W, H, a, b, farneback = fc.case(name)
        _refs[name] = oracle.calculate_flow(a, b, farneback)
        _refs[name].setflags(write=False)
    return _refs[name]


def test_the_case_list_is_what_the_names_say():
    cs = fc.cases()
    assert [c[0] for c in cs] == fc.case_names() and len(set(fc.case_names())) == len(cs)
    for name, W, H, a, b, farneback in cs:
        n2, W2, H2, a2, b2, f2 = fc.case(name)
        assert (W2, H2, f2) == (W, H, farneback) and a.shape == b.shape == (H, W) and a.dtype == b.dtype == np.uint8
        np.testing.assert_array_equal(a, a2)   # deterministic
        np.testing.assert_array_equal(b, b2)
        assert not farneback or W + H >= 100
    contents = {}
    for name in fc.case_names():
        contents.setdefault(name.rsplit("-", 1)[0], []).append(fc.content_of(name))
    for (W, H) in fc.FARNEBACK_ALL:
        assert tuple(contents["fb-%dx%d" % (W, H)]) == fc.CONTENTS
    for (W, H) in fc.FARNEBACK_FEW:
        assert contents["fb-%dx%d" % (W, H)] == ["noise", "saturated", "shifted"]
    assert contents["fb-8128x72"] == ["noise", "shifted"]
    for (W, H) in fc.VARIATIONAL_SIZES:
        assert tuple(contents["var-%dx%d" % (W, H)]) == fc.CONTENTS


def test_contents_are_what_they_say():
    a, b = fc.make_pair("checker", 5, 3)
    assert a[0, 0] == 0 and a[0, 1] == 255 and a[1, 0] == 255 and np.all(a.astype(int) + b == 255)
    a, b = fc.make_pair("step", 10, 4)
    assert not a[:, :5].any() and np.all(a[:, 5:] == 255) and not b[:, 3:8].any() and np.all(b[:, 8:] == 255) and np.all(b[:, :3] == 255)
    a, b = fc.make_pair("saturated", 64, 28)
    assert set(np.unique(a)) == {0, 255} and np.array_equal(b[:, 2:], a[:, :-2])
    a, b = fc.make_pair("impulse", 9, 9)
    assert not a.any() and b.sum() == 255 and b[4, 4] == 255
    a, b = fc.make_pair("noise", 61, 39)
    assert np.count_nonzero(a != b) > 0.98 * a.size and a.min() < 8 and a.max() > 247
    a, b = fc.make_pair("const", 4, 4)
    assert np.all(a == 255) and not b.any()
    a, b = fc.make_pair("identical", 70, 50)
    assert np.array_equal(a, b) and a.std() > 20


@pytest.mark.parametrize("name", fc.case_names())
def test_oracle_is_finite_on_every_case(oracle, name):
    assert np.all(np.isfinite(_ref(oracle, name))), name
    assert not _ref(oracle, name)[..., 3].any()


@pytest.mark.parametrize("W,H", [(61, 39), (60, 40), (129, 65)])
def test_noise_flows_leave_the_frame(oracle, W, H):
    share = fc.outside_share(_ref(oracle, "fb-%dx%d-noise" % (W, H)), W, H)
    print("noise %d x %d: %.1f %% of the targets outside the frame" % (W, H, 100 * share))
    assert share >= 0.30


@pytest.mark.parametrize("W,H", fc.SHIFTED_SIZES)
def test_shifted_flows_leave_the_frame(oracle, W, H):
    share = fc.outside_share(_ref(oracle, "fb-%dx%d-shifted" % (W, H)), W, H)
    print("shifted %d x %d: %.2f %% of the targets outside the frame" % (W, H, 100 * share))
    assert share >= 0.01


def test_the_sizes_with_a_shifted_bar_are_the_seven_of_the_table():
    assert sorted(fc.SHIFTED_SIZES) == sorted([(333, 201), (400, 399), (401, 399), (979, 520), (980, 520), (8127, 72), (8128, 72)])


@pytest.mark.parametrize("name", [n for n in fc.case_names() if fc.content_of(n) in (fc.ZERO_FLOW_FARNEBACK if n.startswith("fb") else fc.ZERO_FLOW_VARIATIONAL)])
def test_flow_is_exactly_zero_where_nothing_moves(oracle, name):
    assert not _ref(oracle, name)[..., :2].any(), name


@pytest.mark.parametrize("name", [n for n in fc.case_names() if fc.content_of(n) == "const"])
def test_variance_of_const_is_255_per_level(oracle, name):
    _, W, H, *_ = fc.case(name)
    np.testing.assert_array_equal(_ref(oracle, name)[..., 2], np.float32(255.0 * fc.compare_levels(W, H)))


def test_the_structured_cases_are_not_all_trivial(oracle):
    """step, saturated and shifted must move something: a non-zero flow at every size but 2 x 2 (else they would test what `zeros` tests)"""
    for name in fc.case_names():
        if fc.content_of(name) in ("step", "saturated", "shifted") and not name.startswith("var-2x2"):
            assert _ref(oracle, name)[..., :2].any(), name


def test_size_table():
    """the dispatch of csrc/flow.hip at the sizes of the cases, restated by flow_cases.farneback_geometry: a change of the dispatch that
    moves a case off the path it is here for shows up in this table"""
    g = fc.farneback_geometry
    # winsize 1 (m = 0); 0 pyramid levels against 1 (40 * 0.8 = 32 is not < 32)
    assert (g(61, 39)["winsize"], g(61, 39)["m"], g(61, 39)["levels"]) == (1, 0, 0)
    assert (g(60, 40)["winsize"], g(60, 40)["m"], g(60, 40)["levels"], g(60, 40)["sizes"]) == (1, 0, 1, [(60, 40), (48, 32)])
    assert (g(60, 39)["winsize"], g(2, 2)["winsize"]) == (0, 0)            # the refused corner
    assert (g(129, 65)["m"], g(129, 65)["forms"][0]) == (0, "fused") and -(-129 // 64) == 3 and 129 % 64 == 1 and 65 % 4 == 1
    assert (g(333, 201)["winsize"], g(333, 201)["m"], set(g(333, 201)["forms"])) == (5, 2, {"fused"})
    # m = 3, the last fused window, against m = 4, the first tiled one
    assert (g(400, 399)["winsize"], g(400, 399)["m"], set(g(400, 399)["forms"])) == (7, 3, {"fused"})
    assert (g(401, 399)["winsize"], g(401, 399)["m"], set(g(401, 399)["forms"])) == (8, 4, {"tiled 64x8"})
    # poly_n 5 against 7; on 256 CUs level 0 has 16 x 33 = 528 >= 512 tiles (64 x 16), the coarser levels of the same call 64 x 8
    for W, n in ((979, 5), (980, 7)):
        d = g(W, 520)
        assert (d["poly_n"], d["m"], d["forms"][0], set(d["forms"][1:])) == (n, 7, "tiled 64x16", {"tiled 64x8"}) and d["levels"] >= 1
    # m = 40 = FB_MAXM: the largest fused window, 115 840 bytes of dynamic LDS (the 160 KiB attribute); m = 41 leaves it
    d = g(8127, 72)
    assert (d["winsize"], d["m"], d["forms"][0], d["lds_bytes"], d["levels"]) == (81, fc.FB_MAXM, "tiled 64x16", 115840, 3)
    assert d["lds_bytes"] <= 160 * 1024
    d = g(8128, 72)
    assert (d["winsize"], d["m"], set(d["forms"])) == (82, 41, {"three-launch"})
    # sizes of the existing suite, for reference: m = 0, 2, 5, 10, 15, 30
    assert [g(W, H)["m"] for (W, H) in ((70, 50), (333, 201), (640, 480), (1280, 720), (1920, 1080), (3840, 2160))] == [0, 2, 5, 10, 15, 30]


def test_variational_sizes_straddle_the_solver_tiles():
    """VT_W x VT_H = 64 x 28 tiles with a halo of 10: smaller than the halo, one tile exactly, one pixel more, one staged region exactly
    (84 x 48 = tile + 2 halos), one more, and three tiles by three"""
    s = set(fc.VARIATIONAL_SIZES)
    assert {(2, 2), (5, 3), (9, 9)} <= s and all(max(w, h) < fc.VT_HALO for (w, h) in ((2, 2), (5, 3), (9, 9)))
    assert (11, 11) in s and 11 > fc.VT_HALO
    assert {(fc.VT_W - 1, fc.VT_H - 1), (fc.VT_W, fc.VT_H), (fc.VT_W + 1, fc.VT_H + 1)} <= s
    assert {(fc.VT_W + 2 * fc.VT_HALO, fc.VT_H + 2 * fc.VT_HALO), (fc.VT_W + 2 * fc.VT_HALO + 1, fc.VT_H + 2 * fc.VT_HALO + 1)} <= s
    assert (fc.VT_W + fc.VT_HALO, fc.VT_H + fc.VT_HALO) in s and (2 * fc.VT_W + 1, 2 * fc.VT_H + 1) in s


@pytest.mark.parametrize("W,H", [(60, 39), (2, 2), (33, 32), (8, 8)])
def test_oracle_refuses_farneback_without_a_window(oracle, W, H):
    z = np.zeros((H, W), np.uint8)
    with pytest.raises(ValueError, match="window"):
        oracle.calculate_flow(z, z, True)
    assert np.all(np.isfinite(oracle.calculate_flow(z, z, False)))   # the variational form stays valid down to 2 x 2
