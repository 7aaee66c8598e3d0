"""CPU twin of tests/test_photometric_cases_gpu.py: what the oracle alone can state about the crafted flowRemap, compare() and resize
inputs of tests/photometric_cases.py -- the inputs reach the branches they are here for, and the oracle keeps the contract the device
is then compared against."""
import numpy as np
import pytest

import photometric_cases as pc


@pytest.fixture(scope="module")
def table(oracle):
    return oracle.cubic_table()


@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_fields_reach_what_they_claim(W, H):
    f = pc.remap_fields(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    u, v = f["fractions"]
    q = np.concatenate([((u + xx) * 64).ravel(), ((v + yy) * 64).ravel()])
    assert np.all(q == np.rint(q))                                         # multiples of 1/64, exact in f32
    assert set(np.mod(q, 64).astype(int)) == set(range(64))                # every 1/32 fraction and every tie between two
    assert (u + xx).min() < -1 and (v + yy).min() < -1                     # on both sides of 0
    fx, fy = np.mod(((u + xx) * 64).astype(int), 64), np.mod(((v + yy) * 64).astype(int), 64)
    if H >= 64:
        assert len(set(zip(fx.ravel(), fy.ravel()))) == 64 * 64            # every pair of them
    for name, comp, n in (("border-x", 0, W), ("border-y", 1, H)):
        pos = f[name][comp] + (xx, yy)[comp]
        assert set(pos.ravel()) == set(np.float32(t) for t in (-2, -1, -1 / 64, 0, n - 1, n - 1 + 1 / 64, n, n + 2))
    u, v = f["border-xy"]
    assert len(set(zip((u + xx).ravel(), (v + yy).ravel()))) == 64          # every x target with every y target
    assert set(np.abs(f["short-x"][0]).ravel()) == {32767.0, 40000.0}
    for name, comps in (("huge-x", (0,)), ("huge-y", (1,)), ("huge-xy", (0, 1))):
        for c in comps:
            h = f[name][c]
            assert np.isnan(h).any() and np.isposinf(h).any() and np.isneginf(h).any()
            with np.errstate(invalid="ignore", over="ignore"):
                assert (np.abs(h) * 32 < 2 ** 31).any() and ((np.abs(h) * 32 >= 2 ** 31) & np.isfinite(h)).any()   # 6e7 fits, 7e7 does not
    u, v = f["huge-xy"]
    assert np.count_nonzero(np.isnan(u) & np.isnan(v)) and np.count_nonzero(np.isnan(u) & np.isinf(v)) and np.count_nonzero(np.isinf(u) & np.isfinite(v))
    for name in ("integer", "integer-far"):
        u, v = f[name]
        assert np.all(u == np.rint(u)) and np.all(v == np.rint(v)) and u.any() and v.any()
    u, v = f["integer-far"]
    assert (u + xx).min() == 0 and (u + xx).max() == W - 1 and (v + yy).min() >= 0 and (v + yy).max() == H - 1   # far, and inside


@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_oracle_equals_the_numpy_mirror(oracle, table, W, H):
    """orc_flow_remap == the Q15 sum restated in numpy, on every field and image, whatever the stride (the ignored channels carry NaN)"""
    for kind in pc.REMAP_IMAGES:
        img = pc.remap_image(kind, W, H)
        for name, (u, v) in pc.remap_fields(W, H).items():
            want, _ = pc.remap_mirror(u, v, img, table)
            for stride in pc.REMAP_STRIDES:
                np.testing.assert_array_equal(oracle.flow_remap(pc.pack_flow(u, v, stride), img), want, err_msg="%s %s stride %d" % (kind, name, stride))


@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_oracle_outside_the_numbers_reads_the_border(oracle, W, H):
    """NaN, the infinities and everything whose x32 value is no int32: output 0, like cvRound's INT_MIN in the reference -- on an image
    without a single 0, so that a sample of pixel (0, 0), or of any pixel, shows"""
    img = np.full((H, W), 200, np.uint8)
    f = pc.remap_fields(W, H)
    for name in pc.ZERO_FIELDS:
        out = oracle.flow_remap(pc.pack_flow(*f[name], 2), img)
        assert not out.any(), (name, np.argwhere(out)[:3])


@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_integer_shifts_are_slices(oracle, W, H):
    f = pc.remap_fields(W, H)
    for kind in pc.REMAP_IMAGES:
        img = pc.remap_image(kind, W, H)
        for name in ("integer", "integer-far"):
            u, v = f[name]
            np.testing.assert_array_equal(oracle.flow_remap(pc.pack_flow(u, v, 2), img), pc.gather_zero_border(img, u, v))


@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_checker_overshoots_into_the_clamp(oracle, table, W, H):
    """the cubic's negative lobes: on the 0 / 255 checker with fractional positions the unclamped sum goes below 0 and above 255, and the
    output holds both 0 and 255 THROUGH the clamp"""
    img = pc.remap_image("checker", W, H)
    u, v = pc.remap_fields(W, H)["fractions"]
    out, raw = pc.remap_mirror(u, v, img, table)
    assert raw.min() < 0 and raw.max() > 255
    got = oracle.flow_remap(pc.pack_flow(u, v, 2), img)
    assert np.all(got[raw < 0] == 0) and np.all(got[raw > 255] == 255)


# ---- compare() --------------------------------------------------------------------------------------------------------------

def test_compare_geometry():
    """one- and two-level pyramids, strips, and the pyramid_tail threshold of 4096 cells, restated"""
    lv = pc.compare_levels
    assert [lv(*s) for s in pc.COMPARE_SIZES] == [1, 2, 2, 1, 1, 2, 4, 7, 7, 7]
    assert pc.compare_level_sizes(8192, 3) == [(8192, 3), (4096, 2)] and pc.compare_tail_start(8192, 3) is None   # 8192 cells: no tail
    assert pc.compare_level_sizes(128, 128)[1] == (64, 64) and pc.compare_tail_start(128, 128) == 1                # exactly 4096 cells
    assert pc.compare_level_sizes(130, 128)[1] == (65, 64) and pc.compare_tail_start(130, 128) == 2                # 4160 cells
    assert pc.compare_tail_start(129, 127) == 2 and pc.compare_tail_start(33, 20) == 1
    assert pc.compare_tail_start(3, 3) is None and pc.compare_tail_start(5, 3) is None and pc.compare_tail_start(2, 2) is None
    # odd destinations of pyrUp on both axes, and an even one from an odd source
    assert pc.compare_level_sizes(129, 127)[:3] == [(129, 127), (65, 64), (33, 32)] and pc.compare_level_sizes(5, 3) == [(5, 3), (3, 2)]


@pytest.mark.parametrize("W,H", pc.COMPARE_SIZES)
def test_compare_oracle_on_the_crafted_pairs(oracle, W, H):
    for name, a, b, exact in pc.compare_pairs(W, H):
        out = oracle.compare(a, b)
        assert np.all(np.isfinite(out)) and out.min() >= 0, name
        if exact is not None:
            np.testing.assert_array_equal(out, np.float32(exact), err_msg=name)
        np.testing.assert_array_equal(out, oracle.compare(b, a), err_msg=name)
        if name.startswith("impulse"):
            y, x = np.argwhere(b)[0]
            assert out[y, x] == out.max() and out[y, x] >= 255.0, name      # level 0 alone contributes 255 there
    assert [pc.compare_levels(W, H) * 255.0 for (W, H) in ((2, 2), (3, 3), (33, 20), (128, 128))] == [255.0, 510.0, 1020.0, 1785.0]


def test_compare_corner_impulses_differ_from_each_other(oracle):
    """a single bright pixel in each corner makes the border branches of pyrUp visible: the four responses are no mirror images of each other
    at an odd size (the zero-insertion grid is anchored at the top left)"""
    W, H = 129, 127
    pairs = {n: oracle.compare(a, b) for n, a, b, _ in pc.compare_pairs(W, H) if n.startswith("impulse-")}
    assert not np.array_equal(pairs["impulse-tl"], pairs["impulse-br"][::-1, ::-1])
    assert not np.array_equal(pairs["impulse-tl"], pairs["impulse-tr"][:, ::-1])


# ---- resize -----------------------------------------------------------------------------------------------------------------

def test_resize_oracle_on_the_crafted_cases(oracle):
    names = [c[0] for c in pc.resize_cases()]
    assert len(set(names)) == len(names)
    for name, img, dw, dh in pc.resize_cases():
        out = oracle.resize_linear(img, dw, dh)
        sh, sw = img.shape[:2]
        if (dw, dh) == (sw, sh):
            np.testing.assert_array_equal(out, img, err_msg=name)          # the identity resize
        if (sw, sh) == (1, 1):
            assert np.all(out == img.reshape(-1)[0]), name                 # one source pixel: every destination pixel is it
        assert out.min() >= img.min() and out.max() <= img.max(), name     # bilinear: no overshoot
    assert any(dw / img.shape[1] > 3 and (dw / img.shape[1]) % 1 for _, img, dw, dh in pc.resize_cases())
