"""flowRemap, compare() and the u8 resize of csrc/photometric.hip on the crafted inputs of tests/photometric_cases.py: every result against
the oracle bit for bit, and what can be stated without it (integer shifts are slices, what is no number reads the border, a constant
difference survives the pyramid exactly, compare() is symmetric) asserted ON THE DEVICE OUTPUT.  tests/test_photometric_cases_cpu.py is
the twin that checks the inputs and the oracle."""
import numpy as np
import pytest

import mvs_amd
import photometric_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(oracle):
    return oracle.cubic_table()


@pytest.mark.parametrize("stride", pc.REMAP_STRIDES)
@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_cases(oracle, table, W, H, stride):
    fields = pc.remap_fields(W, H)
    with mvs_amd.Context(W, H) as ctx:
        for kind in pc.REMAP_IMAGES:
            img = pc.remap_image(kind, W, H)
            for name, (u, v) in fields.items():
                flow = pc.pack_flow(u, v, stride)
                got = ctx.flow_remap(flow, img)
                tag = "%s %s" % (kind, name)
                if name in ("integer", "integer-far"):     # numpy slicing with a zero border
                    np.testing.assert_array_equal(got, pc.gather_zero_border(img, u, v), err_msg=tag)
                if name in pc.ZERO_FIELDS:                 # the short clamp, and NaN / infinite / beyond int32: the border
                    assert not got.any(), (tag, np.argwhere(got)[:3])
                if name == "fractions" and kind == "checker":
                    _, raw = pc.remap_mirror(u, v, img, table)
                    assert (raw < 0).any() and (raw > 255).any()
                    assert np.all(got[raw < 0] == 0) and np.all(got[raw > 255] == 255), tag   # 0 and 255 through the clamp
                np.testing.assert_array_equal(got, oracle.flow_remap(flow, img), err_msg=tag)


@pytest.mark.parametrize("W,H", pc.REMAP_SIZES)
def test_remap_outside_the_numbers_reads_the_border(oracle, W, H):
    """a coordinate whose x32 value is NaN, infinite or outside int32 reads the border: 0 -- on an image without a single 0, where a
    sample of pixel (0, 0) (what a float-to-int conversion that turns NaN into 0 picks) or of any other pixel shows as 200"""
    img = np.full((H, W), 200, np.uint8)
    fields = pc.remap_fields(W, H)
    with mvs_amd.Context(W, H) as ctx:
        for name in pc.ZERO_FIELDS:
            flow = pc.pack_flow(*fields[name], 2)
            got = ctx.flow_remap(flow, img)
            assert not got.any(), (name, np.argwhere(got)[:3])
            np.testing.assert_array_equal(got, oracle.flow_remap(flow, img), err_msg=name)
        # and a NaN in one component only of one pixel leaves every other pixel alone
        flow = np.zeros((H, W, 2), np.float32)
        flow[H // 2, W // 2, 1] = np.nan
        got = ctx.flow_remap(flow, img)
        assert got[H // 2, W // 2] == 0 and np.count_nonzero(got == 200) == W * H - 1


@pytest.mark.parametrize("W,H", pc.COMPARE_SIZES)
def test_compare_cases(oracle, W, H):
    with mvs_amd.Context(W, H) as ctx:
        for name, a, b, exact in pc.compare_pairs(W, H):
            got = ctx.compare(a, b)
            if exact is not None:   # identical: 0; a constant difference c: exactly c per level
                np.testing.assert_array_equal(got, np.float32(exact), err_msg=name)
            np.testing.assert_array_equal(got, ctx.compare(b, a), err_msg=name + " (symmetry)")
            np.testing.assert_array_equal(got, oracle.compare(a, b), err_msg=name)


def test_resize_cases(oracle):
    with mvs_amd.Context(64, 48) as ctx:
        for name, img, dw, dh in pc.resize_cases():
            got = ctx.resize(img, dw, dh)
            if (dw, dh) == (img.shape[1], img.shape[0]):
                np.testing.assert_array_equal(got, img, err_msg=name)   # the identity resize
            np.testing.assert_array_equal(got, oracle.resize_linear(img, dw, dh), err_msg=name)
