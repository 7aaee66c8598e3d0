"""mvs_flow (Context.flow) against oracle.calculate_flow on the crafted pairs of tests/flow_cases.py: all four channels, every pixel, bit
for bit.  tests/test_flow_cases_cpu.py asserts on the oracle alone that every case reaches the path it is here for; the exact-zero and
255-per-level statements are asserted here again ON THE DEVICE OUTPUT, as anchors that do not go through the oracle."""
import numpy as np
import pytest

import flow_cases as fc
import mvs_amd

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(oracle, name):
    """the oracle's answer to a case, computed once and shared, read-only"""
    if name not in _refs:
        _, W, H, a, b, farneback = fc.case(name)
        _refs[name] = oracle.calculate_flow(a, b, farneback)
        _refs[name].setflags(write=False)
    return _refs[name]


def _first_difference(got, ref):
    d = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    if not len(d):
        return "equal"
    y, x, c = d[0]
    return "%d of %d values differ, first at (x %d, y %d, channel %d): device %r, oracle %r" % (len(d), got.size, x, y, c, got[y, x, c], ref[y, x, c])


@pytest.mark.parametrize("name", fc.case_names())
def test_flow_case_matches_oracle(oracle, name):
    _, W, H, a, b, farneback = fc.case(name)
    ref = _ref(oracle, name)
    with mvs_amd.Context(W, H) as ctx:
        got = ctx.flow(a, b, farneback)
    assert np.all(np.isfinite(got)), name
    content = fc.content_of(name)
    if content in (fc.ZERO_FLOW_FARNEBACK if farneback else fc.ZERO_FLOW_VARIATIONAL):
        assert not got[..., :2].any(), name   # exactly 0.0, on the device output itself
    if content == "const":
        np.testing.assert_array_equal(got[..., 2], np.float32(255.0 * fc.compare_levels(W, H)))
    if content in ("zeros", "identical") and not farneback:
        assert not got[..., 2].any(), name
    assert not got[..., 3].any()
    np.testing.assert_array_equal(got, ref, err_msg="%s: %s" % (name, _first_difference(got, ref)))


@pytest.mark.parametrize("first,second", [("fb-401x399-noise", "fb-401x399-zeros"), ("var-85x49-saturated", "var-85x49-zeros"),
                                          ("fb-129x65-saturated", "var-129x65-noise")])
def test_one_context_carries_nothing_from_flow_to_flow(oracle, first, second):
    """two different cases back to back in ONE context, then the first again: the same bytes, each equal to the oracle's -- the arenas and the
    M / M2 / vs aliasing (the fused iteration's second matrix buffer lives in the three-launch form's vertical sums) carry nothing over.
    The third pair switches the algorithm between the calls: the variational arena overlays Farneback's."""
    _, W, H, a1, b1, f1 = fc.case(first)
    if second in fc.case_names():
        _, W2, H2, a2, b2, f2 = fc.case(second)
        ref2 = _ref(oracle, second)
    else:   # the same frame size under the other algorithm (not a case of its own)
        form, size, content = second.split("-")
        W2, H2, f2 = W, H, form == "fb"
        a2, b2 = fc.make_pair(content, W, H)
        ref2 = oracle.calculate_flow(a2, b2, f2)
    assert (W2, H2) == (W, H)
    with mvs_amd.Context(W, H) as ctx:
        g1 = ctx.flow(a1, b1, f1)
        g2 = ctx.flow(a2, b2, f2)
        g3 = ctx.flow(a1, b1, f1)
    assert g1.tobytes() == g3.tobytes()
    np.testing.assert_array_equal(g1, _ref(oracle, first))
    np.testing.assert_array_equal(g2, ref2)


@pytest.mark.parametrize("W,H", [(60, 39), (2, 2)])
def test_farneback_without_a_window_is_refused(oracle, W, H):
    """H + W < 100: the window (H + W) / 100 is 0 and the box scale 1 / window^2 infinite -- MVS_EINVAL with a message that names the window,
    not a NaN map (error -1 is MVS_EINVAL); the context stays usable and the variational form valid at the same size"""
    z = np.zeros((H, W), np.uint8)
    with mvs_amd.Context(W, H) as ctx:
        with pytest.raises(mvs_amd.MvsError, match=r"error -1: .*window"):
            ctx.flow(z, z, True)
        with pytest.raises(ValueError, match="window"):
            oracle.calculate_flow(z, z, True)
        got = ctx.flow(z, z, False)
        with pytest.raises(mvs_amd.MvsError, match="window"):
            ctx.flow(z, z, True)
    assert not got.any()
    np.testing.assert_array_equal(got, oracle.calculate_flow(z, z, False))


def test_farneback_at_the_smallest_window_succeeds(oracle):
    """61 x 39: H + W = 100, window 1 -- the first size that is accepted"""
    _, W, H, a, b, _ = fc.case("fb-61x39-noise")
    with mvs_amd.Context(W, H) as ctx:
        got = ctx.flow(a, b, True)
    assert np.all(np.isfinite(got))
    np.testing.assert_array_equal(got, _ref(oracle, "fb-61x39-noise"))


def test_process_frame_refuses_farneback_without_a_window():
    """mvs_process_frame and mvs_process_frame_slots check the window up front, before the mesh, the frames or anything queued"""
    W, H = 60, 39
    cam = np.eye(4, dtype=np.float32)
    f = np.zeros((H, W), np.uint8)
    with mvs_amd.Context(W, H) as ctx:
        with pytest.raises(mvs_amd.MvsError, match=r"error -1: mvs_process_frame: .*window"):
            ctx.process_frame(cam, f, [cam], [f], use_farneback=True)
        with pytest.raises(mvs_amd.MvsError, match=r"error -1: mvs_process_frame_slots: .*window"):
            ctx.process_frame_slots(cam, 0, [cam], [1], use_farneback=True)
        # without Farneback the same calls get as far as the next check: no mesh is loaded
        with pytest.raises(mvs_amd.MvsError, match="no mesh loaded"):
            ctx.process_frame(cam, f, [cam], [f], use_farneback=False)
