"""Crafted inputs for flowRemap, compare() and the u8 resize (csrc/photometric.hip), numpy only, with plain numpy mirrors of what can be
stated without the oracle.  Shared by tests/test_photometric_cases_cpu.py and tests/test_photometric_cases_gpu.py.  Deterministic."""
import zlib

import numpy as np

REMAP_SIZES = ((65, 5), (64, 4), (301, 177))
REMAP_STRIDES = (2, 3, 4)
REMAP_IMAGES = ("checker", "ramp", "noise")
COMPARE_SIZES = ((2, 2), (3, 3), (5, 3), (2, 500), (8192, 2), (8192, 3), (33, 20), (128, 128), (130, 128), (129, 127))

SHORT = (32767.0, -32767.0, 40000.0, -40000.0)
# beyond the Q5 map's int32: 6e7 * 32 still fits (1.92e9), 7e7 * 32 does not; 3e38 * 32 is infinite in f32
HUGE = (6e7, -6e7, 7e7, -7e7, 1e12, -1e12, 1e19, -1e19, 3e38, -3e38, np.nan, np.inf, -np.inf)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(" ".join(str(k) for k in key).encode()))


def remap_image(kind, W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "checker":   # 0 / 255 squares of 3 pixels: the taps (0, 255, 255, 255) and (255, 0, 0, 0) that make the cubic overshoot
        return ((((xx // 3) + (yy // 3)) & 1) * 255).astype(np.uint8)
    if kind == "ramp":
        return ((xx * 5 + yy * 3) % 256).astype(np.uint8)
    if kind == "noise":
        return _rng("remap", W, H).integers(0, 256, (H, W), dtype=np.uint8)
    raise KeyError(kind)


def _targets(n):
    return np.array([-2.0, -1.0, -1.0 / 64, 0.0, n - 1, n - 1 + 1.0 / 64, n, n + 2], np.float64)


def remap_fields(W, H):
    """{name: (u, v)} flow components (f32, H x W) of the crafted fields; the sample position of pixel (x, y) is (x + u, y + v)"""
    yy, xx = np.mgrid[0:H, 0:W]
    i = yy * W + xx
    out = {}
    z = np.zeros((H, W), np.float32)
    r = _rng("integer", W, H)
    out["integer"] = (r.integers(-3, 4, (H, W)).astype(np.float32), r.integers(-3, 4, (H, W)).astype(np.float32))
    out["integer-far"] = (np.where(xx % 2 == 0, W - 1 - 2 * xx, -xx).astype(np.float32), np.where(yy % 2 == 0, H - 1 - 2 * yy, 1 - yy).astype(np.float32))
    # every 1/32 fraction and the 1/64 ties between them (k / 64, k = 0..63: odd k is a tie of round-half-to-even), both signs of the position
    if H >= 64:
        kx, ky = xx % 64, yy % 64
    else:
        kx, ky = (xx + 7 * yy) % 64, (3 * xx + yy) % 64
    out["fractions"] = ((kx / 64.0 - np.where(xx < 4, 6, 0)).astype(np.float32), (ky / 64.0 - np.where(xx % 16 == 5, 2 + yy, 0)).astype(np.float32))
    tx, ty = _targets(W), _targets(H)
    out["border-x"] = ((tx[(xx + yy) % 8] - xx).astype(np.float32), z)
    out["border-y"] = (z, (ty[(xx + yy) % 8] - yy).astype(np.float32))
    out["border-xy"] = ((tx[xx % 8] - xx).astype(np.float32), (ty[(xx // 8 + yy) % 8] - yy).astype(np.float32))
    s = np.array(SHORT, np.float32)
    out["short-x"] = (s[i % 4], z)
    out["short-y"] = (z, s[i % 4])
    out["short-xy"] = (s[i % 4], s[(i // 4) % 4])
    h = np.array(HUGE, np.float32)
    n = len(HUGE)
    out["huge-x"] = (h[i % n], z)
    out["huge-y"] = (z, h[i % n])
    out["huge-xy"] = (h[i % n], h[(i // n) % n])
    return out


ZERO_FIELDS = ("short-x", "short-y", "short-xy", "huge-x", "huge-y", "huge-xy")   # every sample lands in the border: output 0


def pack_flow(u, v, stride):
    """(u, v) -> H x W x stride; the channels flowRemap ignores carry NaN"""
    f = np.full(u.shape + (stride,), np.nan, np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def gather_zero_border(img, u, v):
    """numpy slicing with a zero border: out(x, y) = img(x + u, y + v) for integer u, v"""
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    sx, sy = xx + u.astype(np.int64), yy + v.astype(np.int64)
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return np.where(ok, img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], 0).astype(np.uint8)


def remap_mirror(u, v, img, table):
    """flowRemap restated in numpy on the Q15 table (1024 x 16 int16): returns (out u8, unclamped rounded sum int64).  Positions are x + u in
    f32, times 32 in f32, rounded half to even; what is no number or no int32 reads the border (0)."""
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        mx = (u.astype(np.float32) + xx.astype(np.float32)) * np.float32(32)
        my = (v.astype(np.float32) + yy.astype(np.float32)) * np.float32(32)
        ok = (mx >= np.float32(-2147483648.0)) & (mx < np.float32(2147483648.0)) & (my >= np.float32(-2147483648.0)) & (my < np.float32(2147483648.0))
    qx = np.rint(np.where(ok, mx, 0)).astype(np.int64)
    qy = np.rint(np.where(ok, my, 0)).astype(np.int64)
    sx, sy = np.clip((qx >> 5) - 1, -32767, 32767), np.clip((qy >> 5) - 1, -32767, 32767)
    wt = table.astype(np.int64)[(qy & 31) * 32 + (qx & 31)]
    total = np.zeros((H, W), np.int64)
    im = img.astype(np.int64)
    for k1 in range(4):
        for k2 in range(4):
            ys, xs = sy + k1, sx + k2
            inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
            total += np.where(inside, im[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)] * wt[..., k1 * 4 + k2], 0)
    val = np.where(ok, (total + (1 << 14)) >> 15, 0)
    return np.clip(val, 0, 255).astype(np.uint8), val


# ---- compare() --------------------------------------------------------------------------------------------------------------

def compare_levels(W, H):
    size, n = min(W, H), 0
    while True:
        n += 1
        if size <= 2:
            return n
        size //= 2


def compare_level_sizes(W, H):
    size, w, h, out = min(W, H), W, H, []
    while True:
        out.append((w, h))
        if size <= 2:
            return out
        w, h, size = (w + 1) // 2, (h + 1) // 2, size // 2


def compare_tail_start(W, H):
    """the first level that compare_batch_device hands to pyramid_tail (one workgroup for every level from there on): the first level
    after level 0 of at most 4096 cells, when at least one more level follows; None when every level runs in a launch of its own"""
    s = compare_level_sizes(W, H)
    for i in range(1, len(s)):
        if s[i][0] * s[i][1] <= 4096:
            return i if i < len(s) - 1 else None
    return None


def compare_pairs(W, H):
    """[(name, a, b, exact)]: exact = the value every pixel of compare(a, b) must have exactly, or None"""
    L = compare_levels(W, H)
    z = np.zeros((H, W), np.uint8)
    r = _rng("compare", W, H)
    tex = r.integers(0, 200, (H, W), dtype=np.uint8)
    out = [("identical", tex, tex.copy(), 0.0),
           ("offset7", np.full((H, W), 100, np.uint8), np.full((H, W), 107, np.uint8), 7.0 * L),
           ("const255", np.full((H, W), 255, np.uint8), z, 255.0 * L),
           ("texture-offset7", tex, (tex + 7).astype(np.uint8), None)]
    xo, yo = (W - 1) if (W - 1) % 2 else W - 2, (H - 1) if (H - 1) % 2 else H - 2   # the last odd column and row
    for name, (x, y) in (("impulse-tl", (0, 0)), ("impulse-tr", (W - 1, 0)), ("impulse-bl", (0, H - 1)), ("impulse-br", (W - 1, H - 1)),
                         ("impulse-centre", (W // 2, H // 2)), ("impulse-last-odd", (xo, yo))):
        b = z.copy()
        b[y, x] = 255
        out.append((name, z, b, None))
    out.append(("noise", r.integers(0, 256, (H, W), dtype=np.uint8), r.integers(0, 256, (H, W), dtype=np.uint8), None))
    return out


# ---- resize -----------------------------------------------------------------------------------------------------------------

def _up(n):
    return {1: 4, 2: 7}.get(n, int(n * 3.7))   # 2 -> 7 (3.5), 7 -> 25 (3.57), 333 -> 1232, 211 -> 780 (3.70)


def resize_cases():
    """[(name, img, dw, dh)]"""
    out = []
    for (sw, sh, ch) in ((1, 1, 1), (1, 7, 1), (7, 1, 1), (2, 2, 1), (2, 2, 3), (333, 211, 3)):
        img = _rng("resize", sw, sh, ch).integers(0, 256, (sh, sw) if ch == 1 else (sh, sw, ch), dtype=np.uint8)
        dsts = [(1, 1), (1, 5), (5, 1), (sw, sh), (_up(sw), _up(sh))]   # the last: a non-integer factor above 3 wherever the length allows one
        if (sw, sh) == (333, 211):
            dsts += [(1, 211), (333, 1)]
        for (dw, dh) in dict.fromkeys(dsts):   # (the identity of a 1 x 1 source is its 1 x 1 destination)
            out.append(("%dx%dx%d-to-%dx%d" % (sw, sh, ch, dw, dh), img, dw, dh))
    return out
