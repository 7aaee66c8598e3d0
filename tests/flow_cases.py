"""Crafted frame pairs for calculateFlow (csrc/flow.hip), numpy only: contents that make the arithmetic degenerate, at the sizes where the
dispatch of the Farneback iteration and the variational solver's tiling change.  Shared by tests/test_flow_cases_cpu.py (the oracle alone:
every case reaches what it claims) and tests/test_flow_cases_gpu.py (mvs_flow against the oracle, bit for bit).  Deterministic."""
import zlib

import numpy as np

CONTENTS = ("zeros", "const", "checker", "step", "saturated", "impulse", "noise", "shifted", "identical")
ZERO_FLOW_VARIATIONAL = ("zeros", "const", "checker", "identical")   # flow exactly 0.0 under the variational form ...
ZERO_FLOW_FARNEBACK = ("zeros", "const", "checker")                  # ... and under Farneback (`identical` is only compared there)

# Farneback sizes: (W, H) -> the shift of its `shifted` pair (None: the plain shift below), chosen so that the flow leaves the frame
FARNEBACK_ALL = {(61, 39): None, (60, 40): None, (129, 65): None, (333, 201): (-6, 5), (400, 399): (-12, 9), (401, 399): (-12, 9)}
FARNEBACK_FEW = {(979, 520): (-12, 9), (980, 520): (-12, 9), (8127, 72): (-6, 4)}   # `noise`, `saturated`, `shifted` only
FARNEBACK_THREE_LAUNCH = {(8128, 72): (-6, 4)}                                       # `noise`, `shifted` only
SHIFTED_SIZES = tuple(s for t in (FARNEBACK_ALL, FARNEBACK_FEW, FARNEBACK_THREE_LAUNCH) for s, shift in t.items() if shift is not None)
PLAIN_SHIFT = (2.5, -1.5)
VARIATIONAL_SIZES = ((2, 2), (5, 3), (9, 9), (11, 11), (63, 27), (64, 28), (65, 29), (74, 38), (84, 48), (85, 49), (129, 57))

FB_MAXM = 40                 # csrc/flow.hip: the largest window radius of the fused iteration
VT_W, VT_H, VT_HALO = 64, 28, 10   # csrc/flow.hip: the variational solver's tile and its halo


def texture_pair(W, H, dx, dy, seed=0):
    """the smooth three-sinusoid texture with sigma = 2 noise of tests/test_flow_gpu.py, and itself shifted by (dx, dy)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def tex(x, y):
        return 127 + 50 * np.sin(x / 7.0) * np.cos(y / 9.0) + 40 * np.sin((x + y) / 13.0) + 30 * np.cos((x - 2 * y) / 17.0)
    a = (tex(xx, yy) + rng.normal(0, 2, (H, W))).clip(0, 255).astype(np.uint8)
    b = (tex(xx - dx, yy - dy) + rng.normal(0, 2, (H, W))).clip(0, 255).astype(np.uint8)
    return a, b


def make_pair(content, W, H, shift=None):
    seed = zlib.crc32(("%s %d %d" % (content, W, H)).encode())
    rng = np.random.default_rng(seed)
    z = np.zeros((H, W), np.uint8)
    if content == "zeros":
        return z, z.copy()
    if content == "const":
        return np.full((H, W), 255, np.uint8), z
    if content == "checker":   # 1-pixel checkerboard against its inverse
        yy, xx = np.mgrid[0:H, 0:W]
        a = (((xx + yy) & 1) * 255).astype(np.uint8)
        return a, (255 - a).astype(np.uint8)
    if content == "step":      # vertical 0 / 255 edge at W // 2, against itself rolled by 3 columns
        a = z.copy()
        a[:, W // 2:] = 255
        return a, np.roll(a, 3, axis=1)
    if content == "saturated":  # random 0 / 255 field against itself rolled by 2 columns
        a = (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)
        return a, np.roll(a, 2, axis=1)
    if content == "impulse":   # all 0 against one 255 pixel at the centre
        b = z.copy()
        b[H // 2, W // 2] = 255
        return z, b
    if content == "noise":     # two independent uniform fields
        return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    if content == "shifted":
        dx, dy = PLAIN_SHIFT if shift is None else shift
        return texture_pair(W, H, dx, dy, seed=W)
    if content == "identical":
        a, _ = texture_pair(W, H, 0, 0, seed=W)
        return a, a.copy()
    raise KeyError(content)


def cases():
    """[(name, W, H, prev, next, farneback)]; the name is unique and is the test id"""
    out = []

    def add(content, W, H, farneback, shift=None):
        a, b = make_pair(content, W, H, shift)
        out.append(("%s-%dx%d-%s" % ("fb" if farneback else "var", W, H, content), W, H, a, b, farneback))
    for (W, H), shift in FARNEBACK_ALL.items():
        for c in CONTENTS:
            add(c, W, H, True, shift)
    for (W, H), shift in FARNEBACK_FEW.items():
        for c in ("noise", "saturated", "shifted"):
            add(c, W, H, True, shift)
    for (W, H), shift in FARNEBACK_THREE_LAUNCH.items():
        for c in ("noise", "shifted"):
            add(c, W, H, True, shift)
    for (W, H) in VARIATIONAL_SIZES:
        for c in CONTENTS:
            add(c, W, H, False)
    return out


def case_names():
    """the names of cases(), without building the pairs (for parametrisation)"""
    names = []
    for (W, H) in FARNEBACK_ALL:
        names += ["fb-%dx%d-%s" % (W, H, c) for c in CONTENTS]
    for (W, H) in FARNEBACK_FEW:
        names += ["fb-%dx%d-%s" % (W, H, c) for c in ("noise", "saturated", "shifted")]
    for (W, H) in FARNEBACK_THREE_LAUNCH:
        names += ["fb-%dx%d-%s" % (W, H, c) for c in ("noise", "shifted")]
    for (W, H) in VARIATIONAL_SIZES:
        names += ["var-%dx%d-%s" % (W, H, c) for c in CONTENTS]
    return names


def case(name):
    """one case of cases() by its name"""
    form, size, content = name.split("-")
    W, H = (int(v) for v in size.split("x"))
    farneback = form == "fb"
    shift = None
    if farneback:
        for t in (FARNEBACK_ALL, FARNEBACK_FEW, FARNEBACK_THREE_LAUNCH):
            shift = t.get((W, H), shift)
    a, b = make_pair(content, W, H, shift)
    return name, W, H, a, b, farneback


def content_of(name):
    return name.split("-")[2]


def compare_levels(W, H):
    """levels of compare()'s pyramid (util.cpp:335,341-351), as tests/test_photometric_cpu.py counts them"""
    size, n = min(W, H), 0
    while True:
        n += 1
        if size <= 2:
            return n
        size //= 2


def farneback_geometry(W, H, num_cus=256):
    """what flow_run / farneback_run / launch_fb_iteration of csrc/flow.hip derive from the frame size, restated: window, radius m, poly_n,
    pyramid levels below level 0, and per level (0 = finest) the form of the iteration:
    "fused" (m < 4), "tiled 64x16" / "tiled 64x8" (m <= FB_MAXM; tall where a level has >= 2 * num_cus tiles of 64 x 16), "three-launch" beyond."""
    winsize = (H + W) // 100
    m = winsize // 2
    poly_sigma = (H + W) / 1000.0
    poly_n = 5 if poly_sigma < 1.5 else 7
    levels, scale = 0, 1.0
    for k in range(10):
        scale *= 0.8
        if W * scale < 32 or H * scale < 32:
            break
        levels = k + 1
    sizes, forms = [], []
    for k in range(levels + 1):
        scale = 1.0
        for _ in range(k):
            scale *= 0.8
        w, h = int(np.rint(W * scale)), int(np.rint(H * scale))
        sizes.append((w, h))
        if m > FB_MAXM:
            forms.append("three-launch")
        elif m < 4:
            forms.append("fused")
        else:
            tiles = -(-w // 64) * -(-h // 16)
            forms.append("tiled 64x16" if tiles >= 2 * num_cus else "tiled 64x8")
    lds = 0
    if 4 <= m <= FB_MAXM:   # dynamic LDS of the largest tiled launch: ty * 5 * (cols + cols / px + 1) doubles
        cols = 64 + 2 * m
        lds = max((16 * 5 * (cols + cols // 4 + 1) if f == "tiled 64x16" else 8 * 5 * (cols + cols // 2 + 1)) * 8 for f in forms)
    return dict(winsize=winsize, m=m, poly_n=poly_n, levels=levels, sizes=sizes, forms=forms, lds_bytes=lds)


def outside_share(flow, W, H):
    """share of pixels whose target (x + u, y + v) lies outside the frame [0, W - 1] x [0, H - 1]"""
    yy, xx = np.mgrid[0:H, 0:W]
    tx, ty = xx + flow[..., 0].astype(np.float64), yy + flow[..., 1].astype(np.float64)
    return float(np.mean((tx < 0) | (tx > W - 1) | (ty < 0) | (ty > H - 1)))
