"""Crafted cameras for the sweep kernels ("Crafted cameras"): inputs that sit on the edges of the parity contracts on
purpose.  The main camera is the identity, so a side camera's clip matrix IS the T of section 2 and Q = S T has dyadic entries: every sample
position of an affine case is an exact float32 number and can be placed on the frame test's bounds, on a rounding tie or on a table
entry.  Planes are plane_table(D, -1, 1); frames are seeded noise unless a case names others.

For a side camera with x row (a, 0, s, t), y row (0, b, s', t') and w row (0, 0, 0, 1) the contract's numbers are
    cx = W/2 + 1/2 + a (col + 1/2 - W/2) + (W/2)(s z + t)          ux = 256 cx + 4
    cy = H/2 + 1/2 + b (row + 1/2 - H/2) - (H/2)(s' z + t')        uy = 256 cy + 4
and with D = 16 the planes are z_d = (2 d - 15) / 16.

Each case carries `premise(case, m)`, a check over the mirror's numbers that the case is what it is there for (m: the dictionary of
`mirror_of`), and `plan_premise(case, plan)`, the same over the planner's descriptors of the device (`read_plan` of an MVS_PLAN_DUMP file).
tests/window_cameras.py reuses the ladders, shear_tie, horizon, axial, checker_extreme, skip_then_border, one_plane and ragged_shear for
the windowed sweeps, the band sweeps and the propagation, with premises of its own over the windows, and adds the cases those kernels need."""
import functools
from fractions import Fraction

import numpy as np

import sweep_mirror as sm

F = np.float32
SKIP, FAST, BORDER, GENERIC = 0, 1, 2, 3
FX_MAX_RW, FX_ROWS, FX_HALF = 224, 32, 112          # the fixed sampler's staging image: 224 quads x 32 rows, two halves of 112
EX_MAX_RW, EX_LDS_QUADS = 192, 5120                 # the exact sampler's: at most 192 quads wide, pitch x rows <= 5120


def cam(x=(1, 0, 0, 0), y=(0, 1, 0, 0), w=(0, 0, 0, 1)):
    """a side camera's clip matrix from its x, y and w rows (the z row plays no part in the sweep)"""
    return np.array([x, y, (0, 0, 1, 0), w], np.float64)


def designed_q(side, W, H):
    """Q = S T of section 2 for the identity main camera, in double precision; asserts that every entry is a float32 number already"""
    T = np.asarray(side, np.float64)
    hw, hh = 0.5 * W, 0.5 * H
    Q = np.stack([hw * T[0] + (hw + 0.5) * T[3], -hh * T[1] + (hh + 0.5) * T[3], T[3]])
    assert (Q.astype(F).astype(np.float64) == Q).all(), "the case's view matrix is not exactly representable"
    return Q.astype(F)


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def checkerboard(W, H, phase=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((xx + yy + phase) & 1) * 255).astype(np.uint8)


def constant(W, H, v):
    return np.full((H, W), v, np.uint8)


class Case:
    def __init__(self, name, W, H, D, cams, frames="noise", premise=None, plan_premise=None, exact_plan_premise=None, rect=False, tile=None):
        self.name, self.W, self.H, self.D = name, W, H, D
        self.cams = [np.asarray(c, np.float64) for c in cams]
        self.V = len(self.cams)
        self.frames_kind = frames
        self.premise, self.plan_premise, self.exact_plan_premise = premise, plan_premise, exact_plan_premise
        self.rect = rect          # pure shifts: the rectified kernels take the default path (plan_shape 4 resp. 5)
        self.tile = tile          # the tile a plan premise looks at
        assert W <= 256 and H <= 64 and D <= 48 and W * H * D * min(self.V, 8) <= 256 * 64 * 48 * 8

    @property
    def main_cam(self):
        return np.eye(4, dtype=F)

    @property
    def side_cams(self):
        return np.stack(self.cams).astype(F)

    def q(self):
        return np.stack([designed_q(c, self.W, self.H) for c in self.cams])

    def z(self):
        return sm.plane_table(self.D, -1.0, 1.0)

    def frames(self):
        """(main, [sides])"""
        W, H, V = self.W, self.H, self.V
        seed = sum(map(ord, self.name)) * 7919 + W * 31 + H
        k = self.frames_kind
        if k == "noise":
            return noise(W, H, seed), [noise(W, H, seed + 1 + v) for v in range(V)]
        if k == "checker":
            return noise(W, H, seed), [checkerboard(W, H, v) for v in range(V)]
        if k == "constant":
            return constant(W, H, 90), [constant(W, H, 200) for _ in range(V)]
        if k == "extremes":
            return constant(W, H, 0), [constant(W, H, 255)] * V
        if k == "stripes":      # view 0: alternating 0 / 1 columns, view 1: alternating rows, the rest: noise
            yy, xx = np.mgrid[0:H, 0:W]
            return noise(W, H, seed), [(xx & 1).astype(np.uint8), (yy & 1).astype(np.uint8)] + [noise(W, H, seed + v) for v in range(2, V)]
        if k == "period4":      # side frames of column period 4: with a shift of one texel per plane, planes d and d + 4 see the same texels
            return noise(W, H, seed), [np.tile(noise(4, H, seed + 1 + v), (1, W // 4)) for v in range(V)]
        raise KeyError(k)


@functools.lru_cache(maxsize=None)
def mirror_of(name, sampler):
    """the mirror's results of a case, computed once per process and never modified: dict(depth, cost, index, volume, views, q, z)"""
    c = CASES[name]
    main, sides = c.frames()
    q, z = c.q(), c.z()
    depth, cost, index, vol, views = sm.sweep(q, z, main, sides, sampler=sampler, details=True)
    for a in (depth, cost, index, vol):
        a.setflags(write=False)
    return dict(depth=depth, cost=cost, index=index, volume=vol, views=views, q=q, z=z)


def counts(m, sampler):
    return np.asarray(m["volume"]) >> (24 if sampler == "fixed" else 16)


# ---- the planner's descriptors -------------------------------------------------------------------------------------------------------
def read_plan(path):
    """an MVS_PLAN_DUMP file (either sampler's) -> structured array [tiles_y, tiles_x, nchunks, V] with fields mode, x0, y0, rw, rh"""
    raw = np.fromfile(path, dtype=np.uint32)
    tx, ty, nc, V = (int(v) for v in raw[:4])
    d = raw[4:].reshape(ty, tx, nc, V, 2)
    out = np.zeros((ty, tx, nc, V), dtype=[("mode", "i4"), ("x0", "i4"), ("y0", "i4"), ("rw", "i4"), ("rh", "i4")])
    out["x0"], out["y0"] = d[..., 0] & 0xffff, d[..., 0] >> 16
    out["rw"], out["rh"], out["mode"] = d[..., 1] & 0xff, (d[..., 1] >> 8) & 0xff, (d[..., 1] >> 16) & 7
    return out


def staged(plan):
    return plan[(plan["mode"] == FAST) | (plan["mode"] == BORDER)]


# ---- premises ------------------------------------------------------------------------------------------------------------------------
def _ladder(W, H, D, edge, tie):
    """x or y row (1, 0, s, t) whose border pixel steps through the frame test's bound: by 2 per plane through lo - 2, lo, lo + 2 (hi
    likewise), or with half the slope by 1 through lo - 1.5 ... lo + 1.5"""
    g = Fraction(1, 2) if tie else Fraction(1)             # u advances by 2 g per plane
    o = 128 if tie else 127
    if edge in ("left", "right"):
        s, t = g * D / (128 * W), Fraction(-o if edge == "left" else o, 128 * W)
        return cam(x=(1, 0, float(s), float(t)))
    s, t = -g * D / (128 * H), Fraction(o if edge == "top" else -o, 128 * H)
    return cam(y=(0, 1, float(s), float(t)))


def _border_pixel(c, edge):
    return {"left": (0, 0, 0), "right": (c.W - 1, 0, 0), "top": (0, 0, 1), "bottom": (0, c.H - 1, 1)}[edge]   # col, row, axis


def _ladder_premise(edge, tie):
    def premise(c, m):
        col, row, axis = _border_pixel(c, edge)
        q, z = m["q"][0], m["z"]
        lo_side = edge in ("left", "top")
        bound = 132 if lo_side else 256 * (c.W if axis == 0 else c.H) + 132
        us = [sm.exact_u(q, col, row, z[d], c.W, c.H, axis) for d in range(c.D)]
        view = m["views"][0]
        u = view["ux" if axis == 0 else "uy"]
        cnt = counts(m, "fixed")[:, row, col]
        k = c.D // 2 - 1 if lo_side else c.D // 2          # the plane that sits on the bound
        inward = k + 1 if lo_side else k - 1
        if tie:
            assert view["tie_x" if axis == 0 else "tie_y"].all(), "every sample of the view is an exact tie"
            seen = [us[d] - bound for d in range(k - 1, k + 3)] if lo_side else [us[d] - bound for d in range(k - 2, k + 2)]
            assert seen == [Fraction(-3, 2), Fraction(-1, 2), Fraction(1, 2), Fraction(3, 2)], seen
            # round to even: bound - 1.5 -> bound - 2, bound - 0.5 -> bound, bound + 0.5 -> bound, bound + 1.5 -> bound + 2
            d0 = k - 1 if lo_side else k - 2
            assert [int(u[d, row, col]) - bound for d in range(d0, d0 + 4)] == [-2, 0, 0, 2]
            assert list(cnt[d0:d0 + 4]) == ([0, 0, 0, 1] if lo_side else [1, 0, 0, 0])
        else:
            assert us[k] == bound and us[inward] == bound + (2 if lo_side else -2), (us[k], us[inward])
            assert cnt[k] == 0 and cnt[inward] == 1
            assert list(cnt) == ([0] * (k + 1) + [1] * (c.D - k - 1) if lo_side else [1] * k + [0] * (c.D - k))
    return premise


def _ladder_end(W, D, edge):
    """the ladder moved so that the bound is hit on an END plane of the chunk: u(0, d) = 132 + 2 d resp. u(W - 1, d) = hi - 30 + 2 d (D = 16).
    The BORDER regions' row shortcut looks at exactly these two planes."""
    return cam(x=(1, 0, D / (128.0 * W), (-113.0 if edge == "left" else 113.0) / (128 * W)))


def _ladder_end_premise(edge):
    def premise(c, m):
        col, row, _ = _border_pixel(c, edge)
        us = [sm.exact_u(m["q"][0], col, row, m["z"][d], c.W, c.H) for d in range(c.D)]
        cnt = list(counts(m, "fixed")[:, row, col])
        if edge == "left":
            assert us[0] == 132 and us[1] == 134 and cnt == [0] + [1] * 15
        else:
            assert us[15] == 256 * c.W + 132 and us[14] == 256 * c.W + 130 and cnt == [1] * 15 + [0]
    return premise


def _shear_premise(c, m):
    v = m["views"][0]
    assert m["q"][0][0, 1] != 0, "q1 != 0: neither a rectified nor a separable view"
    assert v["tie_x"].all(), "every sample is an exact tie in x"
    us = [sm.exact_u(m["q"][0], 0, c.H - 1, m["z"][d], c.W, c.H) for d in range(c.D)]
    assert all(u.denominator == 2 for u in us)


def _skip_premise(c, m):
    cnt = counts(m, "fixed")
    assert not cnt[:16].any() and cnt[16:32].any() and not cnt[16:32].all(), "nothing in frame on planes 0..15, part of the frame on 16..31"
    assert (np.asarray(m["volume"])[:16] == 0).all()


def _skip_plan(c, plan):
    assert (plan["mode"][:, :, 0, :] == SKIP).all(), "every tile of chunk 0 is skipped"
    later = plan["mode"][:, :, 1:, :]
    assert ((later == BORDER) | (later == FAST)).any() and not (later == GENERIC).any()


def _horizon_premise(c, m):
    q = m["q"][0]
    sw = sm.project(q, m["z"], c.W, c.H)[2]
    assert (sw[:, :, 15] == 0).all() and (sw[:, :, :15] < 0).all() and (sw[:, :, 16:] > 0).all(), "s.w is 0 exactly at column 15"
    cnt = counts(m, "fixed")
    assert not cnt[:, :, :16].any() and (cnt[:, :, 16:] == 1).all()


def _horizon_plan(c, plan):
    assert (plan["mode"] == GENERIC).all() and not plan["rw"].any(), "GENERIC by `behind` (an oversize region would carry no size either; the frame is 64 wide)"


def _axial_premise(c, m):
    for q in m["q"]:
        assert q[0, 1] == 0 and q[1, 0] == 0 and q[2, 0] == 0 and q[2, 1] == 0 and q[2, 2] != 0
    sw = sm.project(m["q"][0], m["z"], c.W, c.H)[2]
    assert len(np.unique(sw)) == c.D, "r depends on the plane and on nothing else"


def _axial_plan(c, plan):
    assert (plan["mode"] == FAST).any()


def _zoom_plan(wide, exact):
    def check(c, plan):
        st = staged(plan)
        over = plan[(plan["mode"] == GENERIC)]
        assert len(over) and len(st), "an oversize region and a staged one"
        if not exact:
            assert (st["rw"].max() == FX_MAX_RW) if wide else (st["rh"].max() == FX_ROWS), (st["rw"].max(), st["rh"].max())
        elif wide:
            assert st["rw"].max() == EX_MAX_RW, st["rw"].max()
        else:
            pitch = (st["rw"] + 31) & ~31
            assert (pitch * st["rh"] <= EX_LDS_QUADS).all() and (pitch * (st["rh"] + 1) > EX_LDS_QUADS).any(), "the tallest region that fits the staging buffer"
    return check


LOOKAHEAD_TILE = (0, 1)     # tiles_y, tiles_x
LOOKAHEAD_SEQUENCE = ("narrow FAST", "narrow FAST", "wide", "SKIP", "narrow BORDER", "GENERIC", "narrow FAST", "narrow FAST")


def _lookahead_plan(c, plan):
    ty, tx = LOOKAHEAD_TILE
    for chunk in range(plan.shape[2]):
        got = []
        for d in plan[ty, tx, chunk]:
            mode, rw = int(d["mode"]), int(d["rw"])
            if mode == SKIP:
                got.append("SKIP")
            elif mode == GENERIC:
                got.append("GENERIC")
            elif rw >= FX_HALF + 4:
                got.append("wide")
            else:
                assert rw <= FX_HALF
                got.append("narrow FAST" if mode == FAST else "narrow BORDER")
        assert tuple(got) == LOOKAHEAD_SEQUENCE, (chunk, got)


def _lookahead_premise(c, m):
    sw = sm.project(m["q"][5], m["z"], c.W, c.H)[2]
    assert (sw[:, :, 95] == 0).all() and (sw[:, :, 96:] > 0).all() and (sw[:, :, :95] < 0).all(), "view 5: s.w changes sign inside tile 1"


def _first_in_frame(c, m, sampler="fixed"):
    cnt = counts(m, sampler)
    return np.where(cnt.any(axis=0), (cnt > 0).argmax(axis=0), -1)


def _ties_premise(edge):
    def premise(c, m):
        first = _first_in_frame(c, m)
        col, row, axis = _border_pixel(c, edge)
        k = {17: 8, 33: 16}[c.D]                    # the first plane whose rounded u exceeds 132 (D = 17: 132.06 -> 132 on plane 7; D = 33: 132.03 on plane 15)
        want = np.zeros((c.H, c.W), np.int64)
        if axis == 0:
            want[:, col] = k
        else:
            want[row, :] = k
        assert (first == want).all()
        assert (m["index"] == want).all(), "every cost ties: the lowest plane with a view in frame"
        assert len(np.unique(m["cost"])) == 1
    return premise


def _periodic_premise(c, m):
    vol, idx = np.asarray(m["volume"]), m["index"]
    inner = slice(64, 192)                            # the two interior tile columns: every plane in frame (shifts of at most 15.5 texels)
    assert (counts(m, "fixed")[:, :, inner] == c.V).all()
    for d in range(c.D - 4):
        assert (vol[d, :, inner] == vol[d + 4, :, inner]).all(), "planes d and d + 4 tie cell by cell"
    assert (idx[:, inner] < 4).all() and len(np.unique(idx[:, inner])) == 4, "of eight equal minima the lowest plane wins"


def _periodic_plan(c, plan):
    assert (plan["mode"][:, 1:3] == FAST).all()


def _half_up_premise(c, m):
    mx = mirror_of(c.name, "exact")
    W, H, D = c.W, c.H, c.D
    v0, v1, v2 = mx["views"][:3]
    # view 0: cx = col + 1.5 on columns 0, 1, 0, 1 ...: in frame for col <= W - 2, bilinear = 1/2 everywhere; view 1 likewise in y
    assert v0["valid"].sum() == (W - 1) * H * D and (v0["half"] == v0["valid"]).all()
    assert v1["valid"].sum() == W * (H - 1) * D and (v1["half"] == v1["valid"]).all()
    assert (v0["Iq"][v0["valid"]] == 1).all() and (v1["Iq"][v1["valid"]] == 1).all(), "trunc(1/2 + 1/2) = 1: the half rounds up"
    cx = v2["cx"][v2["valid"]]
    assert len(cx) and (cx == np.trunc(cx)).all() and not v2["half"].any(), "view 2: c is an integer (a = 0)"


def _checker_premise(c, m):
    seen = np.zeros((32, 32), bool)
    for v in m["views"]:
        ok = v["valid"]
        seen[v["ky"][ok], v["kx"][ok]] = True
    assert seen.all(), "%d of 1024 table entries are never used" % (1024 - seen.sum())
    assert m["q"][0][0, 1] != 0


def _max_cells_premise(c, m):
    vol = np.asarray(m["volume"])
    assert (vol == ((255 << 24) | 0xFD02FF)).all(), "every cell: 255 views in frame, each |65025 - 0|"


def _max_cells_plan(c, plan):
    assert (plan["mode"] == FAST).all()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
CASES = {}


def _add(case):
    assert case.name not in CASES
    CASES[case.name] = case


for _W, _H in ((64, 8), (256, 16)):
    _sz = "" if _W == 64 else "_%dx%d" % (_W, _H)
    for _edge in ("left", "right", "top", "bottom"):
        _add(Case("ladder_int_%s%s" % (_edge, _sz), _W, _H, 16, [_ladder(_W, _H, 16, _edge, False)], premise=_ladder_premise(_edge, False), rect=True))
        _add(Case("ladder_tie_%s%s" % (_edge, _sz), _W, _H, 16, [_ladder(_W, _H, 16, _edge, True)], premise=_ladder_premise(_edge, True), rect=True))
    for _edge in ("left", "right"):
        _add(Case("ladder_end_%s%s" % (_edge, _sz), _W, _H, 16, [_ladder_end(_W, 16, _edge)], premise=_ladder_end_premise(_edge), rect=True))
    # ux = 256 (col + 1) + 4 + 128 yn + 8 z - 128: 128 yn and 8 z = (2 d - 15) / 2 put every sample on k + 1/2
    _add(Case("shear_tie" + _sz, _W, _H, 16, [cam(x=(1, 128.0 / (128 * _W) * 1.0, 16.0 / (256 * _W), -128.0 / (128 * _W)))], premise=_shear_premise))
    for _D in (17, 33):
        for _edge in ("left", "top"):
            _add(Case("ties_constant_%s_D%d%s" % (_edge, _D, _sz), _W, _H, _D, [_ladder(_W, _H, 16, _edge, False)], frames="constant", premise=_ties_premise(_edge), rect=True))

# ragged, not dyadic: the same rows, no exact premises
_add(Case("ragged_shift", 200, 20, 17, [_ladder(64, 8, 16, "left", False), _ladder(64, 8, 16, "top", True)], rect=True))
_add(Case("ragged_shear", 200, 20, 33, [cam(x=(1, 1 / 64, 1 / 1024, -1 / 64), y=(1 / 32, 1, 1 / 256, 1 / 128)), cam(x=(0.75, 0, 1 / 8, 0), y=(0, 1.25, 0, 1 / 16), w=(0, 0, 0.25, 1))]))
_add(Case("one_plane", 64, 8, 1, [_ladder(64, 8, 16, "left", True), cam(x=(1, 1 / 64, 0, 1 / 256))]))

# ux = 256 (col + 1) + 4 + 256 (d - 15.5): one texel per plane on frames of period 4, so every cost occurs on eight planes -- four in each
# chunk of 16: the minimum of a chunk has three equals above it (min-key selection), and the second chunk ties with the first (strict comparison)
_add(Case("ties_periodic", 256, 16, 32, [cam(x=(1, 0, 1 / 8, 0)), cam(x=(1, 0, 1 / 8, 1 / 64))], frames="period4", premise=_periodic_premise, plan_premise=_periodic_plan, rect=None))

# cx = col + 1 + 128 z - 64: planes 0..15 (z <= -2/33) leave the frame to the left, 16..31 cross it, 32 is partly in
_add(Case("skip_then_border", 64, 8, 33, [cam(x=(1, 0, 4, -2))], premise=_skip_premise, plan_premise=_skip_plan, exact_plan_premise=None))

# s.w = 64 xn + 33 = 2 (col - 15); cx = 32.5 + (32 xn + 16 z) / s.w, cy = 4.5 - 8 yn / s.w: in frame wherever s.w > 0
_add(Case("horizon", 64, 8, 16, [cam(x=(1, 0, 0.5, 0), y=(0, 2, 0, 0), w=(64, 0, 0, 33))], premise=_horizon_premise, plan_premise=_horizon_plan, exact_plan_premise=_horizon_plan))

# s.w = 1 + z / 4 = (49 + 2 d) / 64
_add(Case("axial", 256, 16, 16, [cam(w=(0, 0, 0.25, 1)), cam(x=(0.75, 0, 0, 1 / 64), y=(0, 0.75, 0, 0), w=(0, 0, 0.25, 1))], premise=_axial_premise, plan_premise=_axial_plan,
          exact_plan_premise=_axial_plan))

_add(Case("zoom_wide", 256, 16, 16, [cam(x=(a, 0, 1 / 512, t)) for a, t in ((3.5, 0.75), (4.5, 0.8125), (3.0, 0.75), (3.0625, 0.75))], plan_premise=_zoom_plan(True, False),
          exact_plan_premise=_zoom_plan(True, True)))
_add(Case("zoom_tall", 64, 64, 16, [cam(y=(0, b, 1 / 512, t)) for b, t in ((4.375, 0.25), (4.5, 0.25), (3.5, 0.75), (4.375, 0.75), (8.0, -1.0))],
          plan_premise=_zoom_plan(False, False), exact_plan_premise=_zoom_plan(False, True)))

_NARROW = [cam(x=(0.5, 0, 1 / 256, 0)), cam(x=(0.5, 1 / 64, 1 / 512, 1 / 8), y=(0, 0.75, 0, 0))]
_add(Case("lookahead_order", 256, 16, 33,
          [_NARROW[0], _NARROW[1],
           cam(x=(2, 0, 1 / 256, 0.5)),                                   # wide: tile 1 lands on texels 64 .. 192
           cam(x=(1, 0, 0, 4)),                                           # 512 texels to the right: nothing in frame
           cam(x=(1, 0, 1 / 256, -0.75)),                                 # 96 texels to the left: tile 1 straddles the left edge
           cam(x=(1, 0, 0.5, 0), w=(256, 0, 0, 65)),                      # s.w = 2 (col - 95)
           cam(x=(0.5, 0, -1 / 256, -1 / 8), y=(1 / 64, 1, 0, 0)), _NARROW[0]],
          premise=_lookahead_premise, plan_premise=_lookahead_plan, tile=LOOKAHEAD_TILE))

# x shifts of 1/2 and of 1 texel, a y shift of 1/2: 32 t = 1/2, 4 t = 1/2
_add(Case("half_up", 64, 8, 16, [cam(x=(1, 0, 0, 1 / 64)), cam(y=(0, 1, 0, -1 / 8)), cam(x=(1, 0, 0, 1 / 32))], frames="stripes", premise=_half_up_premise, rect=True))

# ux = 264 col - 32 row - 8 + (2 d - 15) / 2, uy = 264 row + 232 + 64 (d - 1.5): kx advances by 1 per column (scale 33/32) and by 4 per row
# (the shear), ky by 1 per row and by 8 per plane, and planes 0..3 are in frame on every row; ties in x as in shear_tie
_add(Case("checker_extreme", 64, 8, 16, [cam(x=(33 / 32, 1 / 64, 1 / 1024, -1 / 64), y=(0, 33 / 32, -1 / 2, -3 / 8))], frames="checker", premise=_checker_premise))

# 255 copies of one view that is in frame everywhere (ux = 256 (col + 1) + 4 + 2 d - 15): main 0, sides 255
_add(Case("max_cells", 64, 8, 16, [cam(x=(1, 0, 1 / 512, 0))] * 255, frames="extremes", premise=_max_cells_premise, plan_premise=_max_cells_plan, exact_plan_premise=None, rect=True))

D33 = sorted(n for n, c in CASES.items() if c.D == 33)
