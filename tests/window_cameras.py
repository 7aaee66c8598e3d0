"""Crafted cameras for the windowed sweeps and the propagation ("Crafted cameras for the windowed kernels"): the cases of
tests/sweep_cameras.py that put a sample ON the frame test's bounds, on a rounding tie or on s.w == 0, and cases of their own at the
edges of the window arithmetic.  Every kernel that carries a copy of the fixed sampler (zncc.hip, bestk.hip for the table and band
sweeps, bestk_gated.hip, propagate.hip through zncc_sample / absdiff_sample; band.hip through absdiff_sample) runs on them.

The samples come from tests/sweep_mirror.py alone (sample_fixed: the contract of section 2b restated without the oracle), on the plane
table or, for the band sweeps, on the per-pixel plane map prior + offset.  On top of them stand the PURE functions of the windowed
mirrors -- zncc_mirror.view_cost / box / cells, bestk_mirror.merge, gated_mirror.gates / view_costs, band_mirror.planes / resolve / report
-- and sweep_mirror.select, so nothing here calls the C oracle.  tests/test_window_cases_cpu.py holds the oracle entries the windowed
mirrors stand on against the same samples.

Each case carries `premise(case)`, a check over these numbers that the case is what it is there for.  Results are computed once per
process and are read-only."""
import functools
from fractions import Fraction

import numpy as np

import band_mirror as bm
import bestk_mirror as km
import gated_mirror as gm
import sweep_cameras as sc
import sweep_mirror as sm
import zncc_mirror as zm

F = np.float32
ABSDIFF, ZNCC, KEEP_ALL = km.COST_ABSDIFF, km.COST_ZNCC, km.KEEP_ALL
COST_NAMES = {ABSDIFF: "absdiff", ZNCC: "zncc"}
TILE, BAND_TILE = (32, 16), (32, 8)                 # pixels per tile of the windowed kernels resp. of band.hip
RADII = {ABSDIFF: (0, 1, 2, 3, 4), ZNCC: (1, 2, 3, 4)}
FEW_KEEPS = (1, 2, 3, 4, 5, 8, KEEP_ALL)            # both sides of each list length the kernels are built for (2, 4, 8)


class Case:
    def __init__(self, name, W, H, D, cams, main, sides, premise=None, smap=None, dead=(), edges=()):
        self.name, self.W, self.H, self.D = name, W, H, D
        self.cams = [np.asarray(c, np.float64) for c in cams]
        self.V = len(self.cams)
        self.main = np.asarray(main, np.uint8)
        self.sides = list(sides)
        assert self.main.shape == (H, W) and len(self.sides) == self.V and W * H * D <= 200 * 20 * 33
        self.premise, self.edges = premise, edges          # edges: of a band case whose views are ladders, the edge of each
        self.prior = None
        if smap is not None:          # a band case: prior = s / 8 on the integers s, then the dead pixels
            self.smap = np.asarray(smap, np.int64)
            self.prior = (self.smap.astype(np.float64) / 8.0).astype(F)
            for row, col, v in dead:
                self.prior[row, col] = v
            self.prior.setflags(write=False)

    main_cam = property(lambda self: np.eye(4, dtype=F))
    side_cams = property(lambda self: np.stack(self.cams).astype(F))

    def q(self):
        return np.stack([sc.designed_q(c, self.W, self.H) for c in self.cams])

    def z(self):
        return sm.plane_table(self.D, -1.0, 1.0)

    def views(self):
        """the arguments of Context.sweep_set in front of the plane count"""
        return self.main_cam, self.main, self.side_cams, self.sides

    def planes(self):
        """a band case: (z [D, H, W], live [D, H, W]) of band_mirror.planes on prior + the plane table as offsets"""
        return bm.planes(self.prior, self.z())

    def guide(self):
        """a step image, brighter by one gate width on odd rows: the step on column 33 (of 64; where front_x's frame edge falls on plane
        20) resp. 129, so tau 0 keeps a member's own side and row parity, tau 30 its side, tau 255 everything"""
        yy, xx = np.mgrid[0:self.H, 0:self.W]
        return (np.where(xx < (33 if self.W <= 64 else 129), 40, 200) + 16 * (yy & 1)).astype(np.uint8)

    def start_map(self):
        """a start map for the propagation: values of plane_table(16) (odd multiples of 1/16: every difference and every half of one is
        exact, so the seeded slopes are), in blocks of 4 x 2 pixels with steps of 1/8; NaN, 1.0 and 2.0 on the tile seams"""
        yy, xx = np.mgrid[0:self.H, 0:self.W]
        m = (sm.plane_table(16)[(xx // 4 + 2 * (yy // 2)) % 16]).astype(F)
        for row, col, v in _seam_dead(self.W, self.H):
            m[row, col] = v
        return m


def _seam_dead(W, H):
    """(row, col, value) on both sides of the seams of both tilings, and in two corners"""
    out = [(0, 0, 2.0), (H - 1, W - 1, np.nan)]
    for k, row in enumerate(r for r in (7, 8, 15, 16, 23, 24) if r < H):
        out += [(row, 31 + k % 2, np.nan), (row, 32 - k % 2, 2.0), (row, 5 + k, 1.0)]
    for k, col in enumerate((31, 32)):
        out += [(2 + k, col, np.nan), (5, col, (2.0, -1.0)[k])]
    return [(r, c, v) for r, c, v in out if r < H and c < W]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the samples ---------------------------------------------------------------------------------------------------------------------
def _samples(c, z):
    """sample_fixed per view; views with the same camera and frame share one dictionary (max_views: 255 of them)"""
    table, seen, out = sm.weight_table(), {}, []
    for v in range(c.V):
        key = (c.cams[v].tobytes(), np.asarray(c.sides[v]).tobytes())
        if key not in seen:
            seen[key] = sm.sample_fixed(sc.designed_q(c.cams[v], c.W, c.H), z, sm.pad_frame(c.sides[v]), c.W, c.H, table)
        out.append(seen[key])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def samples(name, band=False):
    """-> per view dict(valid, dot, ...) of sweep_mirror.sample_fixed on the plane table, or (band) on the per-pixel map prior + offset
    with the dead planes taken out of `valid`"""
    c = CASES[name]
    if not band:
        return _samples(c, c.z())
    z, live = c.planes()
    out = _samples(c, np.where(live, z, F(np.nan)))
    for s in out:
        assert not (s["valid"] & ~live).any()
    return out


def _view_costs(main, smp, cost, r):
    """rules 2-4 of section 21 resp. rule 1 of section 22 on one view's samples -> (counted [D, H, W] bool, c [D, H, W] uint32)"""
    ok, A = smp["valid"], np.asarray(main).astype(np.int64)
    if cost == ZNCC:
        B = (smp["dot"] + 127) // 255
        parts = [zm.view_cost(A, B[d], ok[d], r) for d in range(len(ok))]
        return tuple(np.stack(a) for a in zip(*parts))
    e = np.where(ok, np.abs(smp["dot"] - 255 * A[None]), 0)
    N = np.stack([zm.box(m.astype(np.int64), r) for m in ok])
    S = np.stack([zm.box(x, r) for x in e])
    assert S.max(initial=0) < 2 ** 23
    return ok, np.where(ok, S // np.maximum(N, 1), 0).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def view_costs(name, cost, r, band=False):
    """(counted, c) per view"""
    done, out = {}, []
    for s in samples(name, band):
        if id(s) not in done:
            done[id(s)] = _frozen(*_view_costs(CASES[name].main, s, cost, r))
        out.append(done[id(s)])
    return tuple(out)


# ---- the volumes ---------------------------------------------------------------------------------------------------------------------
def _shape(c):
    return (c.D, c.H, c.W)


@functools.lru_cache(maxsize=None)
def sweep_volume(name):
    """the plain fixed-sampler sweep (section 2): sum over the views of ok << 24 | |dot - 255 A|"""
    c = CASES[name]
    return _frozen(sm.sweep(c.q(), c.z(), c.main, c.sides)[3])


@functools.lru_cache(maxsize=None)
def zncc_volume(name, r):
    c = CASES[name]
    vol = np.zeros(_shape(c), np.uint32)
    for counted, cost in view_costs(name, ZNCC, r):
        vol += zm.cells(counted, cost)
    return _frozen(vol)


@functools.lru_cache(maxsize=None)
def bestk_volume(name, cost, r, keep, band=False, nviews=None):
    c = CASES[name]
    return _frozen(km.merge(list(view_costs(name, cost, r, band)[:nviews]), keep, _shape(c)))


@functools.lru_cache(maxsize=None)
def gated_volume(name, cost, r, keep, tau):
    c = CASES[name]
    gate = gm.gates(c.guide(), tau, r)
    A, done, per_view = c.main.astype(np.int64), {}, []
    for s in samples(name):
        if id(s) not in done:
            ok = s["valid"]
            x = np.where(ok, (s["dot"] + 127) // 255 if cost == ZNCC else np.abs(s["dot"] - 255 * A[None]), 0)
            done[id(s)] = gm.view_costs(cost, c.main, (ok, x), gate, r)
        per_view.append(done[id(s)])
    return _frozen(km.merge(per_view, keep, _shape(c)))


@functools.lru_cache(maxsize=None)
def band_volume(name):
    """section 19: every pixel of plane d sampled at prior + offset_d, a dead plane's cell 0"""
    c = CASES[name]
    vol = np.zeros(_shape(c), np.int64)
    for s in samples(name, band=True):
        vol += np.where(s["valid"], (1 << 24) + np.abs(s["dot"] - 255 * c.main.astype(np.int64)[None]), 0)
    return _frozen(vol.astype(np.uint32))


def maps(vol, z):
    """section 2's selection on a packed volume -> (depth, cost, index)"""
    return sm.select(vol, z, 24)


def band_gather(name):
    """what the band's volume must be when prior + offset_d IS plane d + s of the table: the plain sweep's cell of that plane, 0 where the
    pixel has no prior or d + s leaves the table"""
    c = CASES[name]
    vol = sweep_volume(name)
    idx = np.arange(c.D)[:, None, None] + c.smap[None]
    rows, cols = np.indices((c.H, c.W))
    have = bm.inside(c.prior)[None] & (idx >= 0) & (idx < c.D)
    return np.where(have, vol[np.clip(idx, 0, c.D - 1), rows[None], cols[None]], 0).astype(np.uint32)


# ---- premises ------------------------------------------------------------------------------------------------------------------------
def bound_planes(c, edge, v=0):
    """a ladder (view v): (the plane on which the border pixel sits on the frame test's bound, the plane next to it inward, the border line)"""
    col, row, axis = sc._border_pixel(c, edge)
    on = samples(c.name)[v]["valid"][:, row, col]
    out = [d for d in range(c.D) if not on[d]]
    kb, nx = (max(out), max(out) + 1) if edge in ("left", "top") else (min(out), min(out) - 1)
    line = np.zeros((c.H, c.W), bool)
    if axis == 0:
        line[:, col] = True
    else:
        line[row, :] = True
    return kb, nx, line


def _ladder_premise(edge, tie):
    def premise(c):
        col, row, axis = sc._border_pixel(c, edge)
        smp = samples(c.name)[0]
        ok = smp["valid"]
        kb, nx, line = bound_planes(c, edge)
        bound = 132 if edge in ("left", "top") else 256 * (c.W if axis == 0 else c.H) + 132
        u = sm.exact_u(c.q()[0], col, row, c.z()[kb], c.W, c.H, axis)
        assert abs(u - bound) == (Fraction(1, 2) if tie else 0), "the real u of the border pixel: ON the bound, resp. half a step off and rounded onto it"
        assert int(smp["ux" if axis == 0 else "uy"][kb, row, col]) == bound
        assert ok[nx].all() and (ok[kb] == ~line).all(), "the two planes differ by the border line"
        for r in (1, 2, 3, 4):
            np.testing.assert_array_equal(zm.box(ok[nx].astype(np.int64), r) - zm.box(ok[kb].astype(np.int64), r), zm.box(line.astype(np.int64), r))
            for cost in (ABSDIFF, ZNCC):
                counted = view_costs(c.name, cost, r)[0][0]
                assert not counted[kb][line].any() and counted[kb][~line].all() and counted[nx].all(), "the border pixels do not count on the bound plane"
        if c.name == "ladder_int_left":
            N = [zm.box(ok[d].astype(np.int64), 2)[3, :5].tolist() for d in (kb, nx)]
            assert N == [[10, 15, 20, 25, 25], [15, 20, 25, 25, 25]], N
    return premise


def _horizon_premise(c):
    ok = samples(c.name)[0]["valid"]
    assert not ok[:, :, :16].any() and ok[:, :, 16:].all()
    for r in (1, 2, 3, 4):
        N, full = zm.box(ok[0].astype(np.int64), r), zm.box(np.ones((c.H, c.W), np.int64), r)
        assert (N[:, 16:16 + r] < full[:, 16:16 + r]).all() and (N[:, 16 + r:] == full[:, 16 + r:]).all(), "N is reduced for columns 16 .. 15 + R"
        assert not zncc_volume(c.name, r)[:, :, :16].any() and not bestk_volume(c.name, ABSDIFF, r, KEEP_ALL)[:, :, :16].any()
        assert (bestk_volume(c.name, ABSDIFF, r, KEEP_ALL)[:, :, 16:] >> 24 == 1).all()


def first_in_frame(c, axis):
    """per plane the first column (row) of view 0 that is in frame, -1 where none is; the same on every row (column)"""
    ok = samples(c.name)[0]["valid"]
    line = ok.any(axis=1 if axis == 0 else 2)
    assert (ok == (line[:, None, :] if axis == 0 else line[:, :, None])).all()
    return np.where(line.any(axis=1), line.argmax(axis=1), -1)


def _front_premise(axis):
    def premise(c):
        first = first_in_frame(c, axis)
        seam = TILE[axis]
        if axis == 0:
            assert first[17:25].tolist() == [56, 48, 41, 33, 25, 17, 10, 2], first
        else:
            assert first[17:25].tolist() == [28, 24, 20, 16, 13, 9, 5, 1], first
        for r in (1, 2, 3, 4):
            assert any(f >= 0 and abs(int(f) - seam) <= r for f in first), "halo members across the seam that are out of the view's frame"
        assert len({int(f) for f in first if f > 0}) >= 7, "the frame's edge crosses the whole frame"
    return premise


def _window_sums(A, B, r):
    A, B = A.astype(np.int64), B.astype(np.int64)
    one = np.ones_like(A)
    return [zm.box(x, r) for x in (one, A, B, A * B, A * A, B * B)]


def _identity_premise(c):
    for s in samples(c.name):
        assert s["valid"].all() and (s["kx"] == 0).all() and (s["ky"] == 0).all()
    for v, frame in enumerate(c.sides):
        assert (samples(c.name)[v]["dot"] == 255 * frame.astype(np.int64)[None]).all(), "the identity camera: dot == 255 texel"


def _extremes_premise(c):
    _identity_premise(c)
    for r in (1, 2, 3, 4):
        (n0, c0), (n1, c1), (n2, _), = view_costs(c.name, ZNCC, r)
        assert n0.all() and (c0 == 0).all(), "the copy: ncc == 1"
        assert n1.all() and (c1 == 65024).all(), "the inverse: ncc == -1"
        assert not n2.any(), "the constant view is counted nowhere"
        assert (zncc_volume(c.name, r) == ((2 << 24) | 65024)).all()


def _stripes_premise(c):
    _identity_premise(c)
    for r in (1, 2, 3, 4):
        N, Sa, Sb, Sab, _, _ = _window_sums(c.main, c.sides[0], r)
        assert (N * Sab - Sa * Sb == 0).all(), "cov == 0 in every cell, frame borders included"
        counted, cost = view_costs(c.name, ZNCC, r)[0]
        assert counted.all() and (cost == 32512).all(), "ncc == 0"


def _flat_premise(c):
    _identity_premise(c)
    for r in (1, 2, 3, 4):
        N, Sa, Sb, Sab, Saa, Sbb = _window_sums(c.main, c.sides[0], r)
        va, vb = N * Saa - Sa * Sa, N * Sbb - Sb * Sb
        assert ((va == 0) & (vb > 0)).any() and ((vb == 0) & (va > 0)).any() and ((va == 0) & (vb == 0)).any(), "windows without variance in either frame, and in both"
        counted = view_costs(c.name, ZNCC, r)[0][0]
        assert (counted == ((va > 0) & (vb > 0))[None]).all(), "a view counts only where both variances are positive"


def _saturated_premise(c):
    _identity_premise(c)
    for r in (1, 2, 3, 4):
        (n0, c0), (n1, c1) = view_costs(c.name, ZNCC, r)
        assert n0.all() and n1.all(), "every cell is counted"
        assert (c0 == 0).all() and (c1 == 65024).all()
    N, Sa, Sb, Sab, Saa, Sbb = _window_sums(c.main, c.sides[0], 4)
    assert Sab.max() >= 81 * 254 ** 2 and Sab.max() < 2 ** 23 and (N * Sab).max() > 4.2e8, "the widest sums of the packed LDS element"


def _max_views_premise(c):
    _identity_premise(c)
    assert c.V == 255
    if c.name == "max_views_zncc":
        for r in (1, 2, 3, 4):
            assert (zncc_volume(c.name, r) == 0xFFFD0200).all() and (bestk_volume(c.name, ZNCC, r, KEEP_ALL) == 0xFFFD0200).all()
            assert (bestk_volume(c.name, ZNCC, r, 8) == ((8 << 24) | 8 * 65024)).all()
    else:
        for r in RADII[ABSDIFF]:
            assert (bestk_volume(c.name, ABSDIFF, r, KEEP_ALL) == ((255 << 24) | 0xFD02FF)).all()
            assert (bestk_volume(c.name, ABSDIFF, r, 8) == ((8 << 24) | 8 * 65025)).all()


def _few_views_premise(c):
    assert (c.cams[3] == c.cams[0]).all() and c.sides[3] is c.sides[0], "view 3 repeats view 0: equal per-view costs in every cell"
    for cost, r in ((ABSDIFF, 0), (ABSDIFF, 2), (ZNCC, 2)):
        assert set(np.unique(bestk_volume(c.name, cost, r, KEEP_ALL) >> 24)) == {0, 1, 2, 3, 4}
        assert set(np.unique(bestk_volume(c.name, cost, r, KEEP_ALL, nviews=3) >> 24)) == {0, 1, 2, 3}
        for keep in FEW_KEEPS[:-1]:
            k = bestk_volume(c.name, cost, r, keep) >> 24
            assert k.max() == min(keep, 4) and (k == np.minimum(keep, bestk_volume(c.name, cost, r, KEEP_ALL) >> 24)).all()


def _band_premise(c):
    z, live = c.planes()
    table = c.z()
    idx = np.arange(c.D)[:, None, None] + c.smap[None]
    have = bm.inside(c.prior)[None] & (idx >= 0) & (idx < c.D)
    assert (live == have).all() and (z[live] == table[idx[live]]).all(), "prior + offset is exactly plane d + s of the table, or dead"
    np.testing.assert_array_equal(band_volume(c.name), band_gather(c.name))
    dead = ~bm.inside(c.prior)
    assert np.isnan(c.prior).sum() >= 3 and (c.prior == 2.0).sum() >= 3 and (np.abs(c.prior) == 1.0).sum() >= 3
    for tw, th in (TILE, BAND_TILE):        # a dead pixel on each side of a seam of each tiling (those the frame has), next to live ones
        assert dead[:, tw - 1].any() and dead[:, tw].any() and not dead[:, tw - 1].all()
        assert th >= c.H or (dead[th - 1].any() and dead[th].any() and not dead[th].all())
    assert (band_volume(c.name) >> 24).max() == c.V
    for v, edge in enumerate(c.edges):      # ladders: some band plane puts a pixel of the border line ON the bound, another the plane next to it
        kb, nx, line = bound_planes(c, edge, v)
        ok = samples(c.name, band=True)[v]["valid"]
        on_bound, inward = live & (idx == kb) & line[None], live & (idx == nx) & line[None]
        assert on_bound.any() and not ok[on_bound].any() and inward.any() and ok[inward].all()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
CASES = {}


def _add(case):
    assert case.name not in CASES
    CASES[case.name] = case
    return case


def _reuse(name, premise=None):
    c = sc.CASES[name]
    main, sides = c.frames()
    return _add(Case(name, c.W, c.H, c.D, c.cams, main, sides, premise))


LADDERS = []
for _edge in ("left", "right", "top", "bottom"):
    for _tie in (False, True):
        LADDERS.append(_reuse("ladder_%s_%s" % ("tie" if _tie else "int", _edge), _ladder_premise(_edge, _tie)).name)
_reuse("horizon", _horizon_premise)
for _name in ("shear_tie", "axial", "checker_extreme", "skip_then_border", "one_plane", "ragged_shear"):
    _reuse(_name)

# cx = col + 1 + 128 z - 64 (skip_then_border's x row at 64 x 32); cy = row + 1 + 64 z - 32
_add(Case("front_x", 64, 32, 33, [sc.cam(x=(1, 0, 4, -2))], sc.noise(64, 32, 101), [sc.noise(64, 32, 102)], _front_premise(0)))
_add(Case("front_y", 64, 32, 33, [sc.cam(y=(0, 1, -4, 2))], sc.noise(64, 32, 103), [sc.noise(64, 32, 104)], _front_premise(1)))

_W, _H = 64, 32
_yy, _xx = np.mgrid[0:_H, 0:_W]
_checker = sc.checkerboard(_W, _H)
_add(Case("ncc_extremes", _W, _H, 16, [sc.cam()] * 3, _checker, [_checker, 255 - _checker, sc.constant(_W, _H, 77)], _extremes_premise))
_add(Case("ncc_stripes", _W, _H, 16, [sc.cam()], ((_yy & 1) * 255).astype(np.uint8), [((_xx & 1) * 255).astype(np.uint8)], _stripes_premise))
_near = np.where((_yy % 3 == 0) & (_xx % 3 == 0), 254, 255).astype(np.uint8)
_add(Case("near_saturated", _W, _H, 16, [sc.cam()] * 2, _near, [_near, 255 - _near], _saturated_premise))

# a constant block in the main frame and one in the side frame, overlapping in columns 24 .. 33: windows with va == 0, with vb == 0, with both
_flat_main, _flat_side = sc.noise(_W, _H, 401), sc.noise(_W, _H, 402)
_flat_main[4:28, 4:34] = 90
_flat_side[4:28, 24:60] = 200
_add(Case("flat_blocks", _W, _H, 16, [sc.cam()], _flat_main, [_flat_side], _flat_premise))

_small = sc.checkerboard(64, 8)
_inverse = 255 - _small
_add(Case("max_views_zncc", 64, 8, 16, [sc.cam()] * 255, _small, [_inverse] * 255, _max_views_premise))
_white = sc.constant(64, 8, 255)
_add(Case("max_views_absdiff", 64, 8, 16, [sc.cam()] * 255, sc.constant(64, 8, 0), [_white] * 255, _max_views_premise))

# the border lines of the three views meet in pixel (0, 0): column 0 enters view 0 on plane 8 and view 1 on plane 9, row 0 enters view 2 on
# plane 9; view 3 is view 0 again
_few = [sc._ladder(64, 8, 16, "left", False), sc._ladder(64, 8, 16, "left", True), sc._ladder(64, 8, 16, "top", True)]
_few_frames = [sc.noise(64, 8, 201 + v) for v in range(3)]
_add(Case("few_views", 64, 8, 16, _few + [_few[0]], sc.noise(64, 8, 200), _few_frames + [_few_frames[0]], _few_views_premise))

# s over -8 .. 8: prior = s / 8, prior + offset_d = (2 (d + s) - 15) / 16; |s| = 8 is a prior of +-1: no prior
_smap = (3 * _xx + 5 * _yy) % 17 - 8
for _k, (_row, _col) in enumerate(((15, 30), (16, 33), (8, 30), (7, 33), (23, 30), (24, 33))):
    _smap[_row, _col] = 8 if _k % 2 else -8
_add(Case("band_shift", _W, _H, 16,
          [sc.cam(x=(1, 0, 4, -2)), sc.CASES["horizon"].cams[0], sc.CASES["shear_tie"].cams[0]],
          sc.noise(_W, _H, 301), [sc.noise(_W, _H, 302 + v) for v in range(3)], _band_premise, smap=_smap, dead=_seam_dead(_W, _H)))

# the ladders under a per-pixel prior: an integer and a tie ladder on each axis, every edge once
_smap8 = (3 * _xx[:8] + 5 * _yy[:8]) % 17 - 8
_edges = (("left", False), ("right", True), ("bottom", False), ("top", True))
_add(Case("band_ladders", 64, 8, 16, [sc._ladder(64, 8, 16, e, t) for e, t in _edges], sc.noise(64, 8, 501), [sc.noise(64, 8, 502 + v) for v in range(4)],
          _band_premise, smap=_smap8, dead=_seam_dead(64, 8), edges=[e for e, _ in _edges]))

NAMES = sorted(CASES)
BANDS = [n for n in NAMES if CASES[n].prior is not None]
PLAIN = [n for n in NAMES if CASES[n].V <= 8 and CASES[n].prior is None]          # every case but max_views and band_shift
PROPAGATED = ("ladder_int_left", "ladder_tie_top", "horizon", "front_x")
