"""The sweep family's context contract, executable: a numpy class that stands for one mvs_ctx (DESIGN.md sections 13, 16, 18-26 and 30,
the comment blocks of include/mvs.h).  It holds what the context holds as plain arrays -- the packed volume with the layout it was
written in, Wv, S, the depth / cost / index maps, the plane table, the band prior / depth / report, the clean report and sizes, the
filtered map -- and the documented flags.  Every library call is a method that either returns the error code the documents promise and
changes nothing, or updates the arrays by calling the mirrors the suite already has.  No arithmetic is restated here: the new code is
the bookkeeping.

Shadow.call(name, *args) -> return code, and appends to Shadow.history.  Device.call() makes the same call on a real context;
compare() fetches everything the shadow says is fetchable and wants equal bits, and the promised code for everything else.

The packed volume grows and never shrinks, a volume that grows loses its contents, and after a change of the plane count the readers
see the old cells under the new count.  The shadow models it as a flat array of a fixed capacity (the largest plane count of the pool),
so every walk makes its largest-D volume first: the shadow raises Unmodelled if a walk would make it grow later.  Wv and S are read
only at the plane count they were written with, and a call writes all of them: they are plain [D, H, W] arrays."""
import functools
import hashlib
import re

import numpy as np

import band_bestk_mirror as bbm
import band_cases
import band_mirror
import bestk_cases
import bestk_mirror as bkm
import clean_mirror
import depth_filter_mirror as dfm
import gated_mirror
import pyramid_mirror
import sgm_mirror as sgm
import window_mirror
import zncc_mirror

OK, EINVAL, ESTATE = 0, -1, -3
VOLUME, FUSED, BOTH = 1, 2, 3
CS = {"fixed": 24, "exact": 16}
ROW_GRAN = {"fixed": 8, "exact": 16}
PLANE_GRAN = 32
ABSDIFF, ZNCC, KEEP_ALL = bkm.COST_ABSDIFF, bkm.COST_ZNCC, bkm.KEEP_ALL
# the plane tables of the pool: (D, z_lo, z_hi).  All lie inside (-1, 1), so each also serves as a band's offsets.  LARGEST comes first
# in every walk.
LARGEST = (19, -0.3, 0.3)                        # band_cases.Crafted's offsets
TABLES = (LARGEST, (7, -0.6, 0.9), (5, 0.25, 0.75), (9, -0.3, 0.3), (7, -0.3, 0.3))    # the last: the same count over another range
AGG = (8, 16, 128, 4080)                         # paths, p1, p2, cost_cap of every aggregation
WIN = (2, 255)                                   # radius, tau of every window


class Unmodelled(Exception):
    """a walk asked for something the shadow does not model (a buffer that would have to grow): a mistake of the walk, not a finding"""


class Inputs:
    """what is staged on one context, and the prior its band runs take"""

    def __init__(self, name, main_cam, main_img, side_cams, sides, prior, coarse_depth=None):
        self.name, self.main_cam, self.main_img, self.side_cams, self.sides = name, main_cam, main_img, np.asarray(side_cams), list(sides)
        self.H, self.W = main_img.shape
        self.V = len(self.sides)
        self.prior, self.coarse_depth = prior, coarse_depth
        for a in (self.prior, self.coarse_depth):
            if a is not None:
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """"crafted": bestk_cases.crafted() (70 x 19, 6 views) with band_cases.crafted()'s prior; "even": 72 x 20 noise frames made as in
    band_cases, three views, a prior with a step and holes, and a 36 x 10 coarse depth map for mvs_pyramid_prior"""
    if name == "crafted":
        c = bestk_cases.crafted()
        return Inputs(name, c.main_cam, c.main_img, c.side_cams, c.sides, band_cases.crafted().prior.copy())
    assert name == "even"
    from mvs_amd import synth
    W, H, V = 72, 20, 3
    rng = np.random.Generator(np.random.PCG64(0x5AD0))
    b = band_cases.crafted()
    main_img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    sides = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(V)]
    cams = np.stack([synth.camera_at([0.12, 0.02, 0.0], W, H, rot=band_cases.rot_y(4.0)), synth.camera_at([0.03, -0.02, -0.35], W, H),
                     synth.camera_at([0.4, 0.1, 0.0], W, H, rot=band_cases.rot_x(-2.0))])
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    prior = (-0.45 + 0.9 * x / W + 0.01 * y).astype(np.float32)
    prior[9:, 30:] += np.float32(0.25)
    prior[2:6, 5:12] = 1.0
    prior[0, 0] = prior[19, 71] = np.nan
    xc, yc = np.meshgrid(np.arange(W // 2), np.arange(H // 2))
    coarse = (0.4 - 0.8 * xc / (W // 2) - 0.02 * yc).astype(np.float32)      # slopes the other way: rule U of it differs from `prior`
    coarse[3:5, 10:14] = 1.0
    coarse[9, 35] = np.nan
    return Inputs(name, synth.camera_at([0, 0, 0], W, H), main_img, cams, sides, prior, coarse)


def _oracle():
    import orc
    return orc.load()


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


_PRIORS = {}


def _prior_key(prior):
    key = hashlib.sha1(np.ascontiguousarray(prior, np.float32).tobytes()).hexdigest()
    _PRIORS.setdefault(key, np.array(prior, np.float32))
    return key


@functools.lru_cache(maxsize=None)
def table(tab):
    return _frozen(_oracle().plane_table(*tab))[0]


def _views(inp, first, count):
    return inp.main_cam, inp.main_img, inp.side_cams[first:first + count], inp.sides[first:first + count]


@functools.lru_cache(maxsize=None)
def mirror_sweep(name, first, count, tab, sampler):
    """mvs_sweep_run -> (depth, cost, index, volume)"""
    return _frozen(*_oracle().sweep(*_views(inputs(name), first, count), tab[0], tab[1], tab[2], want_volume=True, sampler=sampler))


@functools.lru_cache(maxsize=None)
def mirror_volume(kind, name, first, count, tab, args=(), prior=None):
    """the packed volume of the fixed sampler's other sweeps: kind "zncc" (args: radius), "bestk" (cost, radius, keep), "gated" (cost,
    radius, keep, tau; the guide is the main image), "band" (), "band_bestk" (cost, radius, keep)"""
    o, inp = _oracle(), inputs(name)
    v = _views(inp, first, count)
    if kind == "zncc":
        vol = zncc_mirror.volume(o, *v, table(tab), args[0])
    elif kind == "bestk":
        vol = bkm.volume(o, args[0], *v, tab[0], tab[1], tab[2], args[1], args[2])
    elif kind == "gated":
        vol = gated_mirror.volume(o, args[0], *v, tab[0], tab[1], tab[2], args[1], args[2], args[3], None)
    elif kind == "band":
        vol = band_mirror.band_volume(o, *v, _PRIORS[prior], table(tab))
    else:
        assert kind == "band_bestk"
        vol = bbm.volume(o, args[0], *v, _PRIORS[prior], table(tab), args[1], args[2])
    return _frozen(np.ascontiguousarray(vol, np.uint32))[0]


PROPAGATE = (ABSDIFF, 1, 1, 0.05, 0.0)             # cost, radius, iterations, dz, dg of every propagation (all staged views, two random candidates)


@functools.lru_cache(maxsize=None)
def mirror_propagation(name, V, depth):
    """mvs_propagate_init on the map, then mvs_propagate_run -> ((z, gx, gy, cells), report)"""
    import propagate_mirror as pm
    inp = inputs(name)
    cost, r, it, dz, dg = PROPAGATE
    scene = pm.Scene(_oracle(), inp.main_cam, inp.main_img, inp.side_cams[:V], inp.sides[:V])
    st = pm.State(scene, _PRIORS[depth], cost, r).run(it, dz, dg)
    return _frozen(*st.copy_maps()), st.report()


def select(vol, z, sampler, refine=False):
    """mvs_sweep_argmin (and mvs_sweep_refine_depth) on a volume"""
    o = _oracle()
    depth, cost, index = o.argmin(vol, z, sampler=sampler)
    if refine:
        depth = o.refine_depth(vol, z, index, sampler=sampler)
    return depth, cost, index


class Shadow:
    def __init__(self, name, largest=LARGEST):
        """largest: the plane table with the most planes this context will meet (the capacity of the modelled volume)"""
        self.inp = inputs(name)
        self.name, self.W, self.H = name, self.inp.W, self.inp.H
        self.P = self.W * self.H
        self.cap = largest[0] * self.P
        self.history = []
        self.V = 0                                    # staged side views (0: nothing staged)
        self.tab = None                               # the plane table
        self.sampler, self.source = "fixed", "raw"
        self.own, self.own_cap, self.own_cells = None, 0, None        # the context's own volume: flat cells, cells allocated, layout
        self._fresh_own = False                                      # the own volume is allocated and nothing was written to it yet
        self.ext, self.ext_cells, self.external = None, None, False   # the caller's; whether it is in use
        self.Wv, self.win_planes, self.win_cells = None, 0, None
        self.S, self.agg_planes = None, 0
        self.maps = None                              # [depth, cost, index]
        self.sel_planes = self.sel_band_planes = self.sel_band_lo = self.sel_band_hi = 0
        self.band_planes, self.band_resolved = 0, False
        self.band_prior = self.band_depth = self.band_report = None
        self.clean_report = self.clean_sizes = None
        self.filtered = None
        self.prop = None                              # [z, gx, gy, cells] of the propagation, and its report
        self.prop_report = None

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
    @property
    def D(self):
        return self.tab[0] if self.tab else 0

    @property
    def z(self):
        return table(self.tab)

    def call(self, name, *args):
        rc = getattr(self, "do_" + name)(*args)
        self.history.append((name,) + args + (rc,))
        return rc

    def story(self):
        return "\n".join("  %2d. %s(%s) -> %d" % (i, h[0], ", ".join(repr(a) for a in h[1:-1]), h[-1]) for i, h in enumerate(self.history))

    def _cells(self):
        """the current packed volume: (flat cells or None, capacity in cells, layout)"""
        return (self.ext, self.cap, self.ext_cells) if self.external else (self.own, self.own_cap, self.own_cells)

    def _layout_refused(self, cells):
        """the decision of section 30: cells of a known layout are read only under the sampler that wrote them"""
        return cells is not None and cells != self.sampler

    def _volume(self, flat):
        return flat[:self.D * self.P].reshape(self.D, self.H, self.W)

    def _reader_volume(self):
        """mvs::reader_volume -> (rc, volume [D, H, W] or None, None | "short")"""
        if self.source == "windowed":
            if not self.tab or self.win_planes != self.D:
                return ESTATE, None
            if self._layout_refused(self.win_cells):
                return ESTATE, None
            return OK, self.Wv
        flat, cap, cells = self._cells()
        if self._layout_refused(cells):
            return ESTATE, None
        if flat is None or not self.tab:
            return OK, None
        if cap < self.D * self.P:
            return OK, "short"
        return OK, self._volume(flat)

    def _staged(self):
        return self.V > 0 and self.tab is not None

    def _ensure_own(self):
        need = self.D * self.P
        if self.own is None:
            self.own, self.own_cap = np.zeros(self.cap, np.uint32), need
            self._fresh_own = True
        elif need > self.own_cap:
            raise Unmodelled("the context's own volume would grow from %d to %d cells" % (self.own_cap, need))

    def _write_volume(self, vol, rows=None, planes=None):
        if not self.external:
            self._ensure_own()
        flat = self.ext if self.external else self.own
        view = self._volume(flat)
        r0, r1 = rows or (0, self.H)
        d0, d1 = planes or (0, self.D)
        whole = (r0, r1, d0, d1) == (0, self.H, 0, self.D)
        if not self.external and self._fresh_own and not whole:
            raise Unmodelled("a row band or plane group into a volume that holds nothing yet")
        known = self.ext_cells if self.external else self.own_cells
        # a band or plane group under another sampler than the rest was written with leaves cells of both layouts: no reader until a
        # sweep writes the whole volume
        cells = "mixed" if not whole and known is not None and known != self.sampler else self.sampler
        self._fresh_own = False
        view[d0:d1, r0:r1] = vol[d0:d1, r0:r1]
        if self.external:
            self.ext_cells = cells
        else:
            self.own_cells = cells

    def _write_maps(self, maps, rows=None):
        r0, r1 = rows or (0, self.H)
        if self.maps is None:
            if (r0, r1) != (0, self.H):
                raise Unmodelled("a row band into maps that hold nothing yet")
            self.maps = [None, None, None]
        for k in range(3):
            if self.maps[k] is None:
                self.maps[k] = np.array(maps[k])
            else:
                self.maps[k] = self.maps[k].copy()
                self.maps[k][r0:r1] = maps[k][r0:r1]

    def _full_selection(self):
        self.sel_planes, self.sel_band_planes = self.D, 0

    def _no_selection(self):
        self.sel_planes = self.sel_band_planes = 0

    def _rows_selected(self, r0, r1):
        """section 13, "select rows": the whole image, or bands over the plane count the map already has, keep or make a selection; bands
        over another count end it until they -- each touching or overlapping what the earlier ones covered -- reach every row"""
        D = self.D
        if r0 <= 0 and r1 >= self.H:
            return self._full_selection()
        if self.sel_planes == D:
            return
        self.sel_planes = 0
        if self.sel_band_planes != D or r0 > self.sel_band_hi or r1 < self.sel_band_lo:
            self.sel_band_planes, self.sel_band_lo, self.sel_band_hi = D, r0, r1
        else:
            self.sel_band_lo, self.sel_band_hi = min(r0, self.sel_band_lo), max(r1, self.sel_band_hi)
        if self.sel_band_lo <= 0 and self.sel_band_hi >= self.H:
            self._full_selection()

    def _selection_current(self):
        return self.maps is not None and self.sel_planes != 0 and self.sel_planes == self.D

    # ---- staging -------------------------------------------------------------------------------------------------------------------
    def do_stage(self, tab):
        """mvs_sweep_set_main, mvs_sweep_set_views with every view, mvs_sweep_set_planes"""
        self.V, self.tab = self.inp.V, tab
        return OK

    def do_set_planes(self, tab):
        self.tab = tab       # ends nothing by itself: the readers compare the counts when they are called
        return OK

    def do_set_views(self, count):
        """mvs_sweep_set_views with the first `count` views: the results stay as they are"""
        self.V = count
        return OK

    def do_set_sampler(self, sampler):
        self.sampler = sampler
        return OK

    def do_set_source(self, source):
        self.source = source
        return OK

    def do_use_volume(self, external):
        """mvs_sweep_use_volume with the caller's buffer (of the largest table's size, holding empty cells) or NULL: back to the own one"""
        if external:
            self.ext, self.ext_cells = np.zeros(self.cap, np.uint32), None      # the device side hands in a zeroed buffer every time
        self.external = bool(external)
        return OK

    # ---- the sweeps ----------------------------------------------------------------------------------------------------------------
    def _views_ok(self, first, count):
        return first >= 0 and count >= 0 and first + count <= self.V

    def do_sweep_run(self, first, count, flags, rows=None):
        if not self._staged():
            return ESTATE
        if rows is not None:
            r0, n = rows
            g = ROW_GRAN[self.sampler]
            if r0 < 0 or n < 0 or r0 + n > self.H or r0 % g or ((r0 + n) % g and r0 + n != self.H):
                return EINVAL
            rows = (r0, r0 + n)
        if not self._views_ok(first, count) or not flags & BOTH:
            return EINVAL
        depth, cost, index, vol = mirror_sweep(self.name, first, count, self.tab, self.sampler)
        self.band_planes = 0
        if flags & VOLUME:
            self._write_volume(vol, rows)
        if flags & FUSED:
            self._write_maps((depth, cost, index), rows)
            self._rows_selected(*(rows or (0, self.H)))
        return OK

    def do_sweep_run_rows(self, r0, n, first, count, flags):
        return self.do_sweep_run(first, count, flags, (r0, n))

    def do_sweep_run_planes(self, first, count, plane_first, plane_count, flags):
        """mvs_sweep_run_planes: a plane group of the volume (groups begin and end on multiples of 32 planes or at D); no selection"""
        if flags & FUSED:
            return EINVAL
        d0, d1 = plane_first, plane_first + plane_count
        if d0 < 0 or plane_count < 0 or d1 > self.D or d0 % PLANE_GRAN or (d1 % PLANE_GRAN and d1 != self.D):
            return EINVAL
        if not self._staged():
            return ESTATE
        if not self._views_ok(first, count) or not flags & VOLUME:
            return EINVAL
        if plane_count == 0:
            return OK
        self.band_planes = 0
        self._write_volume(mirror_sweep(self.name, first, count, self.tab, self.sampler)[3], None, (d0, d1))
        return OK

    def _fx_sweep(self, kind, first, count, flags, args=(), prior=None, band=False):
        """the fixed sampler's other sweeps share their checks and what they leave"""
        if band and prior is None:
            return EINVAL
        if not flags & BOTH:
            return EINVAL
        if not self._staged() or self.sampler != "fixed":
            return ESTATE
        if not self._views_ok(first, count):
            return EINVAL
        z = self.z
        if band and not ((z > -1.0) & (z < 1.0)).all():
            return ESTATE
        key = _prior_key(prior) if band else None
        vol = mirror_volume(kind, self.name, first, count, self.tab, tuple(args), key)
        if band:
            self.band_prior = np.array(prior, np.float32)
        if flags & VOLUME:
            self._write_volume(vol)
        if flags & FUSED:
            self._write_maps(select(vol, z, "fixed"))
            self._full_selection()
        else:
            if self.maps is None:
                raise Unmodelled("maps that are allocated and hold nothing")
            self._no_selection()
        self.band_planes, self.band_resolved = (self.D, False) if band else (0, self.band_resolved)
        return OK

    def do_sweep_run_zncc(self, radius, first, count, flags):
        return self._fx_sweep("zncc", first, count, flags, (radius,))

    def do_sweep_run_bestk(self, cost, radius, keep, first, count, flags):
        return self._fx_sweep("bestk", first, count, flags, (cost, radius, keep))

    def do_sweep_run_bestk_gated(self, cost, radius, keep, tau, first, count, flags):
        return self._fx_sweep("gated", first, count, flags, (cost, radius, keep, tau))

    def prior_of(self, which):
        """the priors a band run can take: "crafted" (the pool's), "depth" (the context's depth map), "own" (the context's prior buffer)"""
        return {None: None, "crafted": self.inp.prior, "depth": None if self.maps is None else self.maps[0], "own": self.band_prior}[which]

    def do_sweep_run_band(self, which, first, count, flags):
        return self._fx_sweep("band", first, count, flags, (), self.prior_of(which), band=True)

    def do_sweep_run_band_bestk(self, which, cost, radius, keep, first, count, flags):
        return self._fx_sweep("band_bestk", first, count, flags, (cost, radius, keep), self.prior_of(which), band=True)

    # ---- selection, aggregation, window, cleaning --------------------------------------------------------------------------------
    def do_sweep_argmin(self):
        rc, vol = self._reader_volume()
        if rc:
            return rc
        if vol is None:
            return ESTATE
        if isinstance(vol, str):
            if self.external:
                return EINVAL
            raise Unmodelled("mvs_sweep_argmin would make the own volume grow")
        self._write_maps(select(vol, self.z, self.sampler))
        self._full_selection()
        return OK

    def do_combine_partials(self):
        """mvs_sweep_argmin_partial on the planes [0, 8) and [8, D) of the current packed volume, through the caller's pointers (no
        volume source, no layout check: the cells are decoded as the current sampler's), then mvs_sweep_combine_partials"""
        flat, cap, _ = self._cells()
        if not self.tab or flat is None:
            raise Unmodelled("partials of a volume that is not there")
        if cap < self.D * self.P:
            raise Unmodelled("mvs_sweep_volume_device would make the volume grow")
        self._write_maps(select(self._volume(flat), self.z, self.sampler))
        self._full_selection()
        return OK

    def do_sweep_refine_depth(self):
        rc, vol = self._reader_volume()
        if rc:
            return rc
        if vol is None or self.maps is None or not self.sel_planes or not self._selection_current():
            return ESTATE
        if isinstance(vol, str):
            return EINVAL if self.external else ESTATE
        self._write_maps((_oracle().refine_depth(vol, self.z, self.maps[2], sampler=self.sampler), self.maps[1], self.maps[2]))
        return OK

    def do_sweep_aggregate(self, refine):
        paths, p1, p2, cap = AGG
        rc, vol = self._reader_volume()
        if rc:
            return rc
        if vol is None:
            return ESTATE
        if isinstance(vol, str):
            return EINVAL
        cs = CS[self.sampler]
        S = sgm.aggregate(sgm.cost16(vol, cs, cap), paths, p1, p2)
        seen = sgm.seen_cells(vol, cs)
        depth, cost, index = sgm.select(S, seen, self.z, paths)
        if refine:
            depth = sgm.refine(S, seen, self.z, index)
        self.S, self.agg_planes = S, self.D
        self._write_maps((depth, cost, index))
        self._full_selection()
        return OK

    def do_sweep_window(self, select_maps, refine):
        """mvs_sweep_window reads the RAW volume whatever the volume source is"""
        if refine and not select_maps:
            return EINVAL
        if not self.tab:
            return ESTATE
        flat, cap, cells = self._cells()
        if flat is None or cap < self.D * self.P:
            return ESTATE
        if self._layout_refused(cells):
            return ESTATE
        Wv = window_mirror.window(self._volume(flat), CS[self.sampler], WIN[0], WIN[1]).astype(np.uint32)
        self.Wv, self.win_planes, self.win_cells = Wv, self.D, self.sampler
        if select_maps:
            self._write_maps(select(Wv, self.z, self.sampler, refine))
            self._full_selection()
        return OK

    def do_sweep_clean(self, min_views, uniqueness, speckle_min_size, speckle_max_diff, aggregated):
        if self.maps is None or not self.sel_planes or not self._selection_current():
            return ESTATE
        rc, vol = self._reader_volume()
        if rc:
            return rc
        have = vol is not None and not isinstance(vol, str)
        rule1, rule2 = min_views >= 2 or (min_views == 1 and have), uniqueness > 0
        if (rule1 or rule2) and not have:
            return ESTATE
        if aggregated and self.agg_planes != self.D:
            return ESTATE
        S = self.S if aggregated else None
        depth, cost, index, report, sizes = clean_mirror.clean(*self.maps, vol=vol if rule1 or rule2 else None, cs=CS[self.sampler], S=S if rule2 else None,
                                                               min_views=min_views if rule1 else 0, uniqueness=uniqueness, speckle_min_size=speckle_min_size,
                                                               speckle_max_diff=speckle_max_diff)
        self._write_maps((depth, cost, index))
        self.clean_report, self.clean_sizes = report, sizes
        return OK

    # ---- band state ----------------------------------------------------------------------------------------------------------------
    def band_state(self):
        return OK if self.band_planes and self.tab and self.D == self.band_planes and self._selection_current() else ESTATE

    def do_band_resolve(self):
        if self.band_state():
            return ESTATE
        self.band_depth = band_mirror.resolve(self.band_prior, self.maps[0], self.maps[2])
        self.band_report = band_mirror.report(self.band_prior, self.maps[0], self.maps[2], self.D)
        self.band_resolved = True
        return OK

    def band_fetchable(self):
        return OK if not self.band_state() and self.band_resolved else ESTATE

    def do_pyramid_prior(self):
        """mvs_pyramid_prior(this context as the fine level, the pool's coarse depth map, tau 255): a new prior ends the band run"""
        self.band_prior = pyramid_mirror.prior(self.inp.coarse_depth)
        self.band_planes = 0
        return OK

    # ---- neighbours of the family ---------------------------------------------------------------------------------------------------
    def do_depth_filter(self, radius, tau):
        """mvs_depth_filter on the context's own depth map, the staged main image as the guide: writes the filtered map only"""
        if self.maps is None:
            return EINVAL        # a NULL depth pointer
        self.filtered = dfm.filter(self.maps[0], radius, tau, dfm.INF, self.inp.main_img)
        return OK

    def do_propagate(self, which):
        """mvs_propagate_init on the context's depth map ("depth") or on its prior buffer ("own"), then one mvs_propagate_run: its own
        maps, nothing of the sweep family"""
        if self.prior_of(which) is None:
            return EINVAL
        if not self.V or self.sampler != "fixed":
            return ESTATE
        self.prop, self.prop_report = mirror_propagation(self.name, self.V, _prior_key(self.prior_of(which)))
        return OK

    def do_bystander(self, which):
        """calls of other stages, all accepted: "downsample" (mvs_pyramid_downsample_device on a caller's frames), "undistort" (mvs_set_lens
        and mvs_undistort of a caller's frame)"""
        return OK

    def do_fetch(self, what):
        """a reader that only fetches: compare() checks it after every step, this entry names it in the history"""
        return self.fetch_code(what)

    # ---- what compare() expects -------------------------------------------------------------------------------------------------
    def fetch_code(self, what):
        if what == "maps":
            return OK if self.maps is not None else ESTATE
        if what == "volume":
            flat, cap, cells = self._cells()
            return ESTATE if flat is None or self._layout_refused(cells) else OK
        if what == "window":
            return OK if self.win_planes else ESTATE
        if what == "aggregate":
            return OK if self.agg_planes else ESTATE
        if what == "clean_report":
            return OK if self.clean_report is not None else ESTATE
        if what == "clean_sizes":
            return OK if self.clean_sizes is not None else ESTATE
        if what in ("band_fetch", "band_report"):
            return self.band_fetchable()
        if what in ("propagation", "propagation_report"):
            return OK if self.prop is not None else ESTATE
        assert what == "filtered"
        return OK if self.filtered is not None else ESTATE

    def volume_fetch_is_safe(self):
        """mvs_sweep_fetch copies D planes without looking at the buffer's size: the walk must not ask beyond it"""
        flat, cap, _ = self._cells()
        return flat is None or cap >= self.D * self.P

    def fetched(self, what):
        if what == "maps":
            return tuple(self.maps)
        if what == "volume":
            return self._volume(self._cells()[0])
        return {"window": self.Wv, "aggregate": self.S, "clean_report": self.clean_report, "clean_sizes": self.clean_sizes, "band_fetch": self.band_depth, "band_report": self.band_report,
                "filtered": self.filtered, "propagation": self.prop, "propagation_report": self.prop_report}[what]

    def snapshot(self):
        """every array and flag, for the determinism check"""
        out = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in vars(self).items() if k not in ("inp", "history", "maps", "prop")}
        out["prop"] = None if self.prop is None else tuple(m.tobytes() for m in self.prop)
        out["maps"] = None if self.maps is None else tuple(m.tobytes() for m in self.maps)
        return out


FETCHES = ("maps", "volume", "window", "aggregate", "clean_report", "clean_sizes", "band_fetch", "band_report", "filtered", "propagation", "propagation_report")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- the same calls on a real context ------------------------------------------------------------------------------------------------
class Device:
    """makes Shadow's calls on an mvs_amd.Context (and a half-size one for mvs_pyramid_prior) and returns the library's codes"""

    def __init__(self, name, largest=LARGEST):
        import mvs_amd
        import torch
        self.mvs, self.torch = mvs_amd, torch
        self.inp, self.largest = inputs(name), largest
        self.ctx = mvs_amd.Context(self.inp.W, self.inp.H, 0)
        self.coarse = None
        self.prior = self._device(self.inp.prior)
        self.keep = []                        # caller's buffers stay alive as long as the context may read them

    def close(self):
        self.torch.cuda.synchronize()
        self.ctx.close()
        if self.coarse:
            self.coarse.close()

    def _device(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.torch.cuda.synchronize()
        return t

    def _rc(self, fn, *args, **kw):
        try:
            fn(*args, **kw)
        except self.mvs.MvsError as e:
            m = re.match(r"libmvs_hip error (-?\d+)", str(e))
            if not m:
                raise
            return int(m.group(1))
        return OK

    def _prior_ptr(self, which):
        c = self.ctx
        return {None: 0, "crafted": self.prior.data_ptr(), "depth": c.sweep_result_pointers()[0] or 0, "own": c.sweep_band_pointers()[1]}[which]

    def call(self, name, *args):
        return getattr(self, "do_" + name)(*args)

    def do_stage(self, tab):
        i = self.inp
        return self._rc(self.ctx.sweep_set, i.main_cam, i.main_img, i.side_cams, i.sides, *tab)

    def do_set_planes(self, tab):
        return self._rc(self.ctx.sweep_set_planes, *tab)

    def do_set_views(self, count):
        return self._rc(self.ctx.sweep_set_views, self.inp.side_cams[:count], self.inp.sides[:count])

    def do_set_sampler(self, sampler):
        return self._rc(self.ctx.set_sampler, sampler)

    def do_set_source(self, source):
        return self._rc(self.ctx.set_volume_source, source)

    def do_use_volume(self, external):
        if not external:
            return self._rc(self.ctx.sweep_use_volume, None, 0)
        buf = self.torch.zeros(self.largest[0] * self.inp.W * self.inp.H, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        self.keep.append(buf)
        return self._rc(self.ctx.sweep_use_volume, buf.data_ptr(), buf.numel() * 4)

    def do_sweep_run(self, first, count, flags):
        return self._rc(self.ctx.sweep_run, first, count, flags)

    def do_sweep_run_rows(self, r0, n, first, count, flags):
        return self._rc(self.ctx.sweep_run_rows, r0, n, first, count, flags)

    def do_sweep_run_planes(self, first, count, plane_first, plane_count, flags):
        return self._rc(self.ctx.sweep_run_planes, first, count, plane_first, plane_count, flags)

    def do_sweep_run_zncc(self, radius, first, count, flags):
        return self._rc(self.ctx.sweep_run_zncc, radius, first, count, flags)

    def do_sweep_run_bestk(self, cost, radius, keep, first, count, flags):
        return self._rc(self.ctx.sweep_run_bestk, cost, radius, keep, first, count, flags)

    def do_sweep_run_bestk_gated(self, cost, radius, keep, tau, first, count, flags):
        return self._rc(self.ctx.sweep_run_bestk_gated, cost, radius, keep, tau, None, first, count, flags)

    def do_sweep_run_band(self, which, first, count, flags):
        return self._rc(self.ctx.sweep_run_band, self._prior_ptr(which), first, count, flags)

    def do_sweep_run_band_bestk(self, which, cost, radius, keep, first, count, flags):
        return self._rc(self.ctx.sweep_run_band_bestk, self._prior_ptr(which), cost, radius, keep, first, count, flags)

    def do_sweep_argmin(self):
        return self._rc(self.ctx.sweep_argmin)

    def do_combine_partials(self):
        c, P = self.ctx, self.inp.W * self.inp.H
        vol, _ = c.sweep_volume_device()
        groups = [(0, 8), (8, c.D - 8)] if c.D > 8 else [(0, c.D // 2), (c.D // 2, c.D - c.D // 2)]
        parts = self.torch.zeros(len(groups) * P * 2, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        for k, (first, count) in enumerate(groups):
            rc = self._rc(c.sweep_argmin_partial, vol + 4 * first * P, first, count, parts.data_ptr() + 8 * k * P)
            if rc:
                return rc
        rc = self._rc(c.sweep_combine_partials, parts.data_ptr(), len(groups))
        c.synchronize()
        return rc

    def do_sweep_refine_depth(self):
        return self._rc(self.ctx.sweep_refine_depth)

    def do_sweep_aggregate(self, refine):
        return self._rc(self.ctx.sweep_aggregate, *AGG, refine=refine)

    def do_sweep_window(self, select_maps, refine):
        return self._rc(self.ctx.sweep_window, WIN[0], WIN[1], None, select_maps, refine)

    def do_sweep_clean(self, min_views, uniqueness, speckle_min_size, speckle_max_diff, aggregated):
        return self._rc(self.ctx.sweep_clean, min_views, uniqueness, speckle_min_size, speckle_max_diff, aggregated)

    def do_band_resolve(self):
        return self._rc(self.ctx.sweep_band_resolve, fetch=False)

    def do_pyramid_prior(self):
        if self.coarse is None:
            self.coarse = self.mvs.Context(self.inp.W // 2, self.inp.H // 2, 0)
            self.coarse_depth = self._device(self.inp.coarse_depth)
        return self._rc(self.ctx.pyramid_prior, self.coarse, self.coarse_depth.data_ptr(), 255)

    def do_depth_filter(self, radius, tau):
        ptr = self.ctx.sweep_result_pointers()[0]
        if not ptr:
            return self.ctx.lib.mvs_depth_filter(self.ctx.h, None, None, radius, tau, float("inf"), 0, 3)
        return self._rc(self.ctx.depth_filter, ptr, radius, tau, fetch=False)

    def do_propagate(self, which):
        ptr = self._prior_ptr(which)
        if not ptr:
            return self.ctx.lib.mvs_propagate_init(self.ctx.h, None, 0, 1, ZNCC, 2, KEEP_ALL, float("inf"), 0)
        cost, r, it, dz, dg = PROPAGATE
        rc = self._rc(self.ctx.propagate_init, ptr, cost, r)
        return rc or self._rc(self.ctx.propagate_run, it, dz, dg)

    def do_bystander(self, which):
        H, W = self.inp.H, self.inp.W
        if which == "undistort":
            rc = self._rc(self.ctx.set_lens, [0.05, 0.01])
            return rc or self._rc(self.ctx.undistort, self.inp.main_img)
        assert which == "downsample" and not (H | W) & 1
        src, dst = self._device(self.inp.main_img), self.torch.zeros(H * W // 4, dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        rc = self._rc(self.ctx.pyramid_downsample_device, src.data_ptr(), dst.data_ptr(), 1)
        self.torch.cuda.synchronize()
        return rc

    def pointers(self):
        """every device address the library hands out for the family's buffers (0: not there)"""
        c, lib, h = self.ctx, self.ctx.lib, self.ctx.h
        import ctypes as C
        n = C.c_size_t(0)
        return (tuple(p or 0 for p in c.sweep_result_pointers()) + tuple(c.sweep_band_pointers()) +
                (lib.mvs_sweep_windowed_device(h, C.byref(n)) or 0, lib.mvs_sweep_aggregated_device(h, C.byref(n)) or 0, c.depth_filtered_pointer(),
                 c.propagate_depth_pointer(), c.propagate_cost_pointer()))

    def do_fetch(self, what):
        return self.fetch(what)[0]

    def fetch(self, what):
        """-> (code, what came back or None)"""
        import ctypes as C
        c, out = self.ctx, []
        H, W = self.inp.H, self.inp.W

        def run(fn, *a, **kw):
            try:
                out.append(fn(*a, **kw))
            except self.mvs.MvsError as e:
                return int(re.match(r"libmvs_hip error (-?\d+)", str(e)).group(1))
            return OK

        def sized(device_fn, fetch_fn, dtype, ctype):
            """Wv and S: the size the library reports, then the C entry itself (one element of room where it reports nothing)"""
            n = C.c_size_t(0)
            device_fn(c.h, C.byref(n))
            planes = n.value // (np.dtype(dtype).itemsize * H * W)
            buf = np.empty((planes, H, W) if planes else (1,), dtype)
            rc = fetch_fn(c.h, buf.ctypes.data_as(C.POINTER(ctype)))
            out.append(buf)
            return rc

        if what == "maps":
            rc = run(lambda: c.sweep_fetch()[:3])
        elif what == "volume":
            rc = run(lambda: c.sweep_fetch(want_volume=True)[3])
        elif what == "window":
            rc = sized(c.lib.mvs_sweep_windowed_device, c.lib.mvs_sweep_window_fetch, np.uint32, C.c_uint32)
        elif what == "aggregate":
            rc = sized(c.lib.mvs_sweep_aggregated_device, c.lib.mvs_sweep_aggregate_fetch, np.uint16, C.c_uint16)
        elif what == "propagation":
            rc = run(c.propagate_fetch)
        elif what == "propagation_report":
            rc = run(c.propagate_report)
        elif what == "clean_report":
            rc = run(c.sweep_clean_report)
        elif what == "clean_sizes":
            rc = run(c.sweep_clean_sizes)
        elif what == "band_report":
            rc = run(c.sweep_band_report)
        elif what == "band_fetch":
            depth = np.empty((H, W), np.float32)
            rc = c.lib.mvs_sweep_band_fetch(c.h, depth.ctypes.data_as(C.POINTER(C.c_float)))
            out.append(depth)
        else:
            assert what == "filtered"
            depth = np.empty((H, W), np.float32)
            rc = c.lib.mvs_depth_filter_fetch(c.h, depth.ctypes.data_as(C.POINTER(C.c_float)))
            out.append(depth)
        return rc, (out[0] if rc == OK else None)


def compare(shadow, device, where=""):
    """everything the shadow says is fetchable, bit for bit; the promised code for everything else"""
    for what in FETCHES:
        want = shadow.fetch_code(what)
        if what == "volume" and not shadow.volume_fetch_is_safe():
            continue
        rc, got = device.fetch(what)
        assert rc == want, "%s%s: the fetch returned %d, the contract says %d, after\n%s" % (where, what, rc, want, shadow.story())
        if rc != OK:
            continue
        ref = shadow.fetched(what)
        names = {"maps": ("depth", "cost", "index"), "propagation": ("z", "gx", "gy", "cells of the propagation")}
        pairs = zip(got, ref, names[what]) if what in names else [(got, ref, what)]
        for g, r, name in pairs:
            if isinstance(r, list):
                assert list(g) == r, "%s%s: %s, the contract says %s, after\n%s" % (where, name, list(g), r, shadow.story())
                continue
            g, r = bits(np.asarray(g)), bits(np.asarray(r))
            assert g.shape == r.shape, "%s%s: shape %s, the contract says %s, after\n%s" % (where, name, g.shape, r.shape, shadow.story())
            bad = np.argwhere(g != r)
            assert len(bad) == 0, "%s%s: %d of %d elements differ, first at %s: %s, the contract says %s, after\n%s" % (
                where, name, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], np.asarray(r)[tuple(bad[0])], shadow.story())


def step(shadow, device, name, *args):
    """one call on both sides: the codes agree, then everything fetchable agrees"""
    want = shadow.call(name, *args)
    rc = device.call(name, *args)
    assert rc == want, "%s%s returned %d, the contract says %d, after\n%s" % (name, args, rc, want, shadow.story())
    compare(shadow, device)
    return rc


# ---- the cases: one prologue, the writers, the readers, the bystanders, the walks -------------------------------------------------------
def prologue(name):
    """what every case begins with: the largest table, a sweep with both outputs, a window with selection, an aggregation -- the
    volume, Wv, S and the maps are then as large as any later call can address -- and a propagation, whose state every later call of
    the family must leave alone"""
    V = inputs(name).V
    return [("stage", LARGEST), ("sweep_run", 0, V, BOTH), ("sweep_window", True, False), ("sweep_aggregate", False), ("propagate", "depth")]


def _outputs(stem, make):
    return {"%s_%s" % (stem, n): [make(f)] for n, f in (("volume", VOLUME), ("fused", FUSED), ("both", BOTH))}


def writers(name):
    """name -> the calls of one writer of the matrix (mostly one)"""
    V = inputs(name).V
    w = {}
    w.update(_outputs("run", lambda f: ("sweep_run", 0, V, f)))
    w["rows_part"] = [("sweep_run_rows", 0, 16, 0, V, BOTH)]
    w["rows_all"] = [("sweep_run_rows", 16, inputs(name).H - 16, 0, V, BOTH), ("sweep_run_rows", 0, 16, 0, V, BOTH)]
    w["rows_other_count"] = [("set_planes", TABLES[1]), ("sweep_run_rows", 0, 16, 0, V, BOTH)]
    w.update(_outputs("zncc", lambda f: ("sweep_run_zncc", 2, 0, V, f)))
    w.update(_outputs("bestk", lambda f: ("sweep_run_bestk", ABSDIFF, 1, 2, 0, V, f)))
    w.update(_outputs("gated", lambda f: ("sweep_run_bestk_gated", ZNCC, 1, 2, 20, 0, V, f)))
    w.update(_outputs("band", lambda f: ("sweep_run_band", "crafted", 0, 3, f)))
    w.update(_outputs("band_bestk", lambda f: ("sweep_run_band_bestk", "crafted", ZNCC, 1, KEEP_ALL, 0, 3, f)))
    w["argmin"] = [("sweep_argmin",)]
    w["combine_partials"] = [("combine_partials",)]
    w["aggregate"] = [("sweep_aggregate", False)]
    w["aggregate_refine"] = [("sweep_aggregate", True)]
    w["window"] = [("sweep_window", False, False)]
    w["window_select"] = [("sweep_window", True, False)]
    w["window_refine"] = [("sweep_window", True, True)]
    w["clean"] = [("sweep_clean", 2, 10, 4, 1, False)]
    w["planes_new_count"] = [("set_planes", TABLES[1])]
    w["planes_same_count"] = [("set_planes", (LARGEST[0], -0.25, 0.35))]
    w["views_fewer"] = [("set_views", 3 if V > 3 else 2)]
    w["set_sampler"] = [("set_sampler", "exact")]
    w["set_sampler_and_back"] = [("set_sampler", "exact"), ("set_sampler", "fixed")]
    # a row band under another sampler than the rest of the volume: cells of both layouts until a sweep writes all of it
    w["rows_other_sampler"] = [("set_sampler", "exact"), ("sweep_run_rows", 0, 16, 0, V, VOLUME)]
    w["rows_other_sampler_then_all"] = [("set_sampler", "exact"), ("sweep_run_rows", 0, 16, 0, V, VOLUME), ("sweep_run", 0, V, VOLUME)]
    w["set_source"] = [("set_source", "windowed")]
    w["use_volume"] = [("use_volume", True)]
    w["use_volume_and_back"] = [("use_volume", True), ("sweep_run", 0, 2, VOLUME), ("use_volume", False)]
    if inputs(name).coarse_depth is not None:
        w["pyramid_prior"] = [("pyramid_prior",)]
    return w


READERS = {
    "refine": ("sweep_refine_depth",),
    "clean_views": ("sweep_clean", 2, 0, 0, 1, False),
    "clean_unique": ("sweep_clean", 0, 10, 0, 1, False),
    "clean_speckle": ("sweep_clean", 0, 0, 4, 1, False),
    "clean_aggregated": ("sweep_clean", 0, 10, 0, 1, True),
    "band_resolve": ("band_resolve",),
    "band_report": ("fetch", "band_report"),
    "band_fetch": ("fetch", "band_fetch"),
    "argmin": ("sweep_argmin",),
    "aggregate": ("sweep_aggregate", True),
    "window": ("sweep_window", True, True),
    "window_fetch": ("fetch", "window"),
    "aggregate_fetch": ("fetch", "aggregate"),
    "clean_report": ("fetch", "clean_report"),
    "clean_sizes": ("fetch", "clean_sizes"),
    "fetch_volume": ("fetch", "volume"),
    "depth_filter": ("depth_filter", 2, 30),
    "propagate_depth": ("propagate", "depth"),
    "propagate_prior": ("propagate", "own"),
}
# the band readers look at a band run: the matrix puts one before the writer, so that what the writer does to it shows
BAND_READERS = ("band_resolve", "band_report", "band_fetch")
BAND_RUN = [("sweep_run_band", "crafted", 0, 3, BOTH), ("band_resolve",)]
# what the matrix asks behind every reader: the two calls whose answer shows the selection state and the band state, which no fetch
# shows (a writer that forgets to make a selection or to start a band run is invisible while the baseline's still stands)
PROBES = [("band_resolve",), ("sweep_refine_depth",)]
BYSTANDERS = {
    "depth_filter": ("depth_filter", 2, 30),
    "propagate": ("propagate", "depth"),
    "downsample": ("bystander", "downsample"),
    "undistort": ("bystander", "undistort"),
    "refused_band_run": ("sweep_run_band", None, 0, 3, BOTH),
    "refused_view_range": ("sweep_run", 0, 99, BOTH),
    "refused_rows": ("sweep_run_rows", 3, 5, 0, 2, BOTH),
}


def matrix(name):
    """(id, calls before the reader, the reader's call) of every writer x reader"""
    out = []
    for wn, wcalls in writers(name).items():
        for rn, rcall in READERS.items():
            before = prologue(name) + (BAND_RUN if rn in BAND_READERS else []) + wcalls
            out.append(("%s-%s" % (wn, rn), before, rcall))
    return out


def walk_prologue(name):
    """a walk makes its largest-D volume first and then changes the plane count: everything behind it happens after such a change"""
    return [("stage", LARGEST), ("sweep_run", 0, inputs(name).V, BOTH), ("set_planes", TABLES[1])]


FIXED_ONLY = ("sweep_run_zncc", "sweep_run_bestk", "sweep_run_bestk_gated", "sweep_run_band", "sweep_run_band_bestk")
# readers that the contract never refuses once a sweep has run
NEVER_REFUSED = ("depth_filter",)


def reader_events(shadow, call, rc):
    """the (reader, accepted) pairs one step shows: the call itself if it is a reader's, and the fetches compare() makes behind it"""
    ev = {(n, rc == OK) for n, c in READERS.items() if c == call and c[0] != "fetch"}
    if call[0] in FIXED_ONLY:       # the windowed and the band sweeps, which the exact sampler refuses: part of every walk
        ev.add(("fixed_only_sweep", rc == OK))
    return ev | {(n, shadow.fetch_code(c[1]) == OK) for n, c in READERS.items() if c[0] == "fetch"}


def wanted_events():
    return {(n, a) for n in list(READERS) + ["fixed_only_sweep"] for a in (True, False) if a or n not in NEVER_REFUSED}


def walk_pool(name):
    V = inputs(name).V
    pool = []
    for wn, calls in writers(name).items():
        if not wn.startswith("rows_other_sampler"):      # (the walks meet the mixture through their own row bands and sampler switches)
            pool += [c for c in calls if c[0] != "set_views"]
    pool += list(READERS.values())
    pool += [("set_planes", t) for t in TABLES] * 2 + [("set_sampler", "fixed"), ("set_sampler", "exact")] * 3
    pool += [("set_source", "raw"), ("set_source", "windowed"), ("use_volume", False), ("use_volume", True)]
    pool += [("sweep_run", 0, V, BOTH)] * 4 + [("sweep_run", 0, 3, BOTH)] * 2 + [("sweep_run_band", "depth", 0, 3, BOTH), ("sweep_run_band", "own", 0, 3, FUSED)]
    pool += [("band_resolve",)] * 3
    return pool


WALK_SEEDS = (7, 17, 40)      # chosen on the CPU: each reaches every reader accepted and refused (tests/test_shadow_cpu.py)
WALK_STEPS = 40
# what every walk does at fixed steps, whatever the seed: the plane tables 7 -> 5 -> 9 -> 7 over another range, a caller's volume and
# back, both volume sources, a row band
ITINERARY = {4: ("use_volume", True), 9: ("set_planes", TABLES[2]), 13: ("set_source", "windowed"), 16: ("combine_partials",), 18: ("use_volume", False), 22: ("set_planes", TABLES[3]),
             27: ("set_source", "raw"), 31: ("set_planes", TABLES[4]), 39: ("sweep_run_rows", 0, 16, 0, 3, FUSED)}


def walk_calls(name, seed, steps):
    """the calls of one walk behind walk_prologue(): drawn at random from the pool, 95 times in 100 among the calls that show a
    reader accepting or refusing for the first time in this walk, or that let the next call do so (found by trying them on copies of
    the shadow).  Deterministic in the seed."""
    import copy
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = walk_pool(name)
    distinct = list(dict.fromkeys(pool))
    shadow = replay(name, walk_prologue(name))
    seen, calls = set(), []

    def tried(s, c):
        t = copy.deepcopy(s)
        try:
            return t, reader_events(t, c, t.call(*c))
        except Unmodelled:
            return None, set()

    for k in range(steps):
        if k in ITINERARY:
            seen |= reader_events(shadow, ITINERARY[k], shadow.call(*ITINERARY[k]))
            calls.append(ITINERARY[k])
            continue
        after = [(c,) + tried(shadow, c) for c in distinct]
        modelled = {c for c, t, _ in after if t is not None}
        choice = None
        while choice not in modelled:
            choice = pool[int(rng.integers(len(pool)))]
        if rng.random() < 0.95:
            fresh = [c for c, _, ev in after if ev - seen]
            if not fresh:       # nothing new in one call: a call behind which a reader shows something new
                fresh = [c for c, t, _ in after if t is not None and c not in READERS.values() and any(tried(t, r)[1] - seen for r in READERS.values())]
            if fresh:
                choice = fresh[int(rng.integers(len(fresh)))]
        seen |= reader_events(shadow, choice, shadow.call(*choice))
        calls.append(choice)
    return calls


def replay(name, calls, shadow=None):
    """the calls on a shadow alone -> the shadow"""
    s = shadow or Shadow(name)
    for c in calls:
        s.call(*c)
    return s


# the plane group: mvs_sweep_run_planes takes groups of 32 planes, so a group that is not the whole volume needs more planes than the
# pool's tables have.  Its own baseline at 40 planes, the group [0, 32) under the other sampler, then a sweep of all of it
MANY = (40, -0.3, 0.3)
PLANE_GROUP = [("stage", MANY), ("sweep_run", 0, 3, BOTH), ("sweep_window", True, False), ("sweep_aggregate", False), ("set_sampler", "exact"),
               ("sweep_run_planes", 0, 3, 0, 32, VOLUME)]
DECODING = ("refine", "clean_views", "clean_unique", "clean_speckle", "clean_aggregated", "argmin", "aggregate", "window", "fetch_volume")
