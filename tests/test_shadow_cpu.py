"""The premises of tests/test_shadow_gpu.py, with the mirrors alone: the shadow context (tests/shadow_context.py) makes the transitions
DESIGN.md section 13 writes down; a stale or mis-decoded read would be seen; the matrix and the seeded walks reach what they are meant
to reach; the shadow is deterministic."""
import itertools

import numpy as np
import pytest

import shadow_context as sc
from shadow_context import BOTH, ESTATE, FUSED, OK, VOLUME

WALK_SEEDS, WALK_STEPS = sc.WALK_SEEDS, sc.WALK_STEPS

# section 13's state paragraph as a table.  Every writer runs behind two states: A = the prologue and a resolved band run (a selection
# over the current planes, a band run), B = the prologue and a band run with MVS_SWEEP_VOLUME alone (no selection, a band run).
#   writer: (selection after A, selection after B, rows pending after B, band run after A)
KEPT = (True, False, False, True)               # leaves the selection state alone
MADE = (True, True, False, True)                # makes a selection over all rows, the band run stays
SWEEP_FUSED = (True, True, False, False)        # an ordinary sweep with a selection: ends the band run
SWEEP_VOLUME = (False, False, False, False)     # zncc / best-K with the volume alone: ends the selection and the band run
TRANSITIONS = {
    "run_volume": (True, False, False, False),  # mvs_sweep_run with the volume alone does NOT end the selection; ends the band run
    "run_fused": SWEEP_FUSED, "run_both": SWEEP_FUSED,
    "rows_part": (True, False, True, False),    # bands over the count the map already has keep a selection; else rows are pending
    "rows_all": SWEEP_FUSED,
    "rows_other_count": (False, False, True, False),
    "zncc_volume": SWEEP_VOLUME, "zncc_fused": SWEEP_FUSED, "zncc_both": SWEEP_FUSED,
    "bestk_volume": SWEEP_VOLUME, "bestk_fused": SWEEP_FUSED, "bestk_both": SWEEP_FUSED,
    "gated_volume": SWEEP_VOLUME, "gated_fused": SWEEP_FUSED, "gated_both": SWEEP_FUSED,
    "band_volume": (False, False, False, True), "band_fused": MADE, "band_both": MADE,
    "band_bestk_volume": (False, False, False, True), "band_bestk_fused": MADE, "band_bestk_both": MADE,
    "argmin": MADE, "combine_partials": MADE, "aggregate": MADE, "aggregate_refine": MADE, "window_select": MADE, "window_refine": MADE,
    "window": KEPT, "clean": KEPT,
    "planes_new_count": (False, False, False, True),     # ends nothing by itself: the readers compare the counts
    "planes_same_count": KEPT, "views_fewer": KEPT, "set_sampler": KEPT, "set_sampler_and_back": KEPT, "set_source": KEPT, "use_volume": KEPT,
    "use_volume_and_back": (True, False, False, False),  # (it sweeps into the caller's volume in between)
    "rows_other_sampler": (True, False, False, False), "rows_other_sampler_then_all": (True, False, False, False),
    "pyramid_prior": (True, False, False, False),        # a new prior ends the band run (section 30)
}
STATE_A = sc.BAND_RUN
STATE_B = [("sweep_run_band", "crafted", 0, 3, VOLUME)]


def _name_of(writer):
    return "even" if writer == "pyramid_prior" else "crafted"


@pytest.mark.parametrize("writer", sorted(TRANSITIONS))
def test_transitions_of_section_13(writer):
    name = _name_of(writer)
    calls = sc.writers(name)[writer]
    a = sc.replay(name, sc.prologue(name) + STATE_A + calls)
    b = sc.replay(name, sc.prologue(name) + STATE_B + calls)
    got = (a._selection_current(), b._selection_current(), b.sel_band_planes != 0, a.band_planes != 0)
    assert got == TRANSITIONS[writer], a.story()


def test_the_table_names_every_writer():
    assert set(TRANSITIONS) == set(sc.writers("crafted")) | set(sc.writers("even"))
    assert set(sc.writers("even")) - set(sc.writers("crafted")) == {"pyramid_prior"}


# ---- a stale or mis-decoded read would be seen ---------------------------------------------------------------------------------------
def _pool():
    """what a walk can put on one context: (label, volume, maps) of every sweep of the pool at every plane table"""
    V = sc.inputs("crafted").V
    out = []
    for tab in sc.TABLES:
        for first, count in ((0, V), (0, 3), (0, 2)):
            for sampler in ("fixed", "exact"):
                d, c, i, vol = sc.mirror_sweep("crafted", first, count, tab, sampler)
                out.append((("run", sampler, count, tab), vol, (d, c, i)))
    for calls in sc.writers("crafted").values():
        for call in calls:
            if call[0] in ("sweep_run_zncc", "sweep_run_bestk", "sweep_run_bestk_gated", "sweep_run_band", "sweep_run_band_bestk") and call[-1] == BOTH:
                s = sc.replay("crafted", sc.prologue("crafted") + [call])
                assert s.history[-1][-1] == OK
                out.append(((call[0], s.tab), s.fetched("volume").copy(), s.fetched("maps")))
    return out


def test_two_pool_entries_never_look_alike():
    pool = _pool()
    counts = []
    for (la, va, ma), (lb, vb, mb) in itertools.combinations(pool, 2):
        n = min(va.size, vb.size)               # after a change of the plane count a reader sees the old cells under the new count
        dv = int((va.ravel()[:n] != vb.ravel()[:n]).sum())
        dm = [int((sc.bits(x) != sc.bits(y)).sum()) for x, y in zip(ma, mb)]
        counts.append((dv, dm))
        assert dv > 0 and all(k > 0 for k in dm), (la, lb, dv, dm)
    print("pairs %d; differing cells min %d; differing depth / cost / index pixels min %s" % (
        len(counts), min(c[0] for c in counts), [min(c[1][k] for c in counts) for k in range(3)]))


@pytest.mark.parametrize("written,read", [("fixed", "exact"), ("exact", "fixed")])
def test_cells_decoded_in_the_other_layout_give_other_maps(written, read):
    """finding 1: the volume written under one sampler and refined or cleaned under the other differs from the correct result"""
    o = sc._oracle()
    z = sc.table(sc.LARGEST)
    d, c, i, vol = sc.mirror_sweep("crafted", 0, 6, sc.LARGEST, written)
    right = o.refine_depth(vol, z, i, sampler=written)
    wrong = o.refine_depth(vol, z, i, sampler=read)
    n_refine = int((sc.bits(right) != sc.bits(wrong)).sum())
    import clean_mirror
    kw = dict(min_views=2, uniqueness=10)
    right = clean_mirror.clean(d, c, i, vol=vol, cs=sc.CS[written], **kw)
    wrong = clean_mirror.clean(d, c, i, vol=vol, cs=sc.CS[read], **kw)
    n_clean = int((right[2] != wrong[2]).sum())
    print("written %s, read %s: %d refined depths and %d cleaned indices differ" % (written, read, n_refine, n_clean))
    assert n_refine > 0 and n_clean > 0 and right[3] != wrong[3]


def test_the_new_prior_differs_where_there_is_an_index():
    """finding 2: prior A and the rule-U prior B differ at pixels that hold an index, and so do the resolved depths"""
    import band_mirror
    s = sc.replay("even", sc.prologue("even") + sc.BAND_RUN)
    a, index, offsets = s.band_prior.copy(), s.maps[2], s.maps[0]
    s.call("pyramid_prior")
    b = s.band_prior
    held = index >= 0
    n = int((sc.bits(a) != sc.bits(b))[held].sum())
    wrong = band_mirror.resolve(b, offsets, index)
    print("%d of %d pixels with an index have another prior; %d resolved depths differ" % (n, int(held.sum()), int((sc.bits(wrong) != sc.bits(s.band_depth)).sum())))
    assert n > held.sum() // 2 and (sc.bits(wrong) != sc.bits(s.band_depth))[held].any()
    assert s.call("band_resolve") == ESTATE and s.fetch_code("band_fetch") == ESTATE and s.fetch_code("band_report") == ESTATE


# ---- coverage is a condition --------------------------------------------------------------------------------------------------------
WRITERS = """run_volume run_fused run_both rows_part rows_all rows_other_count zncc_volume zncc_fused zncc_both bestk_volume bestk_fused bestk_both
gated_volume gated_fused gated_both band_volume band_fused band_both band_bestk_volume band_bestk_fused band_bestk_both argmin combine_partials aggregate
aggregate_refine window window_select window_refine clean planes_new_count planes_same_count views_fewer set_sampler set_sampler_and_back
set_source use_volume use_volume_and_back rows_other_sampler rows_other_sampler_then_all""".split()
READERS = """refine clean_views clean_unique clean_speckle clean_aggregated band_resolve band_report band_fetch argmin aggregate window window_fetch
aggregate_fetch clean_report clean_sizes fetch_volume depth_filter propagate_depth propagate_prior""".split()


def test_the_matrix_holds_every_writer_with_every_reader():
    ids = {cid for cid, _, _ in sc.matrix("crafted")}
    assert ids == {"%s-%s" % (w, r) for w in WRITERS for r in READERS}
    assert {cid for cid, _, _ in sc.matrix("even") if cid.startswith("pyramid_prior-")} == {"pyramid_prior-" + r for r in READERS}


def test_the_findings_are_cases_of_the_matrix():
    """the readers behind a sampler switch refuse, and so do the band readers behind a new prior; each of these is accepted behind
    some other writer"""
    codes = {}
    for name in ("crafted", "even"):
        for cid, before, call in sc.matrix(name):
            s = sc.replay(name, before)
            codes[cid] = s.call(*call)
    decoding = ("refine", "clean_views", "clean_unique", "clean_speckle", "clean_aggregated", "argmin", "aggregate", "window", "fetch_volume")
    for r in decoding:
        assert codes["set_sampler-" + r] == ESTATE and codes["set_sampler_and_back-" + r] == OK and codes["run_both-" + r] == OK, r
    for r in decoding:       # a volume of both layouts is read under neither sampler, until a sweep has written all of it
        assert codes["rows_other_sampler-" + r] == ESTATE and codes["rows_other_sampler_then_all-" + r] == OK, r
    for r in ("band_resolve", "band_report", "band_fetch"):
        assert codes["pyramid_prior-" + r] == ESTATE and codes["argmin-" + r] == OK, r
    refused = sorted(cid for cid, rc in codes.items() if rc != OK)
    print("%d of %d cases end in a refusal" % (len(refused), len(codes)))


def _walk(seed):
    calls = sc.walk_calls("crafted", seed, WALK_STEPS)
    s = sc.replay("crafted", sc.walk_prologue("crafted"))
    seen = set()
    for c in calls:
        seen |= sc.reader_events(s, c, s.call(*c))
    return calls, s, seen


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_walks_reach_every_reader(seed):
    """behind the walk's change of the plane count every reader is accepted at least once and -- where the contract has a refusal --
    refused at least once; the walk visits the plane tables, both volume sources, a caller's volume and back, and both samplers"""
    calls, s, seen = _walk(seed)
    assert len(calls) == WALK_STEPS and sc.walk_prologue("crafted")[-1][0] == "set_planes"
    assert not sc.wanted_events() - seen, sorted(sc.wanted_events() - seen)
    assert len({c[1][0] for c in calls if c[0] == "set_planes"}) >= 3
    assert {c[1] for c in calls if c[0] == "set_source"} == {"raw", "windowed"} and {c[1] for c in calls if c[0] == "use_volume"} == {True, False}
    samplers = set()
    t = sc.replay("crafted", sc.walk_prologue("crafted"))
    for c in calls:
        t.call(*c)
        samplers.add(t.sampler)
    assert samplers == {"fixed", "exact"}
    refused_windowed = [h for h in s.history if h[0] in ("sweep_run_zncc", "sweep_run_bestk", "sweep_run_bestk_gated", "sweep_run_band", "sweep_run_band_bestk") and h[-1] == ESTATE]
    print("seed %d: %d calls refused, %d of them windowed or band sweeps under the exact sampler" % (seed, sum(h[-1] != OK for h in s.history), len(refused_windowed)))


def test_walks_make_every_call_between_them():
    made = set()
    for seed in WALK_SEEDS:
        made |= {c[0] for c in sc.walk_calls("crafted", seed, WALK_STEPS)}
    assert made >= {c[0] for c in sc.walk_pool("crafted")} - {"fetch"}      # (compare() makes the fetches behind every step)


def test_the_shadow_is_deterministic():
    a, b = _walk(WALK_SEEDS[0]), _walk(WALK_SEEDS[0])
    assert a[0] == b[0] and a[1].history == b[1].history and a[1].snapshot() == b[1].snapshot()


def test_a_plane_group_under_the_other_sampler_is_read_by_nobody():
    """the premise of the GPU module's plane-group test, on the shadow alone: refused under either sampler, accepted behind a sweep of
    the whole volume; a group that is the whole volume leaves no mixture"""
    for reader in sc.DECODING:
        s = sc.replay("crafted", sc.PLANE_GROUP, sc.Shadow("crafted", sc.MANY))
        assert s.own_cells == "mixed"
        for sampler in ("exact", "fixed"):
            s.call("set_sampler", sampler)
            assert s.call(*sc.READERS[reader]) == ESTATE, reader
        assert s.call("sweep_run", 0, 3, VOLUME) == OK and s.call(*sc.READERS[reader]) == OK, reader
    s = sc.replay("crafted", sc.prologue("crafted") + [("set_sampler", "exact"), ("sweep_run_planes", 0, 3, 0, 19, VOLUME)])
    assert s.history[-1][-1] == OK and s.own_cells == "exact"
    assert s.call("sweep_run_planes", 0, 3, 0, 8, VOLUME) == sc.EINVAL and s.call("sweep_run_planes", 0, 3, 0, 19, BOTH) == sc.EINVAL


def test_the_tabulated_state_is_assigned_by_the_named_transitions_only():
    """section 30's state changes in mvs_internal.hpp (the fields' initialisers and the note_* transitions) and in note_rows_selected
    (select.hip), nowhere else in csrc"""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mesh-reconstruction_amd", "csrc")
    fields = "sel_planes sel_band_planes sel_band_lo sel_band_hi band_planes band_resolved vol_cells_sampler own_cells_sampler win_cells_sampler win_planes".split()
    assigned = re.compile(r"\b(%s)\s*([-+*/|&^]?=(?!=)|\+\+|--)" % "|".join(fields))
    found = []
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        text = open(path, errors="replace").read()
        if os.path.basename(path) == "mvs_internal.hpp":
            assert len(assigned.findall(text)) >= len(fields)       # the check sees assignments where they are
            continue
        if os.path.basename(path) == "select.hip":
            m = re.search(r"^void note_rows_selected\(.*?^}\n", text, re.M | re.S)
            assert m and assigned.search(m.group(0))
            text = text.replace(m.group(0), "")
        found += ["%s: %s" % (os.path.basename(path), line.strip()) for line in text.splitlines() if assigned.search(line)]
    assert not found, found
