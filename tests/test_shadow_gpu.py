"""Every call order of the sweep family against the shadow context (tests/shadow_context.py): each writer followed
by each reader on a fresh context, the bystanders, three seeded walks of 40 steps on one long-lived context each, and the refusals
repeated on poisoned allocations.  Everything that can be fetched is compared bit for bit, everything else must return the promised
code; a failure prints the call history of its context.  tests/test_shadow_cpu.py holds the premises."""
import numpy as np
import pytest

import shadow_context as sc
from shadow_context import OK, WALK_SEEDS, WALK_STEPS

pytestmark = pytest.mark.gpu

MATRIX = {cid: (name, before, call) for name in ("crafted", "even") for cid, before, call in sc.matrix(name)
          if name == "crafted" or cid.startswith("pyramid_prior-")}


def _run(name, calls, compare_each=False, largest=sc.LARGEST):
    """the calls on a fresh shadow and a fresh context; the codes agree -> (shadow, device)"""
    shadow, device = sc.Shadow(name, largest), sc.Device(name, largest)
    try:
        for c in calls:
            if compare_each:
                sc.step(shadow, device, *c)
            else:
                want, rc = shadow.call(*c), device.call(*c)
                assert rc == want, "%s returned %d, the contract says %d, after\n%s" % (c, rc, want, shadow.story())
    except BaseException:
        device.close()
        raise
    return shadow, device


@pytest.mark.parametrize("cid", sorted(MATRIX))
def test_writer_then_reader(cid):
    """a fresh context: the baseline (a sweep with both outputs, a window with selection, an aggregation; a resolved band run for the
    band's readers), the writer, the reader, compare; then the two probes of the selection and the band state.  The two findings of section 30 are [set_sampler-*] and
    [pyramid_prior-band_resolve | band_report | band_fetch]"""
    name, before, call = MATRIX[cid]
    shadow, device = _run(name, before)
    try:
        pointers = device.pointers()
        rc = sc.step(shadow, device, *call)
        if rc != OK:
            assert device.pointers() == pointers, "a refused call moved a buffer, after\n" + shadow.story()
        for probe in sc.PROBES:
            sc.step(shadow, device, *probe)
    finally:
        device.close()


@pytest.mark.parametrize("reader", sc.DECODING)
def test_plane_group_under_the_other_sampler(reader):
    """a plane group swept after a sampler switch leaves cells of both layouts: every reader that decodes cells refuses, whichever
    sampler is set, until one sweep has written all of the volume"""
    shadow, device = _run("crafted", sc.PLANE_GROUP, largest=sc.MANY)
    try:
        sc.compare(shadow, device, "behind the plane group: ")
        for sampler in ("exact", "fixed"):
            sc.step(shadow, device, "set_sampler", sampler)
            assert sc.step(shadow, device, *sc.READERS[reader]) == sc.ESTATE
        assert sc.step(shadow, device, "sweep_run", 0, 3, sc.VOLUME) == OK
        assert sc.step(shadow, device, *sc.READERS[reader]) == OK
    finally:
        device.close()


@pytest.mark.parametrize("writer", ["zncc_volume", "bestk_volume", "gated_volume", "band_volume", "band_bestk_volume"])
def test_a_fixed_sampler_entry_rewrites_an_exact_volume(writer):
    """the volume was last written under the exact sampler; one of the fixed sampler's other entries then writes all of it: the cells
    are the fixed layout's and every reader takes them.  The matrix does not see this: its baseline volume has the fixed layout already,
    and a missing note_volume_written in these entries' common epilogue passed all of it"""
    rewritten = [("set_sampler", "exact"), ("sweep_run", 0, 3, sc.VOLUME), ("set_sampler", "fixed")] + sc.writers("crafted")[writer]
    shadow, device = _run("crafted", sc.prologue("crafted") + rewritten)
    try:
        assert shadow.own_cells == "fixed"
        sc.compare(shadow, device, "behind the rewrite: ")
        assert sc.step(shadow, device, *sc.READERS["argmin"]) == OK
    finally:
        device.close()


@pytest.mark.parametrize("which", sorted(sc.BYSTANDERS))
def test_bystanders_change_nothing(which):
    """calls of other stages and refused calls leave every fetchable of the family as it was"""
    name = "even" if which == "downsample" else "crafted"
    shadow, device = _run(name, sc.prologue(name) + sc.BAND_RUN + [("sweep_clean", 2, 10, 4, 1, False), ("depth_filter", 1, 255)])
    try:
        sc.compare(shadow, device, "before the bystander: ")
        own = {"depth_filter": ("filtered",), "propagate": ("prop", "prop_report")}.get(which, ())      # what the stage writes of its own
        before = shadow.snapshot()
        sc.step(shadow, device, *sc.BYSTANDERS[which])
        after = shadow.snapshot()
        assert {k: v for k, v in after.items() if k not in own} == {k: v for k, v in before.items() if k not in own}
    finally:
        device.close()


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_random_walks_on_one_context(seed):
    """40 steps over all calls on one context, everything compared after every step; then a fresh context that is given the accepted
    calls alone must equal the shadow too: if only the long-lived context differs, something leaked; if both do, a kernel and its mirror
    disagree"""
    calls = sc.walk_prologue("crafted") + sc.walk_calls("crafted", seed, WALK_STEPS)
    shadow, device = _run("crafted", calls, compare_each=True)
    device.close()
    accepted = [h[:-1] for h in shadow.history if h[-1] == OK]
    again, fresh = _run("crafted", accepted)
    try:
        assert again.snapshot() == shadow.snapshot()
        sc.compare(shadow, fresh, "a fresh context with the accepted calls alone: ")
    finally:
        fresh.close()


def _refusals(reader):
    out = []
    for cid, (name, before, call) in sorted(MATRIX.items()):
        if cid.endswith("-" + reader):
            s = sc.replay(name, before)
            if s.call(*call) != OK:
                out.append((cid, name, before, call))
    return out


@pytest.mark.parametrize("reader", sorted(sc.READERS))
def test_refused_calls_allocate_and_write_nothing(reader, monkeypatch):
    """every refusal of the matrix again, on contexts whose allocations come filled with 0xFF bytes: behind the refused call every
    buffer is where it was and holds what it held, fetched raw"""
    monkeypatch.setenv("MVS_POISON_ALLOC", "1")
    cases = _refusals(reader)
    if not cases:       # the baseline of the matrix holds a Wv, an S and a depth map: nothing behind it makes these three refuse
        assert reader in ("window_fetch", "aggregate_fetch", "depth_filter")
    for cid, name, before, call in cases:
        shadow, device = _run(name, before)
        try:
            pointers = device.pointers()
            held = [device.fetch(w) for w in sc.FETCHES if w != "volume" or shadow.volume_fetch_is_safe()]
            assert device.call(*call) == shadow.call(*call) != OK, cid
            assert device.pointers() == pointers, cid
            now = [device.fetch(w) for w in sc.FETCHES if w != "volume" or shadow.volume_fetch_is_safe()]
            for (rc0, a), (rc1, b) in zip(held, now):
                assert rc0 == rc1, cid
                if rc0 == OK:
                    for x, y in zip(a, b) if isinstance(a, tuple) else [(a, b)]:
                        assert (sc.bits(np.asarray(x)) == sc.bits(np.asarray(y))).all(), cid + "\n" + shadow.story()
        finally:
            device.close()
