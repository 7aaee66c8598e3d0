"""The order in which the five fixed-sampler sweep entries refuse (csrc/sweep_shared.hpp: fx_sweep_run, and each entry's own argument
checks in front of it): every refusal of an entry's chain alone returns its own code and message, every two neighbours of the chain
violated together return the earlier one's, and no refused call moves a device buffer.  Only refused calls: no kernel runs."""
import re
import types

import pytest

import bestk_cases
import shadow_context as sc
from shadow_context import EINVAL, ESTATE

pytestmark = pytest.mark.gpu

PLANES = (7, -0.3, 0.3)      # the band's offsets inside (-1, 1)

# violation: (what it changes of the call or of the context, code, fragment of the message)
VIOLATIONS = {
    "null_prior": (dict(prior=False), EINVAL, "prior_dev is null"),
    "cost": (dict(cost=7), EINVAL, "unknown cost 7"),
    "radius": (dict(radius=9), EINVAL, "radius 9 outside"),
    "keep": (dict(keep=9), EINVAL, "keep 9 outside"),
    "tau": (dict(tau=256), EINVAL, "tau 256 outside 0..255"),
    "flag_bits": (dict(extra_flags=0x10), EINVAL, "unknown flag bits 0x10"),
    "no_output": (dict(flags=0), EINVAL, "flags select neither volume nor fused argmin"),
    "not_staged": (dict(staged=False), ESTATE, "set main view, side views and planes first"),
    "exact_sampler": (dict(sampler="exact"), ESTATE, "implemented for MVS_SAMPLER_FIXED"),
    "view_range": (dict(first=4, count=9), EINVAL, "view range [4,13) outside 0..6"),
    "offset": (dict(planes=(7, -0.3, 1.5)), ESTATE, "must lie inside (-1, 1): offset 5 is 1.1"),      # cell centres: -0.3 + 5.5 * 1.8 / 7
    "small_volume": (dict(small_volume=True), EINVAL, "caller volume is 16 bytes"),
}
TAIL = ["flag_bits", "no_output", "not_staged", "exact_sampler", "view_range", "small_volume"]
BAND_TAIL = TAIL[:-1] + ["offset", "small_volume"]
# entry: (its chain of refusals, the call on a Context)
ENTRIES = {
    "zncc": (["radius"] + TAIL, lambda c, a: c.sweep_run_zncc(a.radius, a.first, a.count, a.flags)),
    "bestk": (["cost", "radius", "keep"] + TAIL, lambda c, a: c.sweep_run_bestk(a.cost, a.radius, a.keep, a.first, a.count, a.flags)),
    "band_bestk": (["null_prior", "cost", "radius", "keep"] + BAND_TAIL,
                   lambda c, a: c.sweep_run_band_bestk(a.prior, a.cost, a.radius, a.keep, a.first, a.count, a.flags)),
    "band": (["null_prior"] + BAND_TAIL, lambda c, a: c.sweep_run_band(a.prior, a.first, a.count, a.flags)),
    "bestk_gated": (["cost", "radius", "keep", "tau"] + TAIL,
                    lambda c, a: c.sweep_run_bestk_gated(a.cost, a.radius, a.keep, a.tau, None, a.first, a.count, a.flags)),
}
CASES = [(entry, (v,)) for entry, (chain, _) in ENTRIES.items() for v in chain] + \
        [(entry, pair) for entry, (chain, _) in ENTRIES.items() for pair in zip(chain, chain[1:])]


@pytest.fixture(scope="module")
def contexts():
    """a context staged with the crafted case and one with nothing staged, a prior and a caller's volume of 16 bytes"""
    import mvs_amd
    import torch
    case = bestk_cases.crafted()
    staged, bare = mvs_amd.Context(case.W, case.H, 0), mvs_amd.Context(case.W, case.H, 0)
    staged.sweep_set(*case.views(), *PLANES)
    prior = torch.zeros(case.W * case.H, dtype=torch.float32, device="cuda")
    small = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    yield types.SimpleNamespace(staged=staged, bare=bare, prior=prior, small=small)
    staged.close()
    bare.close()


def _pointers(ctx):
    return sc.Device.pointers(types.SimpleNamespace(ctx=ctx))


@pytest.mark.parametrize("entry,violated", CASES, ids=["%s-%s" % (e, "+".join(v)) for e, v in CASES])
def test_the_earliest_refusal_answers(contexts, entry, violated):
    import mvs_amd
    a = dict(prior=True, cost=bestk_cases.ABSDIFF, radius=1, keep=2, tau=30, first=0, count=3, flags=mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN,
             extra_flags=0, staged=True, sampler="fixed", planes=PLANES, small_volume=False)
    for v in violated:
        a.update(VIOLATIONS[v][0])
    a = types.SimpleNamespace(**a)
    a.flags |= a.extra_flags
    a.prior = contexts.prior.data_ptr() if a.prior else None
    ctx = contexts.staged if a.staged else contexts.bare
    ctx.set_sampler(a.sampler)
    if a.staged:
        ctx.sweep_set_planes(*a.planes)
    if a.small_volume:
        ctx.sweep_use_volume(contexts.small.data_ptr(), 16)
    try:
        before = _pointers(ctx)
        with pytest.raises(mvs_amd.MvsError) as e:
            ENTRIES[entry][1](ctx, a)
        after = _pointers(ctx)
    finally:
        ctx.sweep_use_volume(None, 0)
        ctx.set_sampler("fixed")
        if a.staged:
            ctx.sweep_set_planes(*PLANES)
    code, message = re.match(r"libmvs_hip error (-?\d+): (.*)", str(e.value), re.S).groups()
    _, want_code, fragment = VIOLATIONS[violated[0]]
    print("%s %s -> %s: %s" % (entry, "+".join(violated), code, message))
    assert int(code) == want_code and fragment in message and message.startswith("mvs_sweep_run_%s: " % entry), (code, message)
    assert after == before, "a refused call moved a buffer"
