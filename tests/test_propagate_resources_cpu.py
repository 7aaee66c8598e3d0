"""Resources of the propagation's kernels (csrc/propagate.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS:
propagate_seed and the 36 instantiations of propagate_pass, as in csrc/bestk.hip -- (five radii of the absolute difference + four of
ZNCC) times the four list sizes KMAX = 0 (MVS_KEEP_ALL), 2, 4, 8 -- none with scratch or spills.  Registers,
occupancy and LDS are printed."""
import os

import pytest

from kernel_resources import PKG, fixture

ABSDIFF, ZNCC = 0, 1
INSTANCES = [(cost, r, kmax) for cost, radii in ((ABSDIFF, (0, 1, 2, 3, 4)), (ZNCC, (1, 2, 3, 4))) for r in radii for kmax in (0, 2, 4, 8)]


resources = fixture("propagate.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(INSTANCES) == 36 and len(resources) == len(INSTANCES) + 1, sorted(resources)
    assert sum("14propagate_seed" in n for n in resources) == 1


@pytest.mark.parametrize("cost,r,kmax", INSTANCES)
def test_no_scratch_and_no_spills(resources, cost, r, kmax):
    tag = "14propagate_passILi%dELi%dELi%dEE" % (cost, r, kmax)
    names = [n for n in resources if tag in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(tag, {key: k[key] for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k


def test_the_seed_kernel_has_no_scratch_and_no_spills(resources):
    k = resources[[n for n in resources if "14propagate_seed" in n][0]]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k


def test_nothing_is_allocated_without_a_call():
    """the stage's maps and counters are two buffers of the context; only mvs_propagate_init makes them (behind every argument check),
    mvs_destroy frees them, and nothing else in the library names them"""
    import glob
    users = {}
    for path in glob.glob(os.path.join(PKG, "csrc", "*")):
        text = open(path, errors="replace").read()
        if "prop_maps" in text or "prop_counters" in text:
            users[os.path.basename(path)] = text
    assert sorted(users) == ["context.hip", "mvs_internal.hpp", "propagate.hip"], sorted(users)
    assert users["context.hip"].count("prop_") == 2 and "&ctx->prop_maps, &ctx->prop_counters," in users["context.hip"]     # the list mvs_destroy frees
    src = users["propagate.hip"]
    assert src.count("hipMalloc") == 0 and src.count("ensure(ctx, ctx->prop_") == 2
    body = src[src.index("int mvs_propagate_init("):src.index("int mvs_propagate_run(")]
    assert body.count("ensure(ctx, ctx->prop_") == 2 and body.index("ensure(ctx, ctx->prop_maps") > body.rindex("return fail(")   # behind the last refusal
    assert body.index("prop_have = true") > body.index("ensure(ctx, ctx->prop_counters")
