"""The depth-map filter without a GPU: the three symbols and the three constants of include/mvs.h as the library
exports and the binding states them; the filter's buffers belong to csrc/depth_filter.hip alone, so a context that never calls it
allocates nothing for it; and the kernels' resources from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any instantiation (four radii, gated by a guide or not, median and mean)."""
import glob
import os
import re

import pytest

import mvs_amd
from kernel_resources import PKG, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# depth_filter_median<R, GATED>, depth_filter_mean<R, GATED>
KERNELS = ["%sILi%dELb%dEE" % (stage, r, g) for stage in ("19depth_filter_median", "17depth_filter_mean") for r in (1, 2, 3, 4) for g in (0, 1)]
SYMBOLS = ("mvs_depth_filter", "mvs_depth_filtered_device", "mvs_depth_filter_fetch")


def test_symbols_and_constants():
    lib = mvs_amd.load_library()
    bound = {n: (res, args) for n, res, args in mvs_amd.ABI}
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in bound, name
    assert len(bound["mvs_depth_filter"][1]) == 8 and len(bound["mvs_depth_filter_fetch"][1]) == 2
    header = open(os.path.join(ROOT, "include", "mvs.h")).read()
    for name, value in (("MVS_FILTER_MEDIAN", 1), ("MVS_FILTER_MEAN", 2), ("MVS_FILTER_FILL", 4)):
        m = re.search(r"^#define %s (\d+)u$" % name, header, re.M)
        assert m and int(m.group(1)) == value == getattr(mvs_amd, name), name
    # without a context there is nothing to fetch and no map
    assert lib.mvs_depth_filtered_device(None) is None
    assert lib.mvs_depth_filter(None, None, None, 1, 255, 0.0, 1, 1) == -1 and lib.mvs_depth_filter_fetch(None, None) == -1


def test_nothing_is_allocated_without_a_call():
    """the filtered map and the intermediate map are one buffer of the context; only mvs_depth_filter makes it (one ensure() behind the
    argument checks), mvs_destroy frees it, and nothing else in the library names it"""
    users = {}
    for path in glob.glob(os.path.join(PKG, "csrc", "*")):
        text = open(path, errors="replace").read()
        if "dfilter_" in text:
            users[os.path.basename(path)] = text
    assert sorted(users) == ["context.hip", "depth_filter.hip", "mvs_internal.hpp"], sorted(users)
    assert users["context.hip"].count("dfilter_") == 1 and "&ctx->dfilter_maps}" in users["context.hip"]     # the list mvs_destroy frees
    src = users["depth_filter.hip"]
    assert src.count("ensure(") == 1 and src.count("hipMalloc") == 0
    body = src[src.index("int mvs_depth_filter("):]
    assert body.index("ensure(ctx, ctx->dfilter_maps") > body.index("needs a guide image")       # behind the last refusal
    assert body.count("dfilter_have = true") == 1 and body.index("dfilter_have = true") > body.index("ensure(ctx, ctx->dfilter_maps")


resources = fixture("depth_filter.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(KERNELS) == 16 and len(resources) == len(KERNELS), sorted(resources)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if kernel in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(kernel, {key: k[key] for key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    # the window's keys live in registers: (2R + 1)^2 of them and a dozen more, far from the 512 a SIMD has for one wavefront
    assert int(k["VGPRs"]) + int(k["AGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
