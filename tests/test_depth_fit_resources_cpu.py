"""The depth-map plane fit without a GPU: the ten symbols of include/mvs.h as the library exports and the binding
states them; the stage's one buffer belongs to csrc/depth_fit.hip alone, made by mvs_depth_fit behind its last refusal, so a context that
never fits allocates nothing; the propagation's file gained host lines only; and the kernels' resources from the compiler's report for
gfx950 with the Makefile's own CXXFLAGS: exactly ten kernels, no scratch and no spills (section 32's table is this output)."""
import glob
import os
import re

import pytest

import mvs_amd
from kernel_resources import PKG, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# depth_fit_plane<R, GATED>, depth_fit_normals_kernel, depth_fit_seed_kernel
PLANE = ["15depth_fit_planeILi%dELb%dEE" % (r, g) for r in (1, 2, 3, 4) for g in (0, 1)]
KERNELS = PLANE + ["24depth_fit_normals_kernelE", "21depth_fit_seed_kernelE"]
SYMBOLS = {"mvs_depth_fit": 7, "mvs_depth_fit_device": 1, "mvs_depth_fit_depth_device": 1, "mvs_depth_fit_members_device": 1, "mvs_depth_fit_fetch": 6,
           "mvs_depth_fit_report": 2, "mvs_depth_fit_normals": 2, "mvs_depth_fit_normals_device": 1, "mvs_depth_fit_normals_fetch": 2, "mvs_propagate_set_slopes": 3}
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def test_symbols():
    lib = mvs_amd.load_library()
    bound = {n: (res, args) for n, res, args in mvs_amd.ABI}
    header = open(os.path.join(ROOT, "include", "mvs.h")).read()
    for name, nargs in SYMBOLS.items():
        assert hasattr(lib, name) and name in bound and len(bound[name][1]) == nargs, name
        assert re.search(r"^(int|void \*)\s*%s\(mvs_ctx \*ctx" % name, header, re.M), name
    # without a context there are no maps and nothing to fetch
    for name in ("mvs_depth_fit_device", "mvs_depth_fit_depth_device", "mvs_depth_fit_members_device", "mvs_depth_fit_normals_device"):
        assert getattr(lib, name)(None) is None
    assert lib.mvs_depth_fit(None, None, None, 1, 255, 0.0, 3) == -1 and lib.mvs_depth_fit_fetch(None, None, None, None, None, None) == -1
    assert lib.mvs_depth_fit_report(None, None) == -1 and lib.mvs_depth_fit_normals(None, None) == -1 and lib.mvs_depth_fit_normals_fetch(None, None) == -1
    assert lib.mvs_propagate_set_slopes(None, None, None) == -1
    for method in ("depth_fit", "depth_fit_pointers", "depth_fit_report", "depth_fit_normals", "depth_fit_normals_pointer", "propagate_set_slopes"):
        assert callable(getattr(mvs_amd.Context, method)), method


def test_nothing_is_allocated_without_a_call():
    """the stage's maps, counters and bytes are one buffer of the context; only mvs_depth_fit makes it (one ensure() behind the argument
    checks), mvs_destroy frees it, and nothing else in the library names it"""
    users = {}
    for path in glob.glob(os.path.join(PKG, "csrc", "*")):
        text = open(path, errors="replace").read()
        if "dfit_maps" in text:
            users[os.path.basename(path)] = text
    assert sorted(users) == ["context.hip", "depth_fit.hip", "mvs_internal.hpp"], sorted(users)
    assert users["context.hip"].count("dfit_") == 1 and "&ctx->dfit_maps," in users["context.hip"]           # the list mvs_destroy frees
    assert users["mvs_internal.hpp"].count("mvs::DevBuf dfit_") == 1
    src = users["depth_fit.hip"]
    assert src.count("ensure(") == 1 and src.count("hipMalloc") == 0
    body = src[src.index("int mvs_depth_fit("):src.index("void *mvs_depth_fit_device(")]
    assert body.index("ensure(ctx, ctx->dfit_maps") > body.rindex("return fail(") and body.index("needs a guide image") < body.index("ensure(")
    assert body.count("dfit_have = true") == 1 and body.index("dfit_have = true") > body.index("launch_fit<") > body.index("ensure(ctx, ctx->dfit_maps")
    assert "Synchronize" not in body
    # the other calls allocate nothing and write no flag before their last refusal
    normals = src[src.index("int mvs_depth_fit_normals("):src.index("void *mvs_depth_fit_normals_device(")]
    assert normals.index("dfit_normals_have = true") > normals.index("<<<") > normals.rindex("return fail(") and "Synchronize" not in normals
    setter = src[src.index("int mvs_propagate_set_slopes("):]
    assert setter.index("ctx->dfit_seed_gx = gx_dev") > setter.rindex("return fail(") and "hip" not in setter.split("{", 1)[1], "the setter only records"


def test_the_propagation_gained_host_lines_only():
    """the seed kernel and its launch live in depth_fit.hip behind one function; mvs_propagate_init refuses the combined flag among its
    refusals, calls the function behind its seed launch, and the record is cleared where it is consumed"""
    prop = open(os.path.join(PKG, "csrc", "propagate.hip")).read()
    assert prop.count("__global__") == 2 and prop.count("dfit_") == 2
    init = prop[prop.index("int mvs_propagate_init("):prop.index("int mvs_propagate_run(")]
    assert init.index("ctx->dfit_seed_gx)") < init.index("staged_state(") < init.index("ensure(ctx, ctx->prop_maps")
    assert init.index("propagate_seed<<<") < init.index("dfit_seed_slopes(ctx, ") < init.index("pass(ctx, a)")
    fit = open(os.path.join(PKG, "csrc", "depth_fit.hip")).read()
    seed = fit[fit.index("void dfit_seed_slopes("):fit.index("using namespace mvs;")]
    assert seed.index("if (!ctx->dfit_seed_gx) return;") < seed.index("<<<") < seed.index("ctx->dfit_seed_gx = ctx->dfit_seed_gy = nullptr")
    users = sorted(os.path.basename(p) for p in glob.glob(os.path.join(PKG, "csrc", "*")) if "dfit_seed_" in open(p, errors="replace").read())
    assert users == ["depth_fit.hip", "mvs_internal.hpp", "propagate.hip"], users


resources = fixture("depth_fit.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(KERNELS) == 10 and len(resources) == len(KERNELS), sorted(resources)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if kernel in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(kernel, {key: k[key] for key in KEYS if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    if kernel in PLANE:
        # the tile and its halo: (32 + 2R)(8 + 2R) values, and as many guide bytes when gated; at most 40 x 16 x 5 bytes
        r, gated = int(kernel[len("15depth_fit_planeILi")]), kernel.endswith("Lb1EE")
        cells = (32 + 2 * r) * (8 + 2 * r)
        assert cells * 4 <= int(k["LDS Size [bytes/block]"]) <= cells * (5 if gated else 4) + 16 <= 40 * 16 * 5 + 16, k
        # nine accumulators and the window walk's temporaries: far from the 512 registers a SIMD has for one wavefront
        assert int(k["VGPRs"]) + int(k["AGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
    else:
        assert int(k["LDS Size [bytes/block]"]) == 0, k
