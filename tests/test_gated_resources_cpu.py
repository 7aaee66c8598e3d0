"""Resources of the guide-gated best-K sweep's kernel (csrc/bestk_gated.hip) from the compiler's report for gfx950 with the Makefile's own
CXXFLAGS: exactly 32 kernels -- two costs times the radii 1..4 times the list sizes KMAX = 0 (MVS_KEEP_ALL), 2, 4, 8 -- none with scratch
or spills.  Registers, occupancy and LDS are printed.  And the allocation check of section 22: the entry allocates
what mvs_sweep_run_bestk allocates, behind every argument check, and nothing else in the library knows of it."""
import glob
import os

import pytest

from kernel_resources import PKG, fixture

ABSDIFF, ZNCC = 0, 1
INSTANCES = [(cost, r, kmax) for cost in (ABSDIFF, ZNCC) for r in (1, 2, 3, 4) for kmax in (0, 2, 4, 8)]
SOURCE = os.path.join(PKG, "csrc", "bestk_gated.hip")


resources = fixture("bestk_gated.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(INSTANCES) == 32 and len(resources) == len(INSTANCES), sorted(resources)


@pytest.mark.parametrize("cost,r,kmax", INSTANCES)
def test_no_scratch_and_no_spills(resources, cost, r, kmax):
    tag = "20sweep_fx_bestk_gatedILi%dELi%dELi%dEE" % (cost, r, kmax)
    names = [n for n in resources if tag in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(tag, {key: k[key] for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k


def test_only_the_entrys_own_path_allocates():
    """the entry makes what mvs_sweep_run_bestk makes (the maps, the volume of a volume run, the weight table) through the one body of the fixed-sampler
    entries (fx_sweep_run), behind its last refusal and behind the shared ones; it has no buffer of its own on the context, and the sweeps it is not to touch do not name it"""
    src = open(SOURCE).read()
    assert src.count("hipMalloc") == 0 and src.count("ensure(") == 0 and src.count("DevBuf") == 0
    body = src[src.index("int mvs_sweep_run_bestk_gated("):]
    assert body.count("fx_sweep_run(") == 1
    run = body.index("fx_sweep_run(")
    assert body.rindex("return fail(") < run                                                          # every check of its own comes first
    for check in ("null context", "unknown cost", "radius %d outside 1..4", "keep %d outside", "tau %d outside 0..255"):
        assert check in body[:run], check
    shared = open(os.path.join(PKG, "csrc", "sweep_shared.hpp")).read()
    shared = shared[shared.index("inline int fx_sweep_run("):]
    shared = shared[:shared.index("\n}\n")]
    assert shared.index("fx_sweep_preconditions(") < min(shared.index("sweep_outputs("), shared.index("ensure("), shared.index("ensure_fx_lut("))
    users = sorted(os.path.basename(p) for p in glob.glob(os.path.join(PKG, "csrc", "*")) if "bestk_gated" in open(p, errors="replace").read())
    assert users == ["bestk_gated.hip"], users          # no state of the sweep's on the context, no caller inside the library


def test_the_propagation_gate_adds_no_allocation_and_no_kernel():
    """the gate is two kernel arguments and H * W bytes behind the five maps of the one allocation; its fields have default initialisers"""
    src = open(os.path.join(PKG, "csrc", "propagate.hip")).read()
    assert "5 * P * sizeof(float) + P" in src and src.count("__global__") == 2
    internal = open(os.path.join(PKG, "csrc", "mvs_internal.hpp")).read()
    assert "int prop_gate_tau = 255;" in internal and "const void *prop_gate_guide = nullptr;" in internal and "int prop_tau = 255;" in internal
