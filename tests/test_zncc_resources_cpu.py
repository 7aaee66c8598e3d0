"""Resources of the ZNCC sweep's kernel (csrc/zncc.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any instantiation: four radii times three combinations of outputs."""
import os
import shutil
import subprocess

import pytest

from test_rect_resources_cpu import HIPCC, PKG, _makefile_flags

INSTANCES = [(r, vol, fused) for r in (1, 2, 3, 4) for vol, fused in ((1, 1), (1, 0), (0, 1))]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library"
    out = str(tmp_path_factory.mktemp("zncc") / "zncc.o")
    r = subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-c", os.path.join("csrc", "zncc.hip"), "-o", out,
                                                      "-Rpass-analysis=kernel-resource-usage"], cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        if "remark:" not in line or "[-Rpass-analysis" not in line:
            continue
        key, _, val = line.split("remark:", 1)[1].rsplit("[-Rpass-analysis", 1)[0].strip().rpartition(":")
        if key.strip() == "Function Name":
            cur = kernels.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return kernels


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(resources) == len(INSTANCES), sorted(resources)


@pytest.mark.parametrize("r,vol,fused", INSTANCES)
def test_no_scratch_and_no_spills(resources, r, vol, fused):
    tag = "13sweep_fx_znccILi%dELb%dELb%dEE" % (r, vol, fused)
    names = [n for n in resources if tag in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(tag, {key: k[key] for key in ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
