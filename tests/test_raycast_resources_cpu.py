"""Resources of the ray-cast kernels (csrc/raycast.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch,
no spills, and few enough registers that the 32 KiB brick mask in LDS, not the register file, bounds the ray kernel's
occupancy (5 workgroups of 4 wavefronts per CU need <= 96 VGPRs)."""
import os
import shutil
import subprocess

import pytest

from test_rect_resources_cpu import HIPCC, PKG, _makefile_flags


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library"
    out = str(tmp_path_factory.mktemp("raycast") / "raycast.o")
    r = subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-c", os.path.join("csrc", "raycast.hip"), "-o", out,
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


@pytest.mark.parametrize("kernel", ["tsdf_raycast_kernelILb0E", "tsdf_raycast_kernelILb1E", "tsdf_brick_kernel"])
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if kernel in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) <= 96 and int(k["AGPRs"]) == 0, k
