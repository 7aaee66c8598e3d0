"""Resources of the appearance kernels (csrc/tsdf.hip, csrc/appearance.hip) from the compiler's report for gfx950 with the Makefile's own
CXXFLAGS: no scratch, no spills and at most 96 VGPRs, and the kernels of mvs_tsdf_integrate, whose bodies the new
ones share, keep the figures of DESIGN.md section 12's table."""
import os
import shutil
import subprocess

import pytest

from test_rect_resources_cpu import HIPCC, PKG, _makefile_flags


def _report(tmp, source):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library"
    r = subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-c", os.path.join("csrc", source), "-o", str(tmp / (source + ".o")),
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


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("appearance")
    kernels = _report(tmp, "tsdf.hip")
    kernels.update(_report(tmp, "appearance.hip"))
    return kernels


def _one(resources, kernel):
    names = [n for n in resources if kernel + "E" in n]   # (the mangled name ends in E before the argument types: no prefix matches)
    assert len(names) == 1, sorted(resources)
    return resources[names[0]]


@pytest.mark.parametrize("kernel", ["23tsdf_wmap_frames_kernel", "28tsdf_integrate_frames_kernel", "17tsdf_shade_kernel", "18tsdf_sample_kernel"])
def test_no_scratch_and_no_spills(resources, kernel):
    k = _one(resources, kernel)
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) <= 96 and int(k["AGPRs"]) == 0, k


@pytest.mark.parametrize("kernel, vgprs, sgprs", [("16tsdf_wmap_kernel", 11, 44), ("21tsdf_integrate_kernel", 33, 47), ("17tsdf_field_kernel", 17, 26)])
def test_the_integration_kernels_keep_their_figures(resources, kernel, vgprs, sgprs):
    k = _one(resources, kernel)
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    assert (int(k["VGPRs"]), int(k["TotalSGPRs"])) == (vgprs, sgprs), k
