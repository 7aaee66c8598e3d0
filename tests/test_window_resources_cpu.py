"""Resources of the window kernels (csrc/window.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any kernel of the file, and no more vector registers of both kinds than a SIMD has for one wavefront (DESIGN.md
section 18)."""
import os
import shutil
import subprocess

import pytest

from test_rect_resources_cpu import HIPCC, PKG, _makefile_flags

# window_kernel<R, CS, GATED>: radius 0 is never gated
KERNELS = ["window_kernelILi0ELi%dELb0E" % cs for cs in (24, 16)] + \
          ["window_kernelILi%dELi%dELb%dE" % (r, cs, g) for r in (1, 2, 3, 4) for cs in (24, 16) for g in (0, 1)]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library"
    out = str(tmp_path_factory.mktemp("window") / "window.o")
    r = subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-c", os.path.join("csrc", "window.hip"), "-o", out,
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
    assert len(resources) == len(KERNELS), sorted(resources)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if kernel in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k


@pytest.mark.parametrize("kernel", KERNELS)
def test_vgprs_and_agprs_fit_one_wavefront(resources, kernel):
    """VGPRs and AGPRs share one file of 512 per SIMD on gfx950: values the allocator moves to AGPRs are not reported as spills"""
    k = resources[[n for n in resources if kernel in n][0]]
    assert int(k["VGPRs"]) + int(k["AGPRs"]) <= 512 and int(k["Occupancy [waves/SIMD]"]) >= 1, k
