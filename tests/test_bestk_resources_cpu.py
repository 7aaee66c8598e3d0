"""Resources of the windowed sweeps' tile kernel (csrc/bestk.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS:
no scratch and no spills in any instantiation: (five radii of the absolute difference + four of ZNCC) times the
four list sizes KMAX = 0 (MVS_KEEP_ALL), 2, 4, 8, here on the plane table (BAND = false); tests/test_band_bestk_resources_cpu.py has
the other half of the file's 72 kernels.  `keep` and the two outputs are kernel arguments."""
import os
import shutil
import subprocess

import pytest

from test_rect_resources_cpu import HIPCC, PKG, _makefile_flags

ABSDIFF, ZNCC = 0, 1
INSTANCES = [(cost, r, kmax) for cost, radii in ((ABSDIFF, (0, 1, 2, 3, 4)), (ZNCC, (1, 2, 3, 4))) for r in radii for kmax in (0, 2, 4, 8)]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library"
    out = str(tmp_path_factory.mktemp("bestk") / "bestk.o")
    r = subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-c", os.path.join("csrc", "bestk.hip"), "-o", out,
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
    assert len(INSTANCES) == 36 and len(resources) == 2 * len(INSTANCES), sorted(resources)   # x BAND


@pytest.mark.parametrize("cost,r,kmax", INSTANCES)
def test_no_scratch_and_no_spills(resources, cost, r, kmax):
    tag = "14sweep_fx_bestkILi%dELi%dELi%dELb0EE" % (cost, r, kmax)
    names = [n for n in resources if tag in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(tag, {key: k[key] for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
