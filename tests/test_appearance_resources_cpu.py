"""Resources of the appearance kernels (csrc/tsdf.hip, csrc/appearance.hip) from the compiler's report for gfx950 with the Makefile's own
CXXFLAGS: no scratch, no spills and at most 96 VGPRs, and the kernels of mvs_tsdf_integrate, whose bodies the new
ones share, keep the figures of DESIGN.md section 12's table."""
import pytest

from kernel_resources import fixture


resources = fixture("tsdf.hip", "appearance.hip")


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
