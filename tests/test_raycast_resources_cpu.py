"""Resources of the ray-cast kernels (csrc/raycast.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch,
no spills, and few enough registers that the 32 KiB brick mask in LDS, not the register file, bounds the ray kernel's
occupancy (5 workgroups of 4 wavefronts per CU need <= 96 VGPRs)."""
import pytest

from kernel_resources import fixture


resources = fixture("raycast.hip")


@pytest.mark.parametrize("kernel", ["tsdf_raycast_kernelILb0E", "tsdf_raycast_kernelILb1E", "tsdf_brick_kernel"])
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if kernel in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) <= 96 and int(k["AGPRs"]) == 0, k
