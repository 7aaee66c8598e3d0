"""Resources of the pyramid kernels (csrc/pyramid.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any kernel of the file."""
import pytest

from kernel_resources import fixture

KERNELS = ["pyramid_down_raw", "pyramid_down_quads", "pyramid_prior"]


resources = fixture("pyramid.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(resources) == len(KERNELS), sorted(resources)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if "%d%sE" % (len(kernel), kernel) in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(kernel, {key: k[key] for key in ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
