"""Resources of the cleaning kernels (csrc/clean.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any kernel of the file."""
import pytest

from kernel_resources import fixture

KERNELS = ["clean_rules_kernelILi24ELb0E", "clean_rules_kernelILi24ELb1E", "clean_rules_kernelILi16ELb0E", "clean_rules_kernelILi16ELb1E",
           "clean_count_kernel", "clean_tile_kernel", "clean_merge_kernel", "clean_roots_kernel", "clean_apply_kernel"]


resources = fixture("clean.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(resources) == len(KERNELS), sorted(resources)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(resources, kernel):
    names = [n for n in resources if kernel in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
