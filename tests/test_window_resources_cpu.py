"""Resources of the window kernels (csrc/window.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any kernel of the file, and no more vector registers of both kinds than a SIMD has for one wavefront (DESIGN.md
section 18)."""
import pytest

from kernel_resources import fixture

# window_kernel<R, CS, GATED>: radius 0 is never gated
KERNELS = ["window_kernelILi0ELi%dELb0E" % cs for cs in (24, 16)] + \
          ["window_kernelILi%dELi%dELb%dE" % (r, cs, g) for r in (1, 2, 3, 4) for cs in (24, 16) for g in (0, 1)]


resources = fixture("window.hip")


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
