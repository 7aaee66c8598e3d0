"""Resources of the windowed sweeps' tile kernel (csrc/bestk.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS:
no scratch and no spills in any instantiation: (five radii of the absolute difference + four of ZNCC) times the
four list sizes KMAX = 0 (MVS_KEEP_ALL), 2, 4, 8, here on the plane table (BAND = false); tests/test_band_bestk_resources_cpu.py has
the other half of the file's 72 kernels.  `keep` and the two outputs are kernel arguments."""
import pytest

from kernel_resources import fixture

ABSDIFF, ZNCC = 0, 1
INSTANCES = [(cost, r, kmax) for cost, radii in ((ABSDIFF, (0, 1, 2, 3, 4)), (ZNCC, (1, 2, 3, 4))) for r in radii for kmax in (0, 2, 4, 8)]


resources = fixture("bestk.hip")


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
