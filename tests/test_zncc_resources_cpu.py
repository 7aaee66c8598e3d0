"""Resources of the ZNCC sweep's kernel (csrc/zncc.hip) from the compiler's report for gfx950 with the Makefile's own CXXFLAGS: no scratch
and no spills in any instantiation: four radii times three combinations of outputs."""
import pytest

from kernel_resources import fixture

INSTANCES = [(r, vol, fused) for r in (1, 2, 3, 4) for vol, fused in ((1, 1), (1, 0), (0, 1))]


resources = fixture("zncc.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(resources) == len(INSTANCES), sorted(resources)


@pytest.mark.parametrize("r,vol,fused", INSTANCES)
def test_no_scratch_and_no_spills(resources, r, vol, fused):
    tag = "13sweep_fx_znccILi%dELb%dELb%dEE" % (r, vol, fused)
    names = [n for n in resources if tag in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(tag, {key: k[key] for key in ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
