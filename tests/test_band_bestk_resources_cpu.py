"""Resources of the windowed band sweep's kernel (the BAND = true half of csrc/bestk.hip) from the compiler's report for gfx950 with the
Makefile's own CXXFLAGS: 36 instantiations, as on the plane table -- (five radii of the absolute difference + four of ZNCC) times the
four list sizes KMAX = 0 (MVS_KEEP_ALL), 2, 4, 8 -- none with scratch or spills.  Registers, occupancy and LDS are
printed: the per-sample plane costs NS x 2 vector registers over the table's instantiation."""
import os

import pytest

from kernel_resources import PKG, fixture

ABSDIFF, ZNCC = 0, 1
INSTANCES = [(cost, r, kmax) for cost, radii in ((ABSDIFF, (0, 1, 2, 3, 4)), (ZNCC, (1, 2, 3, 4))) for r in radii for kmax in (0, 2, 4, 8)]


resources = fixture("bestk.hip")


def test_every_kernel_of_the_file_is_listed(resources):
    assert len(INSTANCES) == 36 and sum("Lb1EE" in n for n in resources) == len(INSTANCES), sorted(resources)
    assert not os.path.exists(os.path.join(PKG, "csrc", "band_bestk.hip"))   # one tile kernel: no second copy of the body


@pytest.mark.parametrize("cost,r,kmax", INSTANCES)
def test_no_scratch_and_no_spills(resources, cost, r, kmax):
    tag = "14sweep_fx_bestkILi%dELi%dELi%dELb1EE" % (cost, r, kmax)
    names = [n for n in resources if tag in n]
    assert len(names) == 1, sorted(resources)
    k = resources[names[0]]
    print(tag, {key: k[key] for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]") if key in k})
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
