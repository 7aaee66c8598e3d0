"""Register allocation of the rectified-view sweep kernel (csrc/sweep_rect.hip), from the compiler's resource report for gfx950 with the
Makefile's own CXXFLAGS.  The headline instantiation sweep_fx_rect<RS, true, true> (volume + fused depth selection) must keep 5 wavefronts
per SIMD (<= 96 VGPRs).  The spills are bounded at what the clean region body left them: not the aim -- that is
none -- but a ratchet, so that an edit cannot make them worse unnoticed.  Before that body the headline instantiation spilled 21 SGPRs
(now 28, 29 at RS 64) and the volume-only one 28 (now 52, 58 at RS 64); the spill code sits in the chunk epilogue and the
failed-certificate block, not on the clean path."""
import pytest

from kernel_resources import fixture

RS_ALL = (64, 84, 96, 128)

# per instantiation (WRITE_VOLUME, FUSED): at most this many VGPRs, at least this many waves per SIMD, at most this much scratch
# (bytes per lane), VGPR spills and SGPR spills, at every compiled row stride
BOUNDS = {
    (True, True): dict(vgprs=96, waves=5, scratch=8, vgpr_spill=3, sgpr_spill=29),
    (True, False): dict(vgprs=72, waves=7, scratch=0, vgpr_spill=0, sgpr_spill=58),
    (False, True): dict(vgprs=96, waves=5, scratch=8, vgpr_spill=2, sgpr_spill=16),
}


resources = fixture("sweep_rect.hip")


@pytest.mark.parametrize("inst", sorted(BOUNDS), ids=lambda i: "vol%d_fused%d" % i)
@pytest.mark.parametrize("rs", RS_ALL)
def test_rect_kernel_allocation(resources, rs, inst):
    name = "_ZN3mvs13sweep_fx_rectILi%dELb%dELb%dEEEvNS_8RectArgsE" % (rs, inst[0], inst[1])
    assert name in resources, sorted(resources)
    k, b = resources[name], BOUNDS[inst]
    assert int(k["VGPRs"]) <= b["vgprs"], k
    assert int(k["AGPRs"]) == 0, k
    assert int(k["Occupancy [waves/SIMD]"]) >= b["waves"], k
    assert int(k["ScratchSize [bytes/lane]"]) <= b["scratch"], k
    assert int(k["VGPRs Spill"]) <= b["vgpr_spill"], k
    assert int(k["SGPRs Spill"]) <= b["sgpr_spill"], k
