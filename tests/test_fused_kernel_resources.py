"""The register budget of the headline fused kernel, from the compiler's own resource remark (cross-compiled for gfx950 by
the library's own command, no GPU): the TB-only 256-thread instantiation of the 14-wide chunk,
k_tb_fused<14, 8, 256, false, false, false>, is bound by fp64 VALU issue at THREE waves per SIMD.  One register
past 168 halves nothing but costs the third wave, and scratch in the layer loops costs issue slots: both have undone earlier
changes to this kernel, so they are held here."""
from kernel_unit import resource_usage
from mwr_fast_forward_operators_and_lbls_amd import build

HEADLINE = "k_tb_fused<14, 8, 256, false, false, false>"      # <NFC 14, NFK 8, MAXT 256, OPT, EXTRAS, ALPHA all false>


def test_headline_fused_kernel_keeps_its_register_budget():
    use = resource_usage(build.INST, ("-DMWRT_INST_NFC=14",))
    assert HEADLINE in use, sorted(use)
    u = use[HEADLINE]
    assert u["VGPRs"] <= 168 and u["Occupancy"] >= 3 and u["ScratchSize"] <= 20, u
