"""The register budget of the device K-matrix kernels, from the compiler's own resource remark (cross-compiled for
gfx950 by the library's own command, no GPU): k_jac_rte carries the cloud path as a runtime branch, and its clear-sky speed
rests on 0 bytes of scratch and five waves per SIMD (scheduling fences keep the cloud code's register peak
under the clear loop's)."""
from kernel_unit import resource_usage
from mwr_fast_forward_operators_and_lbls_amd import build


def test_k_matrix_kernels_keep_their_register_budget():
    use = resource_usage(build.TL)
    assert set(use) == {"k_jac_rte", "k_absorb_tl"}, use
    assert use["k_jac_rte"]["ScratchSize"] == 0 and use["k_absorb_tl"]["ScratchSize"] == 0, use
    assert use["k_jac_rte"]["VGPRs"] <= 96 and use["k_jac_rte"]["Occupancy"] >= 5, use      # as before the cloud path
    assert use["k_absorb_tl"]["Occupancy"] >= 2, use
