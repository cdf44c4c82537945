"""The register budget of the cloud / ray-tracing TB-only instantiation of the 14-wide chunk,
k_tb_fused<14, 8, 256, true, false, false>, from the compiler's resource remark (cross-compiled for gfx950, no GPU).  It
sits at the edge of its third wave (167 of 168 VGPRs): the far-line groups of K1 may not cost it that wave, nor more scratch
than it had before them -- 64 B per lane in the commit before the groups, read from that commit's build.

The groups alone took it to 96 B.  Two changes to the OPT code brought it back under: z, T, p and the ozone column are
read again after the line loops instead of riding through them (72 B), and cloud_level builds its record from scalars, which
frees the 16-byte stack slot the zero-initialised struct had left behind (52 B)."""
from kernel_unit import resource_usage
from mwr_fast_forward_operators_and_lbls_amd import build

OPT_HEADLINE = "k_tb_fused<14, 8, 256, true, false, false>"   # <NFC 14, NFK 8, MAXT 256, OPT, no EXTRAS, no ALPHA>
PARENT_SCRATCH = 64                                            # bytes per lane, the commit before the far-line groups


def test_opt_fused_kernel_keeps_its_third_wave_and_its_scratch():
    use = resource_usage(build.INST, ("-DMWRT_INST_NFC=14",))     # the compile test_fused_kernel_resources.py asks for
    assert OPT_HEADLINE in use, sorted(use)
    u = use[OPT_HEADLINE]
    print(u)
    assert u["Occupancy"] >= 3, u
    assert u["ScratchSize"] <= PARENT_SCRATCH, u
