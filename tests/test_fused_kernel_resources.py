"""The register budget of the headline fused kernel, from the compiler's own resource remark (cross-compiled for gfx950,
no GPU): the TB-only 256-thread instantiation of the 14-wide chunk, k_tb_fused<14, 8, 256, false, false, false>, is bound by
fp64 VALU issue at THREE waves per SIMD.  One register past 168 halves nothing but costs the third wave, and
scratch in the layer loops costs issue slots: both have undone earlier changes to this kernel, so they are held here."""
import os
import re
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "k_tb_fusedILi14ELi8ELi256ELb0ELb0ELb0EE"          # <NFC 14, NFK 8, MAXT 256, OPT, EXTRAS, ALPHA all false>


def resource_usage(tmp_path):
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-DMWRT_INST_NFC=14", "-Rpass-analysis=kernel-resource-usage", "-c", build.INST, "-o", str(tmp_path / "inst14.o")]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_headline_fused_kernel_keeps_its_register_budget(tmp_path):
    use = resource_usage(tmp_path)
    mine = [v for k, v in use.items() if HEADLINE in k]
    assert len(mine) == 1, sorted(use)
    u = mine[0]
    assert u["VGPRs"] <= 168 and u["Occupancy"] >= 3 and u["ScratchSize"] <= 20, u
