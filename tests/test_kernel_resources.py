"""The register budget of the device K-matrix kernels, from the compiler's own resource remark (cross-compiled for
gfx950, no GPU): k_jac_rte carries the cloud path as a runtime branch, and its clear-sky speed rests on 0 bytes of scratch
and five waves per SIMD (scheduling fences keep the cloud code's register peak under the clear loop's)."""
import os
import re
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resource_usage(tmp_path):
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", build.TL, "-o", str(tmp_path / "tl.o")]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = "k_jac_rte" if "k_jac_rte" in m.group(1) else ("k_absorb_tl" if "k_absorb_tl" in m.group(1) else None)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_k_matrix_kernels_keep_their_register_budget(tmp_path):
    use = resource_usage(tmp_path)
    assert set(use) == {"k_jac_rte", "k_absorb_tl"}, use
    assert use["k_jac_rte"]["ScratchSize"] == 0 and use["k_absorb_tl"]["ScratchSize"] == 0, use
    assert use["k_jac_rte"]["VGPRs"] <= 96 and use["k_jac_rte"]["Occupancy"] >= 5, use      # as before the cloud path
    assert use["k_absorb_tl"]["Occupancy"] >= 2, use
