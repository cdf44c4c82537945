"""The host units of libmwrt.so (csrc/mwrt.hip and csrc/mwrt_retrieval.hip: streams, caches, handles, argument checks,
entry points) hold no kernel: their device side, cross-compiled for gfx950 with the library's flags (no GPU), defines none.
Kernels live in the kernel units and are reached through the launchers that their interface headers declare."""
import os
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_assembly(unit, tmp_path):
    out = tmp_path / "unit.s"
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "--cuda-device-only", "-S", unit, "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out.read_text()


def test_host_unit_defines_no_kernel(tmp_path):
    assert build.SRC in build.HOST_UNITS and len(build.HOST_UNITS) == 2
    for unit in build.HOST_UNITS:
        asm = device_assembly(unit, tmp_path)
        assert "amdgcn" in asm, (unit, asm[:200])     # it is the gfx950 side that was read
        assert ".amdhsa_kernel" not in asm, (unit, [l for l in asm.splitlines() if ".amdhsa_kernel" in l])
