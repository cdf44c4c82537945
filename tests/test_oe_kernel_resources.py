"""The optimal-estimation unit (csrc/mwrt_oe.hip) without a GPU: the compiler's resource remark for every
kernel of mwrt::oe, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::oe kernels in libmwrt.so (the
nested namespace keeps them out of the mwrt::k_* inventory of test_kernel_instantiations.py, so it is carried here); and
the new ABI surface -- declared, exported, bound, and one record layout on both sides."""
import ctypes
import os
import re
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import _native, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# row tiles of 32 observations per instantiation (m <= 32, 64, 96, 128, 160): VGPRs at most, waves per SIMD at least.
# The occupancy in use is one workgroup (one wave per SIMD) per CU from m = 65 on: LDS, not registers, decides it.
BUDGET = {1: (113, 4), 2: (117, 4), 3: (129, 3), 4: (169, 2), 5: (171, 2)}
KERNELS = {f"k_oe_step<{mr}>" for mr in BUDGET}


def resource_usage(tmp_path):
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", build.OE, "-o", str(tmp_path / "oe.o")]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_oe_stepILi(\d+)E", m.group(1))
            name = int(k.group(1)) if k else m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name is not None:
            out.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_oe_kernels_keep_their_register_budget(tmp_path):
    use = resource_usage(tmp_path)
    assert set(use) == set(BUDGET), use                                  # every kernel of the unit is a k_oe_step<MR>
    for mr, (vgprs, waves) in BUDGET.items():
        assert use[mr]["ScratchSize"] == 0, (mr, use[mr])
        assert use[mr]["VGPRs"] <= vgprs and use[mr]["Occupancy"] >= waves, (mr, use[mr])
        assert use[mr]["LDS"] <= 256, (mr, use[mr])                      # static LDS: nothing but the dynamic block's stub


def test_library_holds_exactly_the_oe_kernels(native_lib):
    out = subprocess.run(["nm", "-C", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"mwrt::oe::(?:\(anonymous namespace\)::)?(k_\w+(?:<[^>()]*>)?)\(", line)
        if m:
            found.add(m.group(1))
    assert found == KERNELS, found
    # and nothing of the unit leaks into the inventory the instantiation tests pin
    assert not re.search(r"mwrt::(?:\(anonymous namespace\)::)?k_oe", out)


def test_abi_surface_of_the_step(native_lib):
    header = open(os.path.join(ROOT, "include", "mwrt.h")).read()
    for sym in ("mwrt_oe_step_device", "mwrt_oe_step_size"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    assert native_lib.mwrt_oe_step_size() == ctypes.sizeof(_native.MwrtOeStep) == 152
    assert _native.MwrtOeStep.d_k.offset == 24 and _native.MwrtOeStep.d_status.offset == 112     # the required part: 120 B
    assert re.search(r"#define MWRT_OE_MAX_M (\d+)", header).group(1) == str(_native.OE_MAX_M)
    assert _native.OE_MAX_M >= 140 and native_lib.mwrt_version() == 301
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    assert native_lib.mwrt_oe_step_device(None, 1, 2, 1, None, None) == -1
