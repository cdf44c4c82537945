"""The optimal-estimation unit (csrc/mwrt_oe.hip) without a GPU: the compiler's resource remark for every
kernel of mwrt::oe, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::oe kernels in libmwrt.so (its
row of the table test_kernel_instantiations.py holds the whole library against, checked here by itself); and the new ABI
surface -- declared, exported, bound, and one record layout on both sides."""
import ctypes
import re

from kernel_unit import MWRT_H, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

# row tiles of 32 observations per instantiation (m <= 32, 64, 96, 128, 160): VGPRs at most, waves per SIMD at least.
# The occupancy in use is one workgroup (one wave per SIMD) per CU from m = 65 on: LDS, not registers, decides it.
BUDGET = {1: (113, 4), 2: (117, 4), 3: (129, 3), 4: (169, 2), 5: (171, 2)}
NAMESPACE = "oe"            # the kernels live in mwrt::oe
KERNELS = {f"k_oe_step<{mr}>" for mr in BUDGET}


def test_oe_kernels_keep_their_register_budget():
    use = resource_usage(build.OE)
    assert set(use) == KERNELS, use                                      # every kernel of the unit is a k_oe_step<MR>
    for mr, (vgprs, waves) in BUDGET.items():
        u = use[f"k_oe_step<{mr}>"]
        assert u["ScratchSize"] == 0, (mr, u)
        assert u["VGPRs"] <= vgprs and u["Occupancy"] >= waves, (mr, u)
        assert u["LDS"] <= 256, (mr, u)                                  # static LDS: nothing but the dynamic block's stub


def test_library_holds_exactly_the_oe_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_abi_surface_of_the_step(native_lib):
    header = open(MWRT_H).read()
    for sym in ("mwrt_oe_step_device", "mwrt_oe_step_size"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    assert native_lib.mwrt_oe_step_size() == ctypes.sizeof(_native.MwrtOeStep) == 152
    assert _native.MwrtOeStep.d_k.offset == 24 and _native.MwrtOeStep.d_status.offset == 112     # the required part: 120 B
    assert re.search(r"#define MWRT_OE_MAX_M (\d+)", header).group(1) == str(_native.OE_MAX_M)
    assert _native.OE_MAX_M >= 140 and native_lib.mwrt_version() == 301
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    assert native_lib.mwrt_oe_step_device(None, 1, 2, 1, None, None) == -1
