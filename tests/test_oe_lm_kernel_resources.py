"""The Levenberg-Marquardt unit (csrc/mwrt_oe_lm.hip) without a GPU: the compiler's resource remark for every
kernel of mwrt::lm, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::lm kernels in libmwrt.so;
and the new ABI surface -- declared, exported, bound, and one record layout on both sides."""
import ctypes
import re

from kernel_unit import MWRT_H, check_record, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build
from test_oe_kernel_resources import BUDGET

NAMESPACE = "lm"            # the kernels live in mwrt::lm
# k_lm_prepare<MR> is the first three steps of k_oe_step<MR>: it is held to that kernel's VGPR and occupancy budget
KERNELS = {f"k_lm_prepare<{mr}>" for mr in BUDGET} | {"k_lm_solve", "k_lm_cost"}


def test_lm_kernels_keep_their_register_budget():
    use = resource_usage(build.OE_LM)
    assert set(use) == KERNELS, use                                      # every kernel of the unit is one of the three
    for name, u in use.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] <= 256, (name, u)                                # static LDS: nothing but the dynamic block's stub
    for mr, (vgprs, waves) in BUDGET.items():
        u = use[f"k_lm_prepare<{mr}>"]
        assert u["VGPRs"] <= vgprs and u["Occupancy"] >= waves, (mr, u)
    # the solve is meant to have more than one workgroup (4 waves) per CU resident at m ~ 98: registers must allow it
    assert use["k_lm_solve"]["Occupancy"] >= 3 and use["k_lm_cost"]["Occupancy"] >= 3, use


def test_library_holds_exactly_the_lm_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_abi_surface_of_the_split(native_lib):
    header = open(MWRT_H).read()
    for sym in ("mwrt_oe_lm_prepare_device", "mwrt_oe_lm_solve_device", "mwrt_oe_cost_device", "mwrt_oe_lm_size"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeLm
    check_record(native_lib, "mwrt_oe_lm", rec, 224)
    assert rec.d_k.offset == 24 and rec.d_x.offset == 56 and rec.d_nobs.offset == 216
    assert native_lib.mwrt_version() == 301
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    for sym in ("mwrt_oe_lm_prepare_device", "mwrt_oe_lm_solve_device", "mwrt_oe_cost_device"):
        assert getattr(native_lib, sym)(None, 1, 2, 1, None, None) == -1
        assert getattr(native_lib, sym)(None, 1, 2, 1, ctypes.byref(rec()), None) == -1
