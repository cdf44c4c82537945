"""The characterisation unit (csrc/mwrt_oe_char.hip) without a GPU: the compiler's resource remark for every
kernel of mwrt::oec, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::oec kernels in libmwrt.so;
and the new ABI surface -- declared, exported, bound, and one record layout on both sides."""
import ctypes
import os
import re

from kernel_unit import MWRT_H, check_record, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build
from test_oe_kernel_resources import BUDGET

NAMESPACE = "oec"            # the kernels live in mwrt::oec
# k_char_gain<MR> is steps 1-4 and 7 of k_oe_step<MR> with one more triangular product: it is held to that kernel's VGPR
# and occupancy budget
KERNELS = {f"k_char_gain<{mr}>" for mr in BUDGET} | {"k_char_product"}


def test_char_kernels_keep_their_register_budget():
    use = resource_usage(build.OE_CHAR)
    assert set(use) == KERNELS, use                                      # every kernel of the unit is one of the two
    for name, u in use.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["AGPRs"] == 0, (name, u)                                # the register cap spills nowhere, AGPRs included
        assert u["LDS"] <= 256, (name, u)                                # static LDS: nothing but the dynamic block's stub
    for mr, (vgprs, waves) in BUDGET.items():
        u = use[f"k_char_gain<{mr}>"]
        assert u["VGPRs"] <= vgprs and u["Occupancy"] >= waves, (mr, u)
    # the product keeps two workgroups (8 waves) per CU resident at least: registers must allow it
    assert use["k_char_product"]["Occupancy"] >= 2, use


def test_lds_plan_fits_and_is_aligned():
    """The plan of csrc/mwrt_oe_char.hip.h, restated: <= 160 KB at the m limit whatever n is, every carve offset 16-byte
    aligned (even in doubles)."""
    text = open(os.path.join(os.path.dirname(build.OE_CHAR), "mwrt_oe_char.hip.h")).read()
    assert "p.total_bytes = sizeof(double) * (p.keep + (size_t)p.mp / 2);" in text      # the rule restated below
    for m in (1, 31, 32, 33, 64, 65, 98, 139, 140):
        mp = (m + 31) // 32 * 32
        kpitch = mp + 1
        wt = (m * (m + 1) // 2 + 1) & ~1
        ks = wt + ((32 * kpitch + 1) & ~1)
        ss = ks + 16 * kpitch
        part = (ss + 16 * 32 + 1) & ~1
        sed = part + 2 * 8 * 32
        red = sed + mp
        keep = red + 256
        total = 8 * (keep + mp // 2)
        assert all(o % 2 == 0 for o in (wt, ks, ss, part, sed, red, keep)), m
        assert ss - ks + 16 * 32 >= 32 * 32                              # Ks | Ss hold the [32][32] column sums
        assert total <= 160 * 1000, (m, total)


def test_library_holds_exactly_the_char_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_abi_surface_of_the_characterisation(native_lib):
    header = open(MWRT_H).read()
    for sym in ("mwrt_oe_gain_device", "mwrt_oe_product_device", "mwrt_oe_char_size"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeChar
    names = check_record(native_lib, "mwrt_oe_char", rec, 200)
    kinds = {f[0]: f[1] for f in rec._fields_}
    assert all(kinds[k] is ctypes.c_int32 for k in ("product", "row_begin", "row_count", "reserved2", "nblk", "reserved"))
    assert all(kinds[k] is ctypes.c_void_p for k in names if k.startswith("d_") and k != "d_k")
    assert rec.d_k.offset == 24 and rec.d_x.offset == 56 and rec.d_status.offset == 104 and rec.d_nobs.offset == 168
    assert rec.product.offset == 176 and rec.reserved2.offset == 188 and rec.d_out.offset == 192
    assert re.search(r"#define MWRT_OE_PRODUCT_AVK\s+(\d+)", header).group(1) == str(_native.OE_PRODUCT_AVK)
    assert re.search(r"#define MWRT_OE_PRODUCT_POST_COV\s+(\d+)", header).group(1) == str(_native.OE_PRODUCT_POST_COV)
    assert native_lib.mwrt_version() == 301
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    for sym in ("mwrt_oe_gain_device", "mwrt_oe_product_device"):
        assert getattr(native_lib, sym)(None, 1, 2, 1, None, None) == -1
        assert getattr(native_lib, sym)(None, 1, 2, 1, ctypes.byref(rec()), None) == -1
