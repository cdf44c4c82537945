"""The reduced-basis unit (csrc/mwrt_basis.hip) without a GPU: the compiler's resource remark for its kernels,
cross-compiled for gfx950 with the library's flags; the inventory of mwrt::basis kernels in libmwrt.so; the new ABI surface --
declared, exported, bound, and the record laid out alike on both sides; and the guard of the GPU tests' shape list against
the tile constants of the plan header as the code has them."""
import ctypes
import os
import re

import basis_reference as bar
from kernel_unit import MWRT_H, check_record, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

NAMESPACE = "basis"            # the kernels live in mwrt::basis
KERNELS = {"k_project", "k_expand"}
SYMBOLS = ("mwrt_basis_create", "mwrt_basis_destroy", "mwrt_basis_project_device", "mwrt_basis_expand_device",
           "mwrt_basis_apply_size")
HEADER = os.path.join(os.path.dirname(build.BASIS), "mwrt_basis.hip.h")


def plan():
    """The tile constants of csrc/mwrt_basis.hip.h, by name."""
    text = open(HEADER).read()
    out = {}
    for name in ("THREADS", "ROWS", "COLS", "KCHUNK", "MR", "NC"):
        out[name] = int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    return out


def test_basis_kernels_keep_their_budgets():
    use = resource_usage(build.BASIS)
    assert set(use) == KERNELS, use                                      # the unit holds these kernels and no other
    t = plan()
    u = use["k_project"]
    assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, u                  # plain fp64 FMAs: no MFMA accumulators, no spill
    # Ks [KCHUNK][ROWS + 1] and Bs [KCHUNK][COLS] doubles: seven workgroups of it fit a CU's 160 KiB
    assert u["LDS"] == 8 * t["KCHUNK"] * (t["ROWS"] + 1 + t["COLS"]) == 20608, u
    # a 4 x 4 tile of doubles, a chunk in flight (8 + 2 doubles) and the operands: four waves per SIMD = four workgroups per CU
    assert u["VGPRs"] <= 128 and u["Occupancy"] >= 4, u
    e = use["k_expand"]
    assert e["ScratchSize"] == 0 and e["AGPRs"] == 0 and e["LDS"] == 0 and e["VGPRs"] <= 32 and e["Occupancy"] == 8, e


def test_library_holds_exactly_the_basis_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_host_unit_carries_no_basis_device_code():
    hosts = {unit: open(unit).read() for unit in build.HOST_UNITS}
    assert '#include "mwrt_basis.hip.h"' in hosts[build.RETRIEVAL]
    assert all("__global__" not in text and "mwrt_oe_blocks.hip.h" not in text for text in hosts.values())
    assert "__global__" not in open(HEADER).read()
    assert (build.BASIS, []) in build.UNITS


def test_abi_surface_of_the_reduced_basis(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtBasisApply
    check_record(native_lib, "mwrt_basis_apply", rec, 80, offsets=[0, 4, 8, 40, 48, 56, 64, 72, 76],
                 names=["struct_size", "reserved", "d_k_in", "d_k_out", "d_c", "d_x_ref", "d_x", "x_ref_per_profile", "reserved2"])
    kinds = {f[0]: f[1] for f in rec._fields_}
    assert kinds["struct_size"] is ctypes.c_uint32 and kinds["reserved"] is ctypes.c_int32
    assert kinds["x_ref_per_profile"] is ctypes.c_int32 and kinds["reserved2"] is ctypes.c_int32
    assert ctypes.sizeof(kinds["d_k_in"]) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert all(kinds[k] is ctypes.c_void_p for k in ("d_k_out", "d_c", "d_x_ref", "d_x"))
    assert native_lib.mwrt_version() == 301 == _native.MWRT_VERSION


def test_null_arguments_are_refused_without_a_gpu(native_lib):
    r = _native.MwrtBasisApply()
    r.struct_size = ctypes.sizeof(r)
    fake = ctypes.c_void_p(8)                                            # never dereferenced: the NULL beside it is seen first
    for call in (lambda *a: native_lib.mwrt_basis_project_device(a[0], a[1], 1, 2, a[2], None),
                 lambda *a: native_lib.mwrt_basis_expand_device(a[0], a[1], 1, a[2], None)):
        assert call(None, None, None) == -1
        assert call(None, None, ctypes.byref(r)) == -1
        assert call(None, fake, ctypes.byref(r)) == -1
        assert b"null" in native_lib.mwrt_last_error()
    h = ctypes.c_void_p(1)
    b = (ctypes.c_double * 2)(1.0, 2.0)
    assert native_lib.mwrt_basis_create(None, 1, 2, 1, b, ctypes.byref(h)) == -1 and h.value is None
    assert native_lib.mwrt_basis_create(None, 1, 2, 1, b, None) == -1
    assert native_lib.mwrt_basis_destroy(None) == 0


def test_the_shapes_straddle_every_tile_edge():
    """tests/basis_reference.py SHAPES against the plan header: the list the GPU tests run has to keep both sides of every
    tile edge of k_project as built, and the values the kernel was asked to be tested at."""
    t = plan()
    assert (t["THREADS"] // 8) * t["MR"] == t["ROWS"] and 8 * t["NC"] == t["COLS"]
    rows = {s[0] * s[1] for s in bar.SHAPES}
    cols = {s[4] for s in bar.SHAPES}
    n = {s[2] * s[3] for s in bar.SHAPES}
    R, C, K = t["ROWS"], t["COLS"], t["KCHUNK"]
    assert {1, R - 1, R, R + 1} <= rows and max(rows) > 2 * R                    # one short, exact, one over; three tiles
    assert any(s[0] > 1 and (s[0] * s[1]) % R != 0 and s[0] * s[1] > R for s in bar.SHAPES)   # nprof m no multiple
    assert {1, C - 1, C, C + 1, 2 * C, 2 * C + 1} <= cols                        # ... and a last column tile of width 1
    assert {1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1} <= n
    assert any(s[3] > 1 and s[2] % K != 0 for s in bar.SHAPES)                   # a chunk that spans two K blocks
    assert any(s[0] * s[1] > R and s[4] > C for s in bar.SHAPES)                 # both grid dimensions beyond one tile
    # what the kernel is to be tested at, whatever its tiles
    assert {1, 3} <= {s[0] for s in bar.SHAPES} and {1, 14, 98, 140} <= {s[1] for s in bar.SHAPES}
    assert {1, 15, 16, 17, 180} <= {s[2] for s in bar.SHAPES} and {1, 2, 4} <= {s[3] for s in bar.SHAPES}
    assert {1, 31, 32, 33, 65} <= cols
    assert len(set(bar.SHAPES)) == len(bar.SHAPES)
