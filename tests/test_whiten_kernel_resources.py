"""The pre-whitening unit (csrc/mwrt_whiten.hip) without a GPU: the compiler's resource remark for its kernels,
cross-compiled for gfx950 with the library's flags; the inventory of mwrt::wh kernels in libmwrt.so; the new ABI surface --
declared, exported, bound, and the record laid out alike on both sides; and the guard of the GPU tests' shape list against
the plan constants of the header as the code has them."""
import ctypes
import os
import re

import whiten_reference as whr
from kernel_unit import MWRT_H, check_record, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

NAMESPACE = "wh"            # the kernels live in mwrt::wh
KERNELS = {"k_wh_factor", "k_wh_apply"}
SYMBOLS = ("mwrt_obs_whiten_device", "mwrt_obs_whiten_apply_device", "mwrt_obs_whiten_size")
HEADER = os.path.join(os.path.dirname(build.WHITEN), "mwrt_whiten.hip.h")
LDS_PER_CU = 160 * 1024


def plan():
    """The plan constants of csrc/mwrt_whiten.hip.h, by name."""
    text = open(HEADER).read()
    return {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
            for name in ("FACTOR_THREADS", "COLS", "ROW_BLOCK", "LOAD_BATCH", "KEEP_WORDS")}


def test_whiten_kernels_keep_their_budgets():
    use = resource_usage(build.WHITEN)
    assert set(use) == KERNELS, use                                      # the unit holds these kernels and no other
    t = plan()
    for u in use.values():
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, u              # plain fp64 FMAs: no MFMA accumulators, no spill
        assert u["LDS"] == 0, u                                          # all LDS is dynamic: the plan's functions below
    assert use["k_wh_factor"]["VGPRs"] <= 32 and use["k_wh_factor"]["Occupancy"] == 8, use
    # four accumulators, their divisions, a batch of rows and the next block's rows of L in flight.  The registers leave seven
    # waves per SIMD, far beyond what the LDS of a tile admits
    assert use["k_wh_apply"]["VGPRs"] <= 72 and use["k_wh_apply"]["Occupancy"] >= 7, use
    # the dynamic LDS of the plan: a tile of vt [m][COLS] doubles and one row block's rows of L per one-wave workgroup -- three of them per CU at the
    # workload's m = 98, two at the limit; the packed triangle and the row flags of the factorisation -- two per CU at the limit
    apply_lds = lambda m: 8 * (m * t["COLS"] + t["ROW_BLOCK"] * m + t["ROW_BLOCK"] * (t["ROW_BLOCK"] + 1) // 2)   # noqa: E731
    factor_lds = lambda m: 8 * (((m * (m + 1) // 2 + 1) & ~1) + (m + 1) // 2)   # noqa: E731
    text = open(HEADER).read()
    assert "(size_t)m * COLS + (size_t)ROW_BLOCK * m + ROW_BLOCK * (ROW_BLOCK + 1) / 2" in text and "((size_t)m * (m + 1) / 2 + 1) & ~(size_t)1) + ((size_t)m + 1) / 2" in text
    assert apply_lds(98) == 53392 and LDS_PER_CU // apply_lds(98) == 3 and LDS_PER_CU // apply_lds(140) == 2
    assert factor_lds(140) == 79520 and LDS_PER_CU // factor_lds(140) == 2
    # where each passes the default limit of 64 KiB, the seams the shape list straddles
    assert apply_lds(120) <= 65536 < apply_lds(121) and factor_lds(127) <= 65536 < factor_lds(128)


def test_library_holds_exactly_the_whiten_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_host_unit_carries_no_whiten_device_code():
    hosts = {unit: open(unit).read() for unit in build.HOST_UNITS}
    assert '#include "mwrt_whiten.hip.h"' in hosts[build.RETRIEVAL]
    assert all("__global__" not in text and "mwrt_oe_blocks.hip.h" not in text for text in hosts.values())
    assert "__global__" not in open(HEADER).read()
    assert (build.WHITEN, []) in build.UNITS


def test_abi_surface_of_the_pre_whitening(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtObsWhiten
    check_record(native_lib, "mwrt_obs_whiten", rec, 152, offsets=[0, 4, 8, 12, 16, 24, 32, 40, 48, 80, 88, 96, 104, 112, 120],
                 names=["struct_size", "nblk", "se_full", "mode", "reserved", "d_se", "d_y", "d_fx", "d_k_in", "d_l", "d_keep",
                        "d_status", "d_y_out", "d_fx_out", "d_k_out"])
    kinds = {f[0]: f[1] for f in rec._fields_}
    assert kinds["struct_size"] is ctypes.c_uint32 and kinds["reserved"] is ctypes.c_int64
    assert all(kinds[k] is ctypes.c_int32 for k in ("nblk", "se_full", "mode"))
    assert all(ctypes.sizeof(kinds[k]) == 4 * ctypes.sizeof(ctypes.c_void_p) for k in ("d_k_in", "d_k_out"))
    assert all(kinds[k] is ctypes.c_void_p for k in ("d_se", "d_y", "d_fx", "d_l", "d_keep", "d_status", "d_y_out", "d_fx_out"))
    assert native_lib.mwrt_version() == 301 == _native.MWRT_VERSION
    assert (_native.WHITEN_FORWARD, _native.WHITEN_TRANSPOSED) == (0, 1)


def test_null_arguments_are_refused_without_a_gpu(native_lib):
    r = _native.MwrtObsWhiten()
    r.struct_size = ctypes.sizeof(r)
    for entry in (native_lib.mwrt_obs_whiten_device, native_lib.mwrt_obs_whiten_apply_device):
        assert entry(None, 1, 2, 3, None, None) == -1
        assert entry(None, 1, 2, 3, ctypes.byref(r), None) == -1
        assert b"null" in native_lib.mwrt_last_error()


def test_the_shapes_straddle_every_seam():
    """tests/whiten_reference.py SHAPES against the plan header: the list the GPU tests run has to keep both sides of every
    seam of the two kernels as built, and the values the kernels were asked to be tested at."""
    t = plan()
    ms = {s[2] for s in whr.SHAPES}
    levs = {s[0] for s in whr.SHAPES if s[1] > 0}
    B, C = t["ROW_BLOCK"], t["COLS"]
    assert {B - 1, B, B + 1} <= ms and {r for r in range(B)} <= {m % B for m in ms}       # the row block and every remainder
    G = t["LOAD_BATCH"]
    assert {G - 1, G, G + 1} <= ms and any(m > G and m % G == 0 for m in ms) and any(m > G and m % G for m in ms)   # the load batch
    assert C == 64 and t["KEEP_WORDS"] * 64 >= 140
    for w in range(1, t["KEEP_WORDS"]):                                  # the words of the row flags, the wave of the row rule
        assert {64 * w - 1, 64 * w, 64 * w + 1} <= ms, w
    assert {C - 1, C, C + 1} <= levs and any(l > 2 * C for l in levs)     # the column tile: one short, exact, one over; three
    assert {120, 121, 127, 128, 129} <= ms                               # both kernels' first raise of the LDS limit
    # what the kernels are to be tested at, whatever their plan
    assert {1, 32, 33, 64, 65, 140} <= ms and {1, 2, 63, 64, 65, 180} <= levs
    assert {0, 1, 2, 3, 4} <= {s[1] for s in whr.SHAPES}
    assert {whr.nprof_of(s) for s in whr.SHAPES} <= {3, 4}
    assert len(set(whr.SHAPES)) == len(whr.SHAPES)
    # the dropped-row patterns sit on the seams of their shape
    m = whr.SEAM_SHAPE[2]
    d = whr.SEAM_DROPS
    assert m == 65 and d["first"] == (0,) and d["last"] == (m - 1,) and d["row-3"] == (B - 1,) and d["row-4"] == (B,)
    assert d["row-63"] == (63,) and d["block-4-7"] == tuple(range(B, 2 * B)) and len(d["all-but-64"]) == m - 1 and len(d["all"]) == m
