"""The instrument-operator unit (csrc/mwrt_obs.hip) without a GPU: the compiler's resource remark for its kernel,
cross-compiled for gfx950 with the library's flags; the inventory of mwrt::obs kernels in libmwrt.so; and the new ABI surface
-- declared, exported, bound, and the record laid out alike on both sides."""
import ctypes
import os
import re

from kernel_unit import MWRT_H, check_record, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

NAMESPACE = "obs"            # the kernels live in mwrt::obs
KERNELS = {"k_obs_apply"}
SYMBOLS = ("mwrt_obs_create", "mwrt_obs_destroy", "mwrt_obs_apply_device", "mwrt_obs_apply_size")


def test_obs_kernel_streams_from_registers_alone():
    use = resource_usage(build.OBS)
    assert set(use) == KERNELS, use                                      # the unit holds this kernel and no other
    u = use["k_obs_apply"]
    assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, u
    assert u["LDS"] <= 256, u                                            # no LDS: nothing is shared between lanes
    # eight row loads in flight per lane and full occupancy: latency is hidden by both
    assert u["VGPRs"] <= 64 and u["Occupancy"] == 8, u


def test_library_holds_exactly_the_obs_kernel(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_host_unit_carries_no_obs_device_code():
    hosts = {unit: open(unit).read() for unit in build.HOST_UNITS}
    assert '#include "mwrt_obs.hip.h"' in hosts[build.RETRIEVAL]
    assert all("__global__" not in text and "mwrt_oe_blocks.hip.h" not in text for text in hosts.values())
    head = open(os.path.join(os.path.dirname(build.OBS), "mwrt_obs.hip.h")).read()
    assert "__global__" not in head
    assert (build.OBS, []) in build.UNITS


def test_abi_surface_of_the_instrument_operator(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtObsApply
    check_record(native_lib, "mwrt_obs_apply", rec, 96,
                 names=["struct_size", "nblk", "reserved", "d_tb_in", "d_tb_out", "d_k_in", "d_k_out"])
    kinds = {f[0]: f[1] for f in rec._fields_}
    assert kinds["struct_size"] is ctypes.c_uint32 and kinds["nblk"] is ctypes.c_int32 and kinds["reserved"] is ctypes.c_int32
    assert kinds["d_tb_in"] is ctypes.c_void_p and kinds["d_tb_out"] is ctypes.c_void_p
    assert ctypes.sizeof(kinds["d_k_in"]) == ctypes.sizeof(kinds["d_k_out"]) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert rec.struct_size.offset == 0 and rec.nblk.offset == 4 and rec.reserved.offset == 8
    assert rec.d_tb_in.offset == 16 and rec.d_tb_out.offset == 24 and rec.d_k_in.offset == 32 and rec.d_k_out.offset == 64
    assert re.search(r"#define MWRT_MAX_ANGLES (\d+)", header).group(1) == str(_native.MAX_ANGLES)
    assert native_lib.mwrt_version() == 301 == _native.MWRT_VERSION


def test_null_arguments_are_refused_without_a_gpu(native_lib):
    r = _native.MwrtObsApply()
    r.struct_size = ctypes.sizeof(r)
    fake = ctypes.c_void_p(8)                                            # never dereferenced: the NULL beside it is seen first
    assert native_lib.mwrt_obs_apply_device(None, None, 1, 2, None, None) == -1
    assert native_lib.mwrt_obs_apply_device(None, None, 1, 2, ctypes.byref(r), None) == -1
    assert native_lib.mwrt_obs_apply_device(None, fake, 1, 2, ctypes.byref(r), None) == -1
    assert b"null" in native_lib.mwrt_last_error()
    h = ctypes.c_void_p(1)
    rp = (ctypes.c_int32 * 2)(0, 1)
    col = (ctypes.c_int32 * 1)(0)
    w = (ctypes.c_double * 1)(1.0)
    assert native_lib.mwrt_obs_create(None, 1, 1, rp, col, w, ctypes.byref(h)) == -1 and h.value is None
    assert native_lib.mwrt_obs_create(None, 1, 1, rp, col, w, None) == -1
    assert native_lib.mwrt_obs_destroy(None) == 0
