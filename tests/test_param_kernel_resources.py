"""The spectroscopic-parameter unit (csrc/mwrt_par.hip) without a GPU: the compiler's resource remark for its
kernels, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::par kernels in libmwrt.so; and the new
ABI surface -- declared, exported, bound, and the record laid out alike on both sides."""
import ctypes
import os
import re

from kernel_unit import MWRT_H, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

NAMESPACE = "par"            # the kernels live in mwrt::par
KERNELS = {"k_par_tangent", "k_par_contract"}
SYMBOLS = ("mwrt_tb_param_jacobian_batch_device", "mwrt_tb_param_jacobian_batch")


def test_parameter_kernels_keep_their_register_budget():
    use = resource_usage(build.PAR)
    assert set(use) == KERNELS, use                                      # the unit holds these kernels and no others
    for u in use.values():
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, use
    # the tangent kernel carries the speed-dependent shape's rational: one wave per workgroup, four waves per SIMD
    assert use["k_par_tangent"]["VGPRs"] <= 128 and use["k_par_tangent"]["Occupancy"] >= 4, use
    assert use["k_par_tangent"]["LDS"] == 0, use
    # the contraction kernel is k_jac_rte's clear-sky loop: the same five waves per SIMD, dynamic LDS only
    assert use["k_par_contract"]["VGPRs"] <= 96 and use["k_par_contract"]["Occupancy"] >= 5, use
    assert use["k_par_contract"]["LDS"] <= 256, use


def test_library_holds_exactly_the_parameter_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_host_unit_carries_no_parameter_device_code():
    hosts = {unit: open(unit).read() for unit in build.HOST_UNITS}
    assert '#include "mwrt_par.hip.h"' in hosts[build.SRC]
    assert all("__global__" not in text and "mwrt_oe_blocks.hip.h" not in text for text in hosts.values())
    csrc = os.path.dirname(build.PAR)
    assert "__global__" not in open(os.path.join(csrc, "mwrt_par.hip.h")).read()
    # the helpers both tangent-linear units use live in one device header, included by both
    shared = open(os.path.join(csrc, "mwrt_tl_dev.hip.h")).read()
    for name in ("struct dd", "hui_w_dw", "layer_value_tl", "block_scan", "block_suffix_excl"):
        assert name in shared, name
        assert not re.search(r"^(?:__device__|struct|template).*\b%s\b" % re.escape(name.split()[-1]), open(build.TL).read(), re.M), name
    for unit in (build.TL, build.PAR):
        assert '#include "mwrt_tl_dev.hip.h"' in open(unit).read(), unit
    assert (build.PAR, []) in build.UNITS


def test_abi_surface_of_the_parameter_jacobian(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtParam
    assert [f[0] for f in rec._fields_] == ["field", "line"] and ctypes.sizeof(rec) == 8
    assert re.search(r"typedef struct mwrt_param \{ int32_t field; int32_t line; \} mwrt_param;", header)
    assert re.search(r"#define MWRT_MAX_PARAMS (\d+)", header).group(1) == str(_native.MAX_PARAMS)
    assert re.search(r"#define MWRT_PAR_ALL_LINES \((-?\d+)\)", header).group(1) == str(_native.PAR_ALL_LINES)
    # the field ids of the header are the binding's, name for name
    ids = {n.lower(): int(v) for n, v in re.findall(r"#define MWRT_PAR_([A-Z0-9_]+)\s+(\d+)\b", header) if n != "NFIELDS"}
    assert ids == _native.PARAM_FIELDS and len(ids) == 24
    assert int(re.search(r"#define MWRT_PAR_NFIELDS\s+(\d+)", header).group(1)) == 24
    assert native_lib.mwrt_version() == 301 == _native.MWRT_VERSION


def test_null_arguments_are_refused_without_a_gpu(native_lib):
    one = (_native.MwrtParam * 1)()
    fake = ctypes.c_void_p(8)                                            # never dereferenced: the NULL beside it is seen first
    dev_args = [1, 2, None, None, None, None, 1, None, 1, None, 1, one, None, None, None, None]
    assert native_lib.mwrt_tb_param_jacobian_batch_device(None, None, *dev_args) == -1
    assert native_lib.mwrt_tb_param_jacobian_batch_device(None, fake, *dev_args) == -1
    assert native_lib.mwrt_tb_param_jacobian_batch_device(fake, None, *dev_args) == -1
    assert b"null" in native_lib.mwrt_last_error()
    assert native_lib.mwrt_tb_param_jacobian_batch(None, None, *dev_args[:-1]) == -1
