"""The ray-traced K-matrix unit (csrc/mwrt_ray.hip) without a GPU: the compiler's resource remark for its two
kernels, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::ray kernels in libmwrt.so; and the new
ABI surface -- declared, exported, bound, in the build recipe."""
import inspect
import os
import re

from kernel_unit import MWRT_H, library_kernels, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

NAMESPACE = "ray"            # the kernels live in mwrt::ray
KERNELS = {"k_ray_paths_tl", "k_jac_rte_ray"}
SYMBOLS = ("mwrt_tb_jacobian_batch_ray_device", "mwrt_tb_jacobian_batch_ray")


def test_ray_kernels_keep_what_they_achieved():
    """What the compiler gives today, as bounds (the same figures stand in DESIGN 4.5.4).  k_jac_rte_ray is the loop that
    runs per (profile, frequency): no scratch, four waves per SIMD (a 1024-lane workgroup's ceiling is 128 VGPRs).
    k_ray_paths_tl runs once per profile and carries a five-direction tangent through the ray tracer: it sits at that
    ceiling and spills."""
    use = resource_usage(build.RAY)
    assert set(use) == KERNELS, use
    rte, path = use["k_jac_rte_ray"], use["k_ray_paths_tl"]
    assert rte["ScratchSize"] == 0 and rte["VGPRs"] <= 105 and rte["Occupancy"] >= 4, rte
    assert rte["LDS"] <= 256, rte                                        # static LDS: none beyond the dynamic rows
    assert path["VGPRs"] <= 128 and path["Occupancy"] >= 4 and path["ScratchSize"] <= 320, path
    assert path["LDS"] <= 16 * 9 * 8 + 256, path                         # the wave seams


def test_library_holds_exactly_the_ray_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_unit_layout_and_build_recipe():
    csrc = os.path.dirname(build.RAY)
    assert "__global__" not in open(os.path.join(csrc, "mwrt_ray.hip.h")).read()
    assert "__global__" not in open(os.path.join(csrc, "mwrt_tl_rte.hip.h")).read()
    hosts = {unit: open(unit).read() for unit in build.HOST_UNITS}
    assert '#include "mwrt_ray.hip.h"' in hosts[build.SRC]
    assert all("__global__" not in text and "mwrt_oe_blocks.hip.h" not in text for text in hosts.values())
    # one adjoint RTE, two kernels: both units instantiate the shared body
    assert "jac_rte_body<false>" in open(build.TL).read() and "jac_rte_body<true>" in open(build.RAY).read()
    assert (build.RAY, []) in build.UNITS


def test_abi_surface_of_the_ray_entries(native_lib):
    header = open(MWRT_H).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header) and hasattr(native_lib, s) and s in _native.SIGNATURES, s
    assert native_lib.mwrt_version() == 301 == _native.MWRT_VERSION
    assert len(_native.SIGNATURES[SYMBOLS[0]][1]) == len(_native.SIGNATURES["mwrt_tb_jacobian_batch_vars_device"][1])
    assert len(_native.SIGNATURES[SYMBOLS[1]][1]) == len(_native.SIGNATURES["mwrt_tb_jacobian_batch_vars"][1])
    for name in ("tb_jacobian_batch_ray_device", "tb_jacobian_batch_ray"):
        params = inspect.signature(getattr(_native.Context, name)).parameters
        assert "ray_tracing" not in params and "d_o3n" not in params, name
        assert getattr(_native.Context, name).__wrapped__ is not None       # @_serialised
    # NULL handles are refused before anything is dereferenced
    null = [None] * 20
    assert native_lib.mwrt_tb_jacobian_batch_ray_device(None, None, 1, 2, *null[:4], 1, None, 1, *null[:10], None) == -1
    assert native_lib.mwrt_tb_jacobian_batch_ray(None, None, 1, 2, *null[:4], 1, None, 1, *null[:10]) == -1
