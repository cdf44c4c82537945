"""The ray-traced K-matrix unit (csrc/mwrt_ray.hip) without a GPU: the compiler's resource remark for its two
kernels, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::ray kernels in libmwrt.so; and the new
ABI surface -- declared, exported, bound, in the build recipe."""
import inspect
import os
import re
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import _native, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_ray_paths_tl", "k_jac_rte_ray"}
SYMBOLS = ("mwrt_tb_jacobian_batch_ray_device", "mwrt_tb_jacobian_batch_ray")


def resource_usage(tmp_path):
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", build.RAY, "-o", str(tmp_path / "ray.o")]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            s = re.search(r"\d+(k_\w+?)ENS", m.group(1))
            name = s.group(1) if s else m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name is not None:
            out.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_ray_kernels_keep_what_they_achieved(tmp_path):
    """What the compiler gives today, as bounds (the same figures stand in DESIGN 4.5.4).  k_jac_rte_ray is the loop that
    runs per (profile, frequency): no scratch, four waves per SIMD (a 1024-lane workgroup's ceiling is 128 VGPRs).
    k_ray_paths_tl runs once per profile and carries a five-direction tangent through the ray tracer: it sits at that
    ceiling and spills."""
    use = resource_usage(tmp_path)
    assert set(use) == KERNELS, use
    rte, path = use["k_jac_rte_ray"], use["k_ray_paths_tl"]
    assert rte["ScratchSize"] == 0 and rte["VGPRs"] <= 105 and rte["Occupancy"] >= 4, rte
    assert rte["LDS"] <= 256, rte                                        # static LDS: none beyond the dynamic rows
    assert path["VGPRs"] <= 128 and path["Occupancy"] >= 4 and path["ScratchSize"] <= 320, path
    assert path["LDS"] <= 16 * 9 * 8 + 256, path                         # the wave seams


def test_library_holds_exactly_the_ray_kernels(native_lib):
    out = subprocess.run(["nm", "-C", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"mwrt::ray::(?:\(anonymous namespace\)::)?(k_\w+(?:<[^>()]*>)?)\(", line)
        if m:
            found.add(m.group(1))
    assert found == KERNELS, found
    # and nothing of the unit leaks into the inventory tests/test_kernel_instantiations.py pins
    assert not re.search(r"mwrt::(?:\(anonymous namespace\)::)?k_(?:ray_paths_tl|jac_rte_ray)", out)


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
    header = open(os.path.join(ROOT, "include", "mwrt.h")).read()
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
