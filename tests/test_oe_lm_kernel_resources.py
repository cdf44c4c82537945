"""The Levenberg-Marquardt unit (csrc/mwrt_oe_lm.hip) without a GPU: the compiler's resource remark for every
kernel of mwrt::lm, cross-compiled for gfx950 with the library's flags; the inventory of mwrt::lm kernels in libmwrt.so;
and the new ABI surface -- declared, exported, bound, and one record layout on both sides."""
import ctypes
import os
import re
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import _native, build
from test_oe_kernel_resources import BUDGET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_lm_prepare<MR> is the first three steps of k_oe_step<MR>: it is held to that kernel's VGPR and occupancy budget
KERNELS = {f"k_lm_prepare<{mr}>" for mr in BUDGET} | {"k_lm_solve", "k_lm_cost"}


def resource_usage(tmp_path):
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", build.OE_LM, "-o", str(tmp_path / "oe_lm.o")]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_lm_prepareILi(\d+)E", m.group(1))
            s = re.search(r"\d+(k_lm_solve|k_lm_cost)E", m.group(1))
            name = int(k.group(1)) if k else s.group(1) if s else m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name is not None:
            out.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_lm_kernels_keep_their_register_budget(tmp_path):
    use = resource_usage(tmp_path)
    assert set(use) == set(BUDGET) | {"k_lm_solve", "k_lm_cost"}, use    # every kernel of the unit is one of the three
    for name, u in use.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["LDS"] <= 256, (name, u)                                # static LDS: nothing but the dynamic block's stub
    for mr, (vgprs, waves) in BUDGET.items():
        assert use[mr]["VGPRs"] <= vgprs and use[mr]["Occupancy"] >= waves, (mr, use[mr])
    # the solve is meant to have more than one workgroup (4 waves) per CU resident at m ~ 98: registers must allow it
    assert use["k_lm_solve"]["Occupancy"] >= 3 and use["k_lm_cost"]["Occupancy"] >= 3, use


def test_library_holds_exactly_the_lm_kernels(native_lib):
    out = subprocess.run(["nm", "-C", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"mwrt::lm::(?:\(anonymous namespace\)::)?(k_\w+(?:<[^>()]*>)?)\(", line)
        if m:
            found.add(m.group(1))
    assert found == KERNELS, found
    # and nothing of the unit leaks into the inventories the other tests pin
    assert not re.search(r"mwrt::(?:oe::)?(?:\(anonymous namespace\)::)?k_lm", out)


def test_abi_surface_of_the_split(native_lib):
    header = open(os.path.join(ROOT, "include", "mwrt.h")).read()
    for sym in ("mwrt_oe_lm_prepare_device", "mwrt_oe_lm_solve_device", "mwrt_oe_cost_device", "mwrt_oe_lm_size"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeLm
    assert native_lib.mwrt_oe_lm_size() == ctypes.sizeof(rec) == 224
    # the record in the header, field by field and in order, is the ctypes mirror
    body = re.search(r"typedef struct mwrt_oe_lm \{(.*?)\} mwrt_oe_lm;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in rec._fields_], names
    assert rec.d_k.offset == 24 and rec.d_x.offset == 56 and rec.d_nobs.offset == 216
    assert native_lib.mwrt_version() == 301
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    for sym in ("mwrt_oe_lm_prepare_device", "mwrt_oe_lm_solve_device", "mwrt_oe_cost_device"):
        assert getattr(native_lib, sym)(None, 1, 2, 1, None, None) == -1
        assert getattr(native_lib, sym)(None, 1, 2, 1, ctypes.byref(rec()), None) == -1
