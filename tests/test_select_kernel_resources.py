"""The unit of the observation selection (csrc/mwrt_select.hip) without a GPU: the compiler's resource remark
for the kernel of mwrt::sel, cross-compiled for gfx950 with the library's flags; the LDS plan against its formula; the
inventory of mwrt::sel kernels in libmwrt.so; the new ABI surface -- declared, exported, bound, in the build recipe, one
record layout on both sides; and the guard of the GPU tests' shape list against the plan as built."""
import ctypes
import os
import re
import subprocess

from mwr_fast_forward_operators_and_lbls_amd import _native, build

import select_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(build.CSRC, "mwrt_select.hip.h")
SYMBOLS = ("mwrt_oe_select_device", "mwrt_oe_select_size")
KERNELS = {"k_sel_select"}
# (VGPRs at most, waves per SIMD at least), from the remark of the build this test was written against (110 VGPRs, rounded up
# to a multiple of 8; occupancy as shown).  One workgroup is four waves, one per SIMD, so four waves per SIMD let four
# profiles share a CU when their LDS blocks fit (n <= 80 or so); beyond that the packed S bounds the residency, not registers.
BUDGET = {"k_sel_select": (112, 4)}


def constants():
    text = open(HEADER).read()
    assert "constexpr int THREADS = oe::THREADS;" in text and "constexpr int WAVES = THREADS / 64;" in text
    assert "constexpr int ROWS_IN_FLIGHT = 4;" in text
    threads = int(re.search(r"constexpr int THREADS = (\d+);", open(os.path.join(build.CSRC, "mwrt_oe.hip.h")).read()).group(1))
    return dict(THREADS=threads, WAVES=threads // 64)


def lds_bytes(n, c):
    """packed S | v | u | k_j (then w) | the waves' best q | their indices and candidate counts"""
    even = lambda v: (v + 1) & ~1                                        # noqa: E731
    return 8 * (even(n * (n + 1) // 2) + 3 * even(n) + c["WAVES"] + c["WAVES"])


def test_the_kernel_keeps_its_register_budget(tmp_path):
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", build.SELECT, "-o", str(tmp_path / "select.o")]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    use, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            s = re.search(r"\d+(k_sel_\w+?)E", m.group(1))
            name = s.group(1) if s else m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name is not None:
            use.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    assert set(use) == KERNELS, use
    for name, u in use.items():
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (name, u)
        vgprs, waves = BUDGET[name]
        assert u["VGPRs"] <= vgprs and u["Occupancy"] >= waves, (name, u)
        assert u["LDS"] <= 256, (name, u)                                # static LDS: nothing but the dynamic block's stub


def test_the_lds_plan_follows_its_formula(tmp_path):
    """The plan is host and device code in one header: a host program that prints it for every n is compiled here with
    hipcc and held against the formula of DESIGN 4.12, written out again from the constants."""
    c = constants()
    assert c == dict(THREADS=256, WAVES=4)
    src = tmp_path / "plans.hip"
    src.write_text('#include <cstdio>\n#include "%s"\nint main() {\n  for (int n = 1; n <= MWRT_OE_NFORM_MAX_N; ++n) {\n'
                   '    const mwrt::sel::SelPlan p = mwrt::sel::sel_plan(n);\n'
                   '    std::printf("%%d %%zu %%zu %%zu %%zu %%zu %%zu %%d\\n", n, p.total_bytes, p.v, p.u, p.kj, p.best, p.ints,\n'
                   '                mwrt::sel::cols_per_lane(n));\n  }\n  return 0;\n}\n' % HEADER)
    exe = str(tmp_path / "plans")
    subprocess.run([build.hipcc_path(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True, capture_output=True)
    rows = [tuple(map(int, ln.split())) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(1, _native.OE_NFORM_MAX_N + 1))
    for n, total, v, u, kj, best, ints, cpl in rows:
        nte, np_ = (n * (n + 1) // 2 + 1) & ~1, (n + 1) & ~1
        assert (v, u, kj, best, ints) == (nte, nte + np_, nte + 2 * np_, nte + 3 * np_, nte + 3 * np_ + c["WAVES"]), n
        assert total == lds_bytes(n, c) and total % 16 == 0, n
        assert cpl == -(-n // 64) and 1 <= cpl <= 2, n
    assert rows[-1][1] == 8 * (8256 + 3 * 128 + 8) == 69184 <= 160 * 1024                    # one packed triangle of 66 KB
    assert min(n for n, total, *_ in rows if total > 64 * 1024) == 125


def test_library_holds_exactly_the_select_kernels(native_lib):
    out = subprocess.run(["nm", "-C", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = re.search(r"mwrt::sel::(?:\(anonymous namespace\)::)?(k_\w+(?:<[^>()]*>)?)\(", line)
        if m:
            found.add(m.group(1))
    assert found == KERNELS, found
    # and nothing of the unit leaks into the inventories the other tests pin: no k_sel_ outside mwrt::sel, none directly in mwrt
    assert not re.search(r"mwrt::(?:oe::|lm::|nf::|nfc::|oec::|basis::)?(?:\(anonymous namespace\)::)?k_sel_", out)
    assert all(name.startswith("k_sel_") for name in KERNELS)


def test_abi_surface_of_the_selection(native_lib):
    header = open(os.path.join(ROOT, "include", "mwrt.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeSelect
    assert native_lib.mwrt_oe_select_size() == ctypes.sizeof(rec) == 176
    assert ("mwrt_oe_select", rec, "_native.py") in _native._RECORD_SIZES
    # the record in the header, field by field and in order, is the ctypes mirror; every pointer 8 bytes after the last
    body = re.search(r"typedef struct mwrt_oe_select \{(.*?)\} mwrt_oe_select;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in rec._fields_], names
    assert [getattr(rec, n).offset for n in names[:7]] == [0, 4, 8, 12, 16, 20, 24]
    assert [getattr(rec, n).offset for n in names[7:]] == list(range(56, 176, 8))
    assert native_lib.mwrt_version() == 301
    # the unit is in the build recipe, its entry in the host unit that holds no device code
    assert (build.SELECT, []) in build.UNITS and len(build.HOST_UNITS) == 2
    host = open(build.RETRIEVAL).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, host), sym
    assert "__global__" not in host and "__global__" not in open(HEADER).read()
    records = open(build.RECORDS).read()                                 # the argument stage: plain C++, no HIP
    assert "oe_select_args" in records and "hip_runtime" not in records and ".hip.h" not in records
    assert hasattr(_native.Context, "oe_select_device")
    # a NULL handle or record is refused, not dereferenced (no GPU needed)
    assert native_lib.mwrt_oe_select_device(None, 1, 2, 1, None, None) == -1
    assert native_lib.mwrt_oe_select_device(None, 1, 2, 1, ctypes.byref(rec()), None) == -1


def test_the_shapes_keep_both_sides_of_every_edge():
    """select_reference.SHAPES (what tests/test_oe_select.py runs) against the plan as built: a lane's one element of a row
    and two (n = 64 | 65), both sides of the first raise of the LDS limit, n = 1 and the limit, one, two and four blocks, m
    below n, m below and beyond one row per wave and per thread, nsel = m and nsel < m."""
    c = constants()
    shapes = sr.SHAPES
    ns = {nlev * nblk for nlev, nblk, _, _ in shapes}
    assert all(n <= _native.OE_NFORM_MAX_N for n in ns) and {1, _native.OE_NFORM_MAX_N} <= ns
    assert {64, 65} <= ns
    raised = min(n for n in range(1, 129) if lds_bytes(n, c) > 64 * 1024)
    assert {raised - 1, raised} <= ns, raised
    assert {nblk for _, nblk, _, _ in shapes} >= {1, 2, 4}
    assert any(m < nlev * nblk for nlev, nblk, m, _ in shapes) and any(m > 2 * c["THREADS"] for _, _, m, _ in shapes)
    assert any(m % c["WAVES"] for _, _, m, _ in shapes) and any(m > _native.OE_MAX_M for _, _, m, _ in shapes)
    assert any(nsel == m for _, _, m, nsel in shapes) and any(nsel < m for _, _, m, nsel in shapes)
    assert all(1 <= nsel <= m for _, _, m, nsel in shapes)
    assert all(s in shapes for s in [(1, 1, 5, 5), (8, 1, 20, 20), (12, 2, 224, 24), (33, 1, 16, 16), (64, 1, 140, 40),
                                     (65, 1, 300, 32), (32, 4, 513, 32)])
