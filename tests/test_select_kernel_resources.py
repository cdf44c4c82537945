"""The unit of the observation selection (csrc/mwrt_select.hip) without a GPU: the compiler's resource remark
for the kernel of mwrt::sel, cross-compiled for gfx950 with the library's flags; the LDS plan against its formula; the
inventory of mwrt::sel kernels in libmwrt.so; the new ABI surface -- declared, exported, bound, in the build recipe, one
record layout on both sides; and the guard of the GPU tests' shape list against the plan as built."""
import ctypes
import os
import re

from kernel_unit import MWRT_H, check_record, library_kernels, plan_rows, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

import select_reference as sr

HEADER = os.path.join(build.CSRC, "mwrt_select.hip.h")
SYMBOLS = ("mwrt_oe_select_device", "mwrt_oe_select_size")
NAMESPACE = "sel"            # the kernels live in mwrt::sel
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


def test_the_kernel_keeps_its_register_budget():
    use = resource_usage(build.SELECT)
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
    rows = plan_rows(HEADER, '    const mwrt::sel::SelPlan p = mwrt::sel::sel_plan(n);\n'
                             '    std::printf("%d %zu %zu %zu %zu %zu %zu %d\\n", n, p.total_bytes, p.v, p.u, p.kj, p.best, p.ints,\n'
                             '                mwrt::sel::cols_per_lane(n));', tmp_path)
    assert [r[0] for r in rows] == list(range(1, _native.OE_NFORM_MAX_N + 1))
    for n, total, v, u, kj, best, ints, cpl in rows:
        nte, np_ = (n * (n + 1) // 2 + 1) & ~1, (n + 1) & ~1
        assert (v, u, kj, best, ints) == (nte, nte + np_, nte + 2 * np_, nte + 3 * np_, nte + 3 * np_ + c["WAVES"]), n
        assert total == lds_bytes(n, c) and total % 16 == 0, n
        assert cpl == -(-n // 64) and 1 <= cpl <= 2, n
    assert rows[-1][1] == 8 * (8256 + 3 * 128 + 8) == 69184 <= 160 * 1024                    # one packed triangle of 66 KB
    assert min(n for n, total, *_ in rows if total > 64 * 1024) == 125


def test_library_holds_exactly_the_select_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS
    assert all(name.startswith("k_sel_") for name in KERNELS)


def test_abi_surface_of_the_selection(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeSelect
    assert ("mwrt_oe_select", rec, "_native.py") in _native._RECORD_SIZES
    # the record in the header, field by field and in order, is the ctypes mirror; every pointer 8 bytes after the last
    check_record(native_lib, "mwrt_oe_select", rec, 176, offsets=[0, 4, 8, 12, 16, 20, 24] + list(range(56, 176, 8)))
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
