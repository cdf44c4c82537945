"""The unit of the n-form's characterisation (csrc/mwrt_nform_char.hip) without a GPU: the compiler's
resource remark for every kernel of mwrt::nfc, cross-compiled for gfx950 with the library's flags; the LDS plan against its
formula; the inventory of mwrt::nfc kernels in libmwrt.so; the new ABI surface -- declared, exported, bound, in the build
recipe, one record layout on both sides; and the guard of the GPU tests' shape list against the plans as built."""
import ctypes
import os
import re

from kernel_unit import MWRT_H, check_record, library_kernels, plan_rows, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

import nform_char_reference as ncr

HEADER = os.path.join(build.CSRC, "mwrt_nform_char.hip.h")
SYMBOLS = ("mwrt_oe_nform_char_device", "mwrt_oe_nform_gain_device", "mwrt_oe_nform_char_size")
NAMESPACE = "nfc"            # the kernels live in mwrt::nfc
KERNELS = {"k_nfc_char", "k_nfc_gain"}
# (VGPRs at most, waves per SIMD at least), from the remark of the build this test was written against (38 and 128 VGPRs,
# rounded up to a multiple of 8; occupancy as shown): k_nfc_char must not be held back by registers (its LDS block is what
# bounds it), k_nfc_gain holds a 4 x 4 tile of accumulators and one chunk in flight and must keep four waves per SIMD.
BUDGET = {"k_nfc_char": (40, 8), "k_nfc_gain": (128, 4)}
GAIN_STATIC_LDS = 8 * (16 * 129 + 16 * 32)                               # Ks [KCHUNK][KPITCH] | Ss [KCHUNK][COLS]


def constants():
    """The plan constants of csrc/mwrt_nform_char.hip.h as written (THREADS is oe::THREADS)."""
    text = open(HEADER).read()
    c = {name: int(value) for name, value in re.findall(r"constexpr int (\w+) = (\d+);", text)}
    assert set(c) == {"ROWS", "COLS", "KCHUNK", "MR", "NC"} and "constexpr int THREADS = oe::THREADS;" in text
    assert "constexpr int KPITCH = ROWS + 1;" in text
    c["THREADS"] = int(re.search(r"constexpr int THREADS = (\d+);", open(os.path.join(build.CSRC, "mwrt_oe.hip.h")).read()).group(1))
    return c


def char_lds_bytes(n, c):
    even = lambda v: (v + 1) & ~1                                        # noqa: E731
    return 8 * (2 * even(n * (n + 1) // 2) + even(n) + c["THREADS"])


def test_the_kernels_keep_their_register_budget():
    use = resource_usage(build.NFORM_CHAR)
    assert set(use) == KERNELS, use                                      # every kernel of the unit is one of the two
    for name, u in use.items():
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (name, u)
        vgprs, waves = BUDGET[name]
        assert u["VGPRs"] <= vgprs and u["Occupancy"] >= waves, (name, u)
    assert use["k_nfc_char"]["LDS"] <= 256                               # static LDS: nothing but the dynamic block's stub
    assert use["k_nfc_gain"]["LDS"] == GAIN_STATIC_LDS == 20608


def test_the_lds_plan_follows_its_formula(tmp_path):
    """The plan is host and device code in one header: a host program that prints it for every n is compiled here with
    hipcc and held against the formula of DESIGN 4.11.1, written out again from the constants."""
    c = constants()
    assert c == dict(ROWS=128, COLS=32, KCHUNK=16, MR=4, NC=4, THREADS=256)
    assert c["THREADS"] // 8 * c["MR"] == c["ROWS"] and 8 * c["NC"] == c["COLS"] and 2 * c["THREADS"] == c["KCHUNK"] * c["COLS"]
    rows = plan_rows(HEADER, '    std::printf("%d %zu %zu %zu %d %d\\n", n, mwrt::nfc::char_plan(n).total_bytes, mwrt::nfc::char_plan(n).s,\n'
                             '                mwrt::nfc::char_plan(n).dg, mwrt::nfc::cols_per_lane(n), mwrt::nfc::gain_col_tiles(n));',
                     tmp_path)
    assert [r[0] for r in rows] == list(range(1, _native.OE_NFORM_MAX_N + 1))
    for n, total, s, dg, cpl, ctiles in rows:
        nte = (n * (n + 1) // 2 + 1) & ~1
        assert (s, dg) == (nte, 2 * nte) and total == char_lds_bytes(n, c), n                # the two triangles do not overlap
        assert cpl == -(-n // 64) and 1 <= cpl <= 2 and ctiles == -(-n // c["COLS"]), n
    assert rows[-1][1] == 8 * (2 * 8256 + 128 + 256) == 135168 <= 160 * 1024                  # two packed triangles of 66 KB
    assert min(n for n, total, *_ in rows if total > 64 * 1024) == 89


def test_library_holds_exactly_the_nform_char_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS
    assert not any(name.startswith("k_nf_") for name in KERNELS)


def test_abi_surface_of_the_nform_char(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeNformChar
    assert native_lib.mwrt_oe_nform_size() == ctypes.sizeof(_native.MwrtOeNform) == 240
    # the record in the header, field by field and in order, is the ctypes mirror; every pointer 8 bytes after the last
    check_record(native_lib, "mwrt_oe_nform_char", rec, 168, offsets=[0, 4, 8, 12, 16, 20, 24] + list(range(56, 168, 8)))
    assert native_lib.mwrt_version() == 301
    # the unit is in the build recipe, its entries in the host unit that holds no device code
    assert (build.NFORM_CHAR, []) in build.UNITS and len(build.HOST_UNITS) == 2
    host = open(build.RETRIEVAL).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, host), sym
    assert "__global__" not in host and "__global__" not in open(HEADER).read()
    records = open(build.RECORDS).read()                                 # the argument stage: plain C++, no HIP
    assert "oe_nform_char_args" in records and "hip_runtime" not in records and ".hip.h" not in records
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    for sym in SYMBOLS[:2]:
        assert getattr(native_lib, sym)(None, 1, 2, 1, None, None) == -1
        assert getattr(native_lib, sym)(None, 1, 2, 1, ctypes.byref(rec()), None) == -1


def test_the_shapes_keep_both_sides_of_every_edge():
    """nform_char_reference.SHAPES (what tests/test_oe_nform_char.py runs) against the plans as built.  k_nfc_char: a lane's
    one column of A and two (n = 64 | 65), both sides of the first raise of its LDS limit, n = 1 and the limit, one to four
    blocks.  k_nfc_gain: one row tile and two; a last row tile full, short by one row and one row long; one column tile
    and two and the last; a contraction chunk full and short by one; an m beyond MWRT_OE_MAX_M."""
    c = constants()
    shapes = ncr.SHAPES
    ns = {nlev * nblk for nlev, nblk, _ in shapes}
    ms = {m for _, _, m in shapes}
    assert all(n <= _native.OE_NFORM_MAX_N for n in ns) and {1, _native.OE_NFORM_MAX_N} <= ns
    assert {64, 65} <= ns                                                # lane l's columns l and l + 64
    raised = min(n for n in range(1, 129) if char_lds_bytes(n, c) > 64 * 1024)
    assert {raised - 1, raised} <= ns, raised
    assert {nblk for _, nblk, _ in shapes} == {1, 2, 3, 4}
    rows, cols, kc = c["ROWS"], c["COLS"], c["KCHUNK"]
    assert any(m < rows for m in ms) and any(rows < m <= 2 * rows for m in ms) and any(m > 2 * rows for m in ms)
    assert {rows - 1, rows, rows + 1} <= ms and {m % rows for m in ms} >= {0, 1, rows - 1}
    assert any(m % rows == 0 and m > rows for m in ms) and any(m % rows == 1 and m > 2 * rows for m in ms)
    assert {cols - 1, cols, cols + 1} <= ns and {-(-n // cols) for n in ns} == {1, 2, 3, 4}
    assert {n % kc for n in ns} >= {0, 1, kc - 1} and any(n < kc for n in ns) and any(n % kc == kc - 1 and n > kc for n in ns)
    assert any(m > _native.OE_MAX_M for m in ms)
    assert all(s in shapes for s in [(8, 1, 128), (9, 2, 127), (5, 3, 129), (40, 1, 256), (65, 1, 300), (128, 1, 513)])
