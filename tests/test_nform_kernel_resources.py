"""The n-form unit (csrc/mwrt_nform.hip) without a GPU: the compiler's resource remark for every kernel of
mwrt::nf, cross-compiled for gfx950 with the library's flags; the LDS plans against their formulas; the inventory of mwrt::nf
kernels in libmwrt.so; the new ABI surface -- declared, exported, bound, in the build recipe, one record layout on both
sides; and the guard of the tests' shape list against the plan constants as built."""
import ctypes
import os
import re

from kernel_unit import MWRT_H, check_record, library_kernels, plan_rows, resource_usage
from mwr_fast_forward_operators_and_lbls_amd import _native, build

import nform_reference as nfr

HEADER = os.path.join(build.CSRC, "mwrt_nform.hip.h")
SYMBOLS = ("mwrt_oe_nform_prepare_device", "mwrt_oe_nform_solve_device", "mwrt_oe_nform_cost_device", "mwrt_oe_nform_size")
NAMESPACE = "nf"            # the kernels live in mwrt::nf
KERNELS = {"k_nf_normal<1>", "k_nf_normal<2>", "k_nf_normal<3>", "k_nf_solve", "k_nf_cost"}
# (VGPRs at most, waves per SIMD at least), from the remark of the build this test was written against (146 / 232 / 230,
# 88 and 28 VGPRs): k_nf_normal<TT> holds TT 4 x 4 tiles of accumulators and one chunk of K in flight and must keep two
# workgroups of four waves resident per CU; the solve and the cost must not be held back by registers.
BUDGET = {"k_nf_normal<1>": (160, 3), "k_nf_normal<2>": (240, 2), "k_nf_normal<3>": (240, 2), "k_nf_solve": (96, 5),
          "k_nf_cost": (40, 8)}


def constants():
    """The plan constants of csrc/mwrt_nform.hip.h as written (THREADS is oe::THREADS)."""
    text = open(HEADER).read()
    c = {name: int(value) for name, value in re.findall(r"constexpr int (\w+) = (\d+);", text)}
    assert set(c) == {"ROW_CHUNK", "TILE", "MAX_TILES"} and "constexpr int THREADS = oe::THREADS;" in text
    c["THREADS"] = int(re.search(r"constexpr int THREADS = (\d+);", open(os.path.join(build.CSRC, "mwrt_oe.hip.h")).read()).group(1))
    return c


def tiles_per_thread(n, c):
    nb = -(-n // c["TILE"])
    return -(-(nb * (nb + 1) // 2) // c["THREADS"])


def solve_lds_bytes(n, c):
    even = lambda v: (v + 1) & ~1                                        # noqa: E731
    return 8 * (even(n * (n + 1) // 2) + 4 * even(n) + c["THREADS"])


def test_nform_kernels_keep_their_register_budget():
    use = resource_usage(build.NFORM)
    assert set(use) == KERNELS, use                                      # every kernel of the unit is one of the three
    for name, u in use.items():
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (name, u)
        assert u["LDS"] <= 256, (name, u)                                # static LDS: nothing but the dynamic block's stub
        vgprs, waves = BUDGET[name]
        assert u["VGPRs"] <= vgprs and u["Occupancy"] >= waves, (name, u)


def test_the_lds_plans_follow_their_formulas(tmp_path):
    """The plans are host and device code in one header: a host program that prints them for every n is compiled here with
    hipcc and held against the formulas of DESIGN 4.11, written out again from the constants."""
    c = constants()
    assert c == dict(ROW_CHUNK=16, TILE=4, MAX_TILES=3, THREADS=256)
    assert c["ROW_CHUNK"] % (c["THREADS"] // 64) == 0                    # whole rows per wave
    assert tiles_per_thread(_native.OE_NFORM_MAX_N, c) == c["MAX_TILES"]
    rows = plan_rows(HEADER, '    std::printf("%d %d %d %zu %zu %zu\\n", n, mwrt::nf::tiles_per_thread(n), mwrt::nf::normal_plan(n).pitch,\n'
                             '                mwrt::nf::normal_plan(n).total_bytes, mwrt::nf::solve_plan(n).total_bytes,\n'
                             '                mwrt::nf::cost_plan(n).total_bytes);', tmp_path)
    assert [r[0] for r in rows] == list(range(1, _native.OE_NFORM_MAX_N + 1))
    for n, tt, pitch, normal, solve, cost in rows:
        assert tt == tiles_per_thread(n, c) and 1 <= tt <= c["MAX_TILES"], n
        assert pitch == -(-n // c["TILE"]) * c["TILE"], n
        assert normal == 8 * (2 * c["ROW_CHUNK"] * pitch + 2 * c["ROW_CHUNK"] + 4), n
        assert solve == solve_lds_bytes(n, c), n
        assert cost == 8 * (((n + 1) & ~1) + c["THREADS"]), n
    assert max(r[3] for r in rows) <= 64 * 1024 and max(r[5] for r in rows) <= 64 * 1024      # never raised
    assert rows[-1][4] == 8 * (8256 + 512 + 256) == 72192                                   # the packed triangle: 66 KB of it


def test_library_holds_exactly_the_nform_kernels(native_lib):
    assert library_kernels(_native.LIB_PATH)[NAMESPACE] == KERNELS


def test_abi_surface_of_the_nform(native_lib):
    header = open(MWRT_H).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in _native.SIGNATURES and hasattr(native_lib, sym), sym
    rec = _native.MwrtOeNform
    assert re.search(r"#define MWRT_OE_NFORM_MAX_N %d\b" % _native.OE_NFORM_MAX_N, header) and _native.OE_NFORM_MAX_N == 128
    # the record in the header, field by field and in order, is the ctypes mirror; every pointer 8 bytes after the last
    check_record(native_lib, "mwrt_oe_nform", rec, 240, offsets=[0, 4, 8, 12, 16, 24] + list(range(56, 240, 8)))
    assert native_lib.mwrt_version() == 301
    # the unit is in the build recipe, its entries in the host unit that holds no device code
    assert (build.NFORM, []) in build.UNITS and len(build.HOST_UNITS) == 2
    host = open(build.RETRIEVAL).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, host), sym
    assert "__global__" not in host and "__global__" not in open(HEADER).read()
    # NULL handles and records are refused, not dereferenced (no GPU needed)
    for sym in SYMBOLS[:3]:
        assert getattr(native_lib, sym)(None, 1, 2, 1, None, None) == -1
        assert getattr(native_lib, sym)(None, 1, 2, 1, ctypes.byref(rec()), None) == -1


def test_the_shapes_keep_both_sides_of_every_edge():
    """nform_reference.SHAPES against the plan as built: every tiles-per-thread count with both sides of each of its edges,
    both sides of the first raise of the solve's LDS limit, of a lane's second column, of a row-chunk edge (one chunk and
    more, a last chunk full, short by one row and one row long), one to four blocks, n = 1 and the limit, and an m beyond
    MWRT_OE_MAX_M."""
    c = constants()
    shapes = nfr.SHAPES
    ns = {nlev * nblk for nlev, nblk, _ in shapes}
    ms = {m for _, _, m in shapes}
    assert all(n <= _native.OE_NFORM_MAX_N for n in ns) and {1, _native.OE_NFORM_MAX_N} <= ns
    for tt in range(1, c["MAX_TILES"]):                                  # the last n of tt tiles per thread | the first of tt + 1
        edge = max(n for n in range(1, 129) if tiles_per_thread(n, c) == tt)
        assert {edge, edge + 1} <= ns, (tt, edge)
    assert {tiles_per_thread(n, c) for n in ns} == set(range(1, c["MAX_TILES"] + 1))
    raised = min(n for n in range(1, 129) if solve_lds_bytes(n, c) > 64 * 1024)
    assert {raised - 1, raised} <= ns, raised
    assert {64, 65} <= ns                                                # lane l's columns l and l + 64
    assert any(n % c["TILE"] for n in ns) and any(n % c["TILE"] == 0 for n in ns)
    rc = c["ROW_CHUNK"]
    assert any(m < rc for m in ms) and {rc, rc + 1, 2 * rc - 1, 2 * rc, 2 * rc + 1} <= ms
    assert {m % rc for m in ms} >= {0, 1, rc - 1} and max(ms) > 64 * rc
    assert {nblk for _, nblk, _ in shapes} == {1, 2, 4} or {nblk for _, nblk, _ in shapes} == {1, 2, 3, 4}
    assert any(m > _native.OE_MAX_M for m in ms) and (33, 1, 141) in shapes
    required = [(1, 1, 1), (2, 1, 1), (1, 2, 3), (8, 1, 98), (31, 1, 14), (32, 1, 98), (33, 1, 141), (64, 1, 140), (65, 1, 300),
                (43, 2, 154), (32, 4, 98), (127, 1, 98), (128, 1, 513), (16, 2, 1025)]
    assert all(s in shapes for s in required)
