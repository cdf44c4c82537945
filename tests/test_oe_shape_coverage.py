"""What tests/oe_reference.py::SHAPES reaches in the optimal-estimation kernels, without a GPU.

The step, Levenberg-Marquardt and characterisation suites take every shape from that one list, and what a shape reaches is
decided by rules that live in the code: the launchers dispatch k_oe_step<MR>, k_lm_prepare<MR> and k_char_gain<MR> on the
row-tile count ceil(m / ROW_TILE); a launch whose dynamic LDS is above 64 KiB goes through the raise of the kernel's limit;
and the four plans (oe::lds_plan, lm::solve_plan, lm::cost_plan, oec::gain_plan) decide that size and, in oe::lds_plan,
whether the state vector outgrows the panel buffers it aliases.  This test restates those rules, holds the restatement to
the code (a host program that includes the three headers prints the plans for every m; the dispatch and the raise are
held by their text), and asserts the list against it: a shape dropped from SHAPES, or a plan that moves a seam, fails here
instead of silently un-testing an instantiation."""
import os
import subprocess

import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native, build

PANEL, KCHUNK, ROW_TILE, THREADS, PARTS = 32, 16, 32, 256, 8
LDS_DEFAULT = 64 * 1024                      # the dynamic-LDS limit a kernel has before launch_raised raises it

PROBE = r"""
#include "mwrt_oe_char.hip.h"
#include "mwrt_oe_lm.hip.h"
#include <cstdio>
#include <cstdlib>
using namespace mwrt;
int main(int argc, char** argv) {
  std::printf("%d %d %d %d %d %d %d\n", oe::PANEL, oe::KCHUNK, oe::ROW_TILE, oe::THREADS, oec::PARTS, oe::MAX_ROW_TILES,
              MWRT_OE_MAX_M);
  for (int a = 1; a < argc; ++a) {
    const int n = std::atoi(argv[a]);
    for (int m = 1; m <= MWRT_OE_MAX_M; ++m) {
      const oe::LdsPlan p = oe::lds_plan(m, n);
      std::printf("%d %d %zu %zu %zu %zu %zu %zu\n", m, n, p.total_bytes, lm::solve_plan(m, n).total_bytes,
                  lm::cost_plan(m, n, 0).total_bytes, lm::cost_plan(m, n, 1).total_bytes, oec::gain_plan(m).total_bytes,
                  p.d - p.region);
    }
  }
  return 0;
}
"""


def even(v):
    return (v + 1) & ~1


def tiles(m):
    """the launchers' dispatch: MR of k_oe_step<MR>, k_lm_prepare<MR>, k_char_gain<MR>"""
    return (m + ROW_TILE - 1) // ROW_TILE


def panel_region(m):
    """Wt | Ks | Ss of oe::lds_plan in doubles: what x - xa and v = K^T u alias"""
    return (PANEL + KCHUNK) * (tiles(m) * ROW_TILE + 1) + KCHUNK * PANEL


def region_len(m, n):
    return even(max(panel_region(m), n))


def step_bytes(m, n):
    """oe::lds_plan: k_oe_step and k_lm_prepare"""
    mp = tiles(m) * ROW_TILE
    return 8 * (even(m * (m + 1) // 2) + region_len(m, n) + 3 * mp + THREADS + mp // 2)


def solve_bytes(m, n):
    mp = even(m)
    return 8 * (even(m * (m + 1) // 2) + 2 * mp + even(n) + mp // 2)


def cost_bytes(m, n, se_full):
    mp = even(m)
    return 8 * (even(n) + mp + THREADS + mp // 2 + (even(m * (m + 1) // 2) if se_full else 0))


def gain_bytes(m, n=None):
    mp = tiles(m) * ROW_TILE
    kpitch = mp + 1
    ks = even(m * (m + 1) // 2) + even(PANEL * kpitch)
    part = even(ks + KCHUNK * kpitch + KCHUNK * PANEL)
    return 8 * (part + 2 * PARTS * PANEL + mp + THREADS + mp // 2)


def plans_of_the_code(tmp_path, ns):
    """{(m, n): (step, solve, cost diag, cost full, gain, region length)} for every m and the given n, and the constants,
    as a host program that includes the headers prints them."""
    csrc = os.path.dirname(build.OE)
    src, exe = tmp_path / "oe_plans.cpp", tmp_path / "oe_plans"
    src.write_text(PROBE)
    subprocess.run([build.hipcc_path(), "-x", "hip", "--offload-host-only", "-std=c++17", "-I" + csrc, str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    lines = subprocess.run([str(exe)] + [str(n) for n in ns], check=True, capture_output=True, text=True).stdout.splitlines()
    table = {}
    for line in lines[1:]:
        v = [int(t) for t in line.split()]
        table[(v[0], v[1])] = tuple(v[2:])
    return [int(t) for t in lines[0].split()], table


def test_the_shapes_reach_what_they_are_for(tmp_path):
    shapes = set(oer.SHAPES)
    assert len(shapes) == len(oer.SHAPES)
    ms = {m for _, _, m in shapes}
    ns = sorted({nlev * nblk for nlev, nblk, _ in shapes})

    # ---- the restatement above is the code ----
    consts, code = plans_of_the_code(tmp_path, ns)
    max_m = _native.OE_MAX_M
    assert consts == [PANEL, KCHUNK, ROW_TILE, THREADS, PARTS, tiles(max_m), max_m], consts
    assert len(code) == max_m * len(ns)
    for (m, n), got in code.items():
        want = (step_bytes(m, n), solve_bytes(m, n), cost_bytes(m, n, False), cost_bytes(m, n, True), gain_bytes(m),
                region_len(m, n))
        assert got == want, (m, n, got, want)
    csrc = os.path.dirname(build.OE)
    text = {name: open(os.path.join(csrc, name)).read() for name in ("mwrt_oe.hip", "mwrt_oe_lm.hip", "mwrt_oe_char.hip",
                                                                     "mwrt_oe_blocks.hip.h")}
    for name, m_of, kernel in (("mwrt_oe.hip", "a.m", "launch_mr<%d>("), ("mwrt_oe_lm.hip", "a.o.m", "launch_raised<k_lm_prepare<%d>>("),
                               ("mwrt_oe_char.hip", "a.o.m", "launch_raised<k_char_gain<%d>>(")):
        assert "switch ((%s + ROW_TILE - 1) / ROW_TILE) {" % m_of in text[name], name
        for mr in range(1, tiles(max_m) + 1):
            assert ("case %d: return " % mr + kernel % mr) in text[name], (name, mr)
        assert "case %d:" % (tiles(max_m) + 1) not in text[name], name
    assert "return launch_raised<k_oe_step<MR>>(a, nprof, lds, st);" in text["mwrt_oe.hip"]
    assert "if (lds > 64 * 1024) {" in text["mwrt_oe_blocks.hip.h"]
    assert "if (rlen < (size_t)n) rlen = (size_t)n;" in open(os.path.join(csrc, "mwrt_oe.hip.h")).read()

    # ---- every instantiation, both sides of every tile edge, the ends of m, every count of state blocks ----
    assert {tiles(m) for m in ms} == set(range(1, tiles(max_m) + 1))
    for k in range(1, tiles(max_m)):
        assert ROW_TILE * k in ms and ROW_TILE * k + 1 in ms, k
    assert 1 in ms and max_m in ms
    assert {nblk for _, nblk, _ in shapes} == {1, 2, 3, 4}
    # wave 0's solves keep entry i in lane i & 63 of register i >> 6: the last lane of v0 and v1, the first of v1 and v2
    assert {64, 65, 128, 129} <= ms

    # ---- the first raise of every kernel's LDS limit: one shape at or below 64 KiB, its neighbour in m above it ----
    def straddles(nbytes):
        return sorted((nlev, nblk, m) for nlev, nblk, m in shapes if (nlev, nblk, m + 1) in shapes
                      and nbytes(m, nlev * nblk) <= LDS_DEFAULT < nbytes(m + 1, nlev * nblk))

    seams = {name: straddles(f) for name, f in (("step", step_bytes), ("gain", gain_bytes), ("solve", solve_bytes),
                                                ("cost", lambda m, n: cost_bytes(m, n, True)))}
    assert all(seams.values()), seams
    # ... which is the kernel's first: the plans grow with m, so nothing below the lower shape is above the limit
    for f in (step_bytes, solve_bytes, gain_bytes, lambda m, n: cost_bytes(m, n, True), lambda m, n: cost_bytes(m, n, False)):
        for n in ns:
            assert all(f(m, n) <= f(m + 1, n) for m in range(1, max_m)), n
    # with a diagonal Se the cost kernel never needs the raise at those n (its plan has no term in m^2)
    assert all(cost_bytes(max_m, nlev * nblk, False) <= LDS_DEFAULT for nlev, nblk, _ in seams["cost"])

    # ---- the state vector outgrows the panel buffers it aliases (the `rlen < n` arm), narrowly, at tile counts 1 and 2 ----
    for mr in (1, 2):
        over = [(nlev, nblk, m) for nlev, nblk, m in shapes if tiles(m) == mr and 0 < nlev * nblk - panel_region(m) < 32]
        assert over, mr
        for nlev, nblk, m in over:                               # and the arm is what sizes the block there
            assert region_len(m, nlev * nblk) == even(nlev * nblk) > panel_region(m)
    # every other shape of the list stays inside them: the arm is reached by those shapes alone
    assert any(nlev * nblk <= panel_region(m) and nlev * nblk > 2000 for nlev, nblk, m in shapes)

    # ---- the level axis: a panel remainder, and the wave seam of the rows' lane loops ----
    assert any((nlev * nblk) % PANEL for nlev, nblk, _ in shapes) and any((nlev * nblk) % PANEL == 0 for nlev, nblk, _ in shapes)
    nlevs = {nlev for nlev, _, _ in shapes}
    assert {63, 64, 65} <= nlevs and min(nlevs) < 64 < max(nlevs)
