"""The LDS row stride that the sorted K2 passes of k_tb_fused rely on, asked of the planning code itself (CPU).

A sorted pass runs every segment for the full `seglen` layers, so the last segment of a row reads up to index
nseg * seglen; the kernel zero-fills each row from nlev to the stride.  The stride therefore has to reach past that index for
every geometry the planner can emit -- also after plan_fused has shrunk the split to fit a small LDS -- and stays odd
(ds_read_b64 rows on distinct banks).  The same run holds the plan restated in tests/test_rte_loop_edges.py to the code."""
import json
import os
import shutil
import subprocess

import pytest

import test_rte_loop_edges as edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")
LDS_MAX = 160 * 1024
K2_SORT_MIN_SEGLEN = 16


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_dump") / "plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "plan_dump.cpp"), os.path.join(CSRC, "mwrt_plan.cpp"),
                    "-o", exe], check=True)

    def run(requests):
        r = subprocess.run([exe], input="\n".join("fused %d %d %d %d %d %d" % q for q in requests) + "\n",
                           capture_output=True, text=True, check=True)
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(requests)
        return out
    return run


def lanes(nlev):
    return -(-nlev // 64) * 64


def test_row_stride_covers_every_sorted_segment(ask):
    requests = [(nlev, nf, nang, 0, lds_max, threads)
                for nlev in list(range(2, 300)) + [511, 512, 513, 1023, 1024]
                for nf in (1, 5, 8, 14, 16, 33)
                for nang in (1, 2, 3, 7, 10, 64)
                for lds_max in (LDS_MAX, 48 * 1024)
                for threads in {lanes(nlev), max(lanes(nlev), 256)}]
    sorted_seen = padded = 0
    for q, g in zip(requests, ask(requests)):
        nlev, ld = q[0], g["ldrow"]
        assert ld % 2 == 1 and ld >= nlev + 1, (q, g)
        for nseg, seglen in zip(g["nseg"], g["seglen"]):
            assert nseg * seglen >= nlev - 1 or nlev < 2, (q, g)
            if seglen >= K2_SORT_MIN_SEGLEN:
                sorted_seen += 1
                padded += nseg * seglen > nlev - 1
                assert ld >= nseg * seglen + 1, (q, g)
        assert ld <= max(nlev + 1, max(ns * sl for ns, sl in zip(g["nseg"], g["seglen"])) + 1) + 1, (q, g)     # and no further
    assert sorted_seen > 1000 and padded > 100


def test_the_edge_tests_restate_the_plan(ask):
    cases = sorted({(nlev, nf, nang) for nlev, nf, nang in edges.CASES})
    got = ask([(nlev, nf, nang, 0, LDS_MAX, lanes(nlev)) for nlev, nf, nang in cases])
    for (nlev, nf, nang), g in zip(cases, got):
        passes, ld = edges.plan(nlev, nf, nang)
        assert [(ns, sl) for ns, sl, _ in passes] == list(zip(g["nseg"], g["seglen"]))[:len(passes)] and ld == g["ldrow"], \
            ((nlev, nf, nang), passes, ld, g)
