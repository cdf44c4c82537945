"""The far-line groups of K1 in the fused kernel (far_groups_accumulate: the far-line sum of a frequency rides across up to
FAR_GROUP_QUADS = 5 quads as a fraction and is divided out once) and the wet sums parked in LDS through dry_absorb, against
the oracle at the project's bars: 1e-6 K on TB (C oracle, every profile) and 1e-9 relative on the zenith layer optical depths
that the all-columns variant writes (Python oracle, one profile).  3 profiles per case.

Frequency lists and tables are chosen by the size of the oxygen far set of their (single) chunk -- tests/far_set_dump.cpp asks
the library's own chunk_masks and the test prints and asserts the counts:

   0 lines   8 channels in 20 MHz at 90 GHz: every line is "very far" and goes through the Taylor set, none through a quad
   3         R98, 74.9 - 75.1 GHz: no quad, a pair and one line for the general loop
   4         R24, 8 channels in 4 MHz at 69 GHz: exactly one quad, a group of one
   5, 7      R24, 74.9 - 75.1 and 44.9 - 45.1 GHz: one quad and the leftovers (one line; a pair and one line)
  12         R24, 8 channels in 4 MHz at 60 GHz, inside the oxygen band (it does not empty the far set: the band's own
             lines beyond 0.25 GHz stay far): three quads, one short group
  20         R24, 53.175 - 53.325 GHz: five quads, exactly one full group
  24         R24, 51.35 - 51.65 GHz: a full group and a group of one quad
  38 / 49    the 14 HATPRO channels at chunk widths 14 and 16 (nine quads = 5 + 4, and a pair) and 8 (a second chunk with all
             49 lines: twelve quads = 5 + 5 + 2); water: 1 far line (no quad)
   9         R24, 895 - 907 GHz: two quads next to the 895-GHz oxygen line -- the largest denominators the tables reach
  49 + 13    one channel at 31.4 GHz: twelve oxygen quads and the only water far set with quads (13 lines: three and one)

Level counts put the layer step's LDS neighbour read on its edges: 64 (one wave), 65 (the second wave holds one level, whose
neighbour is lane 63 of the first), 129 and 180."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
from oracle import c_oracle, lbl_oracle as lo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")
TOL_K = 1e-6
RTOL_TAU = 1e-9
NPROF = 3
ANG = np.array([90.0, 19.2, 4.2])
TABLES = {}                          # kept alive: the context caches device tables per record


def tables_of(name):
    if name not in TABLES:
        TABLES[name] = sp.get_model(name)
    return TABLES[name]


def band(lo_ghz, hi_ghz):
    return np.round(np.linspace(lo_ghz, hi_ghz, 8), 4)


# name -> (tables, frequencies, chunk width (0 = automatic), levels, expected (o2, h2o) far lines of each chunk)
CASES = {
    "empty":        ("R24", band(89.99, 90.01), 8, 64, [(0, 0)]),
    "three":        ("R98", band(74.9, 75.1), 8, 65, [(3, 0)]),
    "one_quad":     ("R24", band(68.998, 69.002), 8, 129, [(4, 0)]),
    "quad_plus_1":  ("R24", band(74.9, 75.1), 8, 64, [(5, 0)]),
    "quad_plus_3":  ("R24", band(44.9, 45.1), 8, 65, [(7, 0)]),
    "band60":       ("R24", band(59.998, 60.002), 8, 180, [(12, 0)]),
    "full_group":   ("R24", band(53.175, 53.325), 8, 129, [(20, 0)]),
    "group_plus_1": ("R24", band(51.35, 51.65), 8, 65, [(24, 0)]),
    "hatpro_8":     ("R24", pr.HATPRO_FRQS, 8, 180, [(38, 1), (49, 13)]),
    "hatpro_14":    ("R24", pr.HATPRO_FRQS, 14, 180, [(38, 1)]),
    "hatpro_16":    ("R98", pr.HATPRO_FRQS, 16, 64, [(33, 1)]),
    "thz":          ("R24", np.array([895.0, 897.0, 899.0, 900.0, 901.0, 903.0, 905.0, 907.0]), 8, 129, [(9, 0)]),
    "one_channel":  ("R24", np.array([31.4]), 8, 180, [(49, 13)]),
}


@pytest.fixture(scope="module")
def far_sets(tmp_path_factory):
    """tests/far_set_dump.cpp + csrc/mwrt_plan.cpp, built with the host C++ compiler: (tables, frq, width) -> [(o2, h2o)]."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("far_set_dump")
    exe = str(tmp / "far_set_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "far_set_dump.cpp"), os.path.join(CSRC, "mwrt_plan.cpp"),
                    "-o", exe], check=True)

    def ask(name, frq, width):
        path = tmp / (name + ".desc")
        if not path.exists():
            path.write_bytes(bytes(tables_of(name).to_c()))
        r = subprocess.run([exe, str(path), str(width)] + [repr(float(f)) for f in frq], capture_output=True, text=True, check=True)
        return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    return ask


def profiles_of(nlev):
    return pr.synthetic_profiles(NPROF, 47, nlev=nlev)


@functools.lru_cache(maxsize=None)
def reference(case):
    """C-oracle TB [NPROF][nang][nf] of every profile and Python-oracle zenith layer depths [nf][nlev] of profile 1."""
    name, frq, _, nlev, _ = CASES[case]
    m, P = tables_of(name), profiles_of(nlev)
    tb, valid = c_oracle.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG)
    assert valid.tolist() == [1] * NPROF
    tau = lo.tb_cloud_rte(m, P["z"][1], P["p"][1], P["t"][1], P["rh"][1], frq, ANG[:1])["taulay"][:, 0, :]
    tb.setflags(write=False); tau.setflags(write=False)
    return tb, tau


@pytest.fixture
def width(gpu_ctx):
    def pin(w):
        gpu_ctx.set_chunk_width(w)
    yield pin
    gpu_ctx.set_chunk_width(0)


@pytest.mark.parametrize("case", list(CASES))
def test_far_set_sizes_against_the_oracle(gpu_ctx, far_sets, width, case):
    name, frq, w, nlev, want = CASES[case]
    got = far_sets(name, frq, w)
    print(f"{case}: {name}, {len(frq)} frequencies, chunk width {w}, {nlev} levels: far lines (o2, h2o) per chunk {got} -> "
          f"o2 quads {[o // 4 for o, _ in got]}, h2o quads {[h // 4 for _, h in got]}")
    assert got == want
    m, P = tables_of(name), profiles_of(nlev)
    ref_tb, ref_tau = reference(case)
    width(w)
    tb, valid = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG)
    tbx, validx, ex = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG, extras=True)
    assert valid.tolist() == [1] * NPROF and validx.tolist() == [1] * NPROF
    d, dx = np.abs(tb - ref_tb).max(), np.abs(tbx - ref_tb).max()
    rel = np.abs(ex["taulay"][1][:, 1:] / ref_tau[:, 1:] - 1).max()
    print(f"{case}: |dTB| {d:.3e} K (TB only), {dx:.3e} K (all columns); layer depths rel {rel:.3e}; "
          f"TB-only against all-columns variant {np.abs(tb - tbx).max():.3e} K")
    assert d <= TOL_K and dx <= TOL_K
    assert np.allclose(ex["taulay"][1], ref_tau, rtol=RTOL_TAU, atol=1e-16)


@pytest.mark.parametrize("case", ["group_plus_1", "hatpro_14"])
def test_nan_profile_leaves_its_neighbours_bits(gpu_ctx, width, case):
    name, frq, w, nlev, _ = CASES[case]
    m, P = tables_of(name), profiles_of(nlev)
    width(w)
    clean, _ = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG)
    Q = {k: v.copy() for k, v in P.items()}
    Q["t"][1, nlev // 2] = np.nan
    tb, valid = gpu_ctx.tb_batch(m, Q["z"], Q["p"], Q["t"], Q["rh"], frq, ANG)
    assert valid.tolist() == [1, 0, 1] and np.isnan(tb[1]).all()
    assert np.array_equal(tb[[0, 2]], clean[[0, 2]])


@pytest.mark.parametrize("nlev", [64, 65, 129, 180])
def test_cloud_in_one_profile_only(gpu_ctx, nlev):
    """The cloud block reuses the rows that hold the parked wet sums: profile 1 carries liquid and ice and is held against the
    C oracle; the cloud-free profiles of the same call equal the clear call bit for bit (the variants share every K1 form)."""
    m, P = tables_of("R24"), profiles_of(nlev)
    frq = pr.HATPRO_FRQS
    dl, di = np.zeros_like(P["z"]), np.zeros_like(P["z"])
    dl[1, nlev // 6: nlev // 4] = 0.3
    di[1, nlev // 3: nlev // 2] = 0.05
    clear, _ = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG)
    tb, valid = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG, denliq=dl, denice=di)
    assert valid.tolist() == [1] * NPROF
    assert np.array_equal(tb[[0, 2]], clear[[0, 2]])
    ref = c_oracle.tb_profile_opt(m, P["z"][1], P["p"][1], P["t"][1], P["rh"][1], frq, ANG, denliq=dl[1], denice=di[1])
    d = np.abs(tb[1].ravel() - ref["tbtotal"]).max()
    print(f"nlev={nlev}: cloudy profile |dTB| {d:.3e} K; cloud moves TB by up to {np.abs(tb[1] - clear[1]).max():.2f} K")
    assert d <= TOL_K and np.abs(tb[1] - clear[1]).max() > 1.0
    zero, _ = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG, denliq=np.zeros_like(dl), denice=np.zeros_like(di))
    assert np.array_equal(zero, clear)
