"""K1 line set-ups of the fused kernel after the moves of wave-uniform values were taken out: the oxygen set-up hands the
offsets of its three table polynomials (Y, the second-order shift and strength factors) to the vector side with one move
each and asks for four fields of its line record in one scalar load at its top, and a later quad of a far-line group updates
the group's numerators in place (csrc/mwrt_absorption.hip.h: table_addend, fma_in_place).  None of this changes an operand
or an operation, so the bars are the ones of tests/test_far_line_groups.py: 1e-6 K on TB against the C oracle, every profile of
every case.

The cases are the smallest at which the set-ups and the group loop take another path:

  levels       2 (fewer lanes than table lines), 64, 65 (wave seam), 180 (the headline), 300 (the 512-thread instantiation)
               and 600 with 2 profiles (the 1024-thread instantiation, which keeps the quad form)
  frequencies  1 and 8 (chunk 8), 14, 16 and 17 (two chunks), 6 (under VF_MIN_FREQS = 7: no Taylor sets), and two lists that
               sit on line centres, so the near loops of both species run
  tables       every shipped model at 65 levels (they differ in line counts, mixing order and shift modes)
  groups       oxygen far sets of 4, 12, 16, 20 and 38 lines: groups of 1, 3, 4, 5 and 5 + 4 quads (the counts are asked
               from the library's own chunk_masks, as in tests/test_far_line_groups.py)
  exits        a NaN level in one profile of three; a table whose wet continuum is negative, with one dry profile that
               does not trip it; one call with cloud (the OPT variant, whose cloud block reuses the rows)

3 profiles per case (2 at 600 levels); the references are computed once per case and shared."""
import dataclasses
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
from oracle import c_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mwr_fast_forward_operators_and_lbls_amd", "csrc")
TOL_K = 1e-6                          # tests/test_far_line_groups.py
ANG = np.array([90.0, 19.2, 4.2])
TABLES = {}                           # kept alive: the context caches device tables per record


def tables_of(name):
    if name not in TABLES:
        TABLES[name] = sp.get_model(name)
    return TABLES[name]


def band(lo_ghz, hi_ghz):
    return np.round(np.linspace(lo_ghz, hi_ghz, 8), 4)


@functools.lru_cache(maxsize=None)
def profiles_of(nlev, nprof=3):
    """Synthetic profiles; under 20 levels (the generator's floor) every (64 // nlev)-th level of a 64-level set."""
    if nlev >= 20:
        P = pr.synthetic_profiles(nprof, 53, nlev=nlev)
    else:
        Q = pr.synthetic_profiles(nprof, 53, nlev=64)
        idx = np.arange(nlev) * (64 // nlev)
        P = {k: np.ascontiguousarray(v[:, idx]) for k, v in Q.items()}
    for v in P.values():
        v.setflags(write=False)
    return P


HATPRO = pr.HATPRO_FRQS
F16 = np.concatenate([HATPRO, [90.0, 150.0]])
F17 = np.concatenate([HATPRO, [90.0, 150.0, 183.31]])
# R24 oxygen lines 9-, 3+, 7+, 5+ and the 118.75-GHz line, water 22.2351 and 183.3101: the near loops run for all of them
CENTRES6 = np.array([22.2351, 56.2648, 58.4466, 60.3061, 118.7503, 183.3101])
CENTRES8 = np.array([22.2351, 56.2648, 58.4466, 59.1642, 60.3061, 62.4863, 118.7503, 183.3101])

# name -> (tables, frequencies, chunk width (0 = automatic), levels, profiles)
SHAPES = {
    "lev2_nf1":     ("R24", np.array([31.4]), 0, 2, 3),
    "lev2_nf14":    ("R24", HATPRO, 0, 2, 3),
    "lev64_nf8":    ("R24", HATPRO[:8], 8, 64, 3),
    "lev65_nf16":   ("R24", F16, 0, 65, 3),
    "lev65_nf17":   ("R24", F17, 0, 65, 3),
    "lev65_nf14_8": ("R24", HATPRO, 8, 65, 3),
    "lev180_nf14":  ("R24", HATPRO, 0, 180, 3),
    "lev300_nf14":  ("R24", HATPRO, 0, 300, 3),
    "lev600_nf14":  ("R24", HATPRO, 0, 600, 2),
    "six_freqs":    ("R24", HATPRO[:6], 0, 65, 3),
    "centres6":     ("R24", CENTRES6, 0, 65, 3),
    "centres8":     ("R24", CENTRES8, 0, 180, 3),
}
SHAPES.update({"model_" + name: (name, HATPRO, 0, 65, 3) for name in sp.implemented_models()})

# name -> (frequencies, levels, oxygen far lines of the single chunk of width 8)
GROUPS = {
    "one_quad":    (band(68.998, 69.002), 65, 4),
    "three_quads": (band(59.998, 60.002), 64, 12),
    "four_quads":  (band(51.05, 51.2), 65, 16),
    "five_quads":  (band(53.175, 53.325), 64, 20),
}
SHAPES.update({"group_" + k: ("R24", f, 8, nlev, 3) for k, (f, nlev, _) in GROUPS.items()})


@functools.lru_cache(maxsize=None)
def reference(case):
    name, frq, _, nlev, nprof = SHAPES[case]
    P = profiles_of(nlev, nprof)
    tb, valid = c_oracle.tb_batch(tables_of(name), P["z"], P["p"], P["t"], P["rh"], frq, ANG)
    assert valid.tolist() == [1] * nprof
    tb.setflags(write=False)
    return tb


@pytest.fixture
def width(gpu_ctx):
    def pin(w):
        gpu_ctx.set_chunk_width(w)
    yield pin
    gpu_ctx.set_chunk_width(0)


@pytest.mark.parametrize("case", list(SHAPES))
def test_tb_against_the_oracle(gpu_ctx, width, case):
    name, frq, w, nlev, nprof = SHAPES[case]
    P = profiles_of(nlev, nprof)
    ref = reference(case)
    width(w)
    tb, valid = gpu_ctx.tb_batch(tables_of(name), P["z"], P["p"], P["t"], P["rh"], frq, ANG)
    d = np.abs(tb - ref).max()
    print(f"{case}: {name}, {len(frq)} frequencies, chunk width {w}, {nlev} levels, {nprof} profiles: |dTB| {d:.3e} K")
    assert valid.tolist() == [1] * nprof
    assert d <= TOL_K


def test_group_lengths_are_the_intended_ones(tmp_path):
    """The far-set sizes behind the group_* cases, from the library's own chunk_masks (tests/far_set_dump.cpp): 4, 12, 16 and
    20 lines are groups of 1, 3, 4 and 5 quads; the HATPRO chunk of width 14 holds 38 (nine quads, 5 + 4, and a pair)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "far_set_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "far_set_dump.cpp"), os.path.join(CSRC, "mwrt_plan.cpp"),
                    "-o", exe], check=True)
    desc = tmp_path / "R24.desc"
    desc.write_bytes(bytes(tables_of("R24").to_c()))

    def o2_far(frq, w):
        r = subprocess.run([exe, str(desc), str(w)] + [repr(float(f)) for f in frq], capture_output=True, text=True, check=True)
        return [int(line.split()[0]) for line in r.stdout.splitlines()]
    for k, (frq, _, want) in GROUPS.items():
        got = o2_far(frq, 8)
        print(f"{k}: oxygen far lines {got}")
        assert got == [want]
    assert o2_far(HATPRO, 14) == [38]


@pytest.mark.parametrize("case", ["lev2_nf14", "lev65_nf17", "lev180_nf14"])
def test_nan_level_blanks_its_profile_only(gpu_ctx, width, case):
    """The NaN exit leaves the workgroup before K1: the other profiles of the call keep the oracle's values."""
    name, frq, w, nlev, nprof = SHAPES[case]
    P = profiles_of(nlev, nprof)
    ref = reference(case)
    Q = {k: v.copy() for k, v in P.items()}
    Q["t"][1, nlev // 2] = np.nan
    width(w)
    tb, valid = gpu_ctx.tb_batch(tables_of(name), Q["z"], Q["p"], Q["t"], Q["rh"], frq, ANG)
    assert valid.tolist() == [1, 0, 1] and np.isnan(tb[1]).all()
    d = np.abs(tb[[0, 2]] - ref[[0, 2]]).max()
    print(f"{case}: neighbours of the NaN profile |dTB| {d:.3e} K")
    assert d <= TOL_K


@pytest.mark.parametrize("nlev", [40, 65])
def test_negative_absorption_in_some_profiles(gpu_ctx, nlev):
    """A table with a negative foreign continuum trips the negative-absorption exit wherever there is vapour; a profile without
    any (rh = 0: the wet term is zero) passes, in the same call, and equals the oracle."""
    bad = dataclasses.replace(tables_of("R98"), name=f"R98_negcont_k1_{nlev}", h2o_cf=-1e-6)
    P = {k: v.copy() for k, v in profiles_of(nlev).items()}
    P["rh"][1] = 0.0
    ref, ref_valid = c_oracle.tb_batch(bad, P["z"], P["p"], P["t"], P["rh"], HATPRO, ANG)
    tb, valid = gpu_ctx.tb_batch(bad, P["z"], P["p"], P["t"], P["rh"], HATPRO, ANG)
    print(f"nlev={nlev}: valid {valid.tolist()} (oracle {ref_valid.tolist()}); dry profile |dTB| {np.abs(tb[1] - ref[1]).max():.3e} K")
    assert valid.tolist() == [2, 1, 2] and ref_valid.tolist() == [2, 1, 2]
    assert np.isnan(tb[[0, 2]]).all()
    assert np.abs(tb[1] - ref[1]).max() <= TOL_K


def test_cloud_call_reuses_the_rows(gpu_ctx):
    """One call of the OPT variant with liquid and ice in profile 1: its cloud block writes the rows that held the parked wet
    sums.  The cloudy profile against the C oracle; the cloud-free ones against the clear-sky reference."""
    case = "lev65_nf17"
    name, frq, _, nlev, nprof = SHAPES[case]
    m, P = tables_of(name), profiles_of(nlev, nprof)
    dl, di = np.zeros_like(P["z"]), np.zeros_like(P["z"])
    dl[1, nlev // 6: nlev // 4] = 0.3
    di[1, nlev // 3: nlev // 2] = 0.05
    tb, valid = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], frq, ANG, denliq=dl, denice=di)
    assert valid.tolist() == [1] * nprof
    ref = c_oracle.tb_profile_opt(m, P["z"][1], P["p"][1], P["t"][1], P["rh"][1], frq, ANG, denliq=dl[1], denice=di[1])
    d_cloud = np.abs(tb[1].ravel() - ref["tbtotal"]).max()
    d_clear = np.abs(tb[[0, 2]] - reference(case)[[0, 2]]).max()
    print(f"cloudy profile |dTB| {d_cloud:.3e} K, cloud-free profiles {d_clear:.3e} K")
    assert d_cloud <= TOL_K and d_clear <= TOL_K
