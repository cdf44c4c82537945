"""The division-free thin step of K2's per-step vote loop (k_tb_fused), against the oracle at the project's bars: 1e-6 K on
TB (tests/test_gpu_parity.py) and rtol 1e-9 on awet / adry (the golden-vector test).  4 profiles, the 14 HATPRO channels.

  level counts   20 (one wave), 65 (a wave seam plus one lane), 180 (the headline's three waves; with seven elevations the
                 only small shape that runs the multi-round per-step vote loop of K2)
  models         R98, R17, R20, R24
  elevations     [90] and BENCH_ELEVATIONS_7; the zenith TB of the two calls agrees to 1e-9 K; one NaN elevation blanks its
                 own rows only
  votes          at 180 levels and 4.2 degrees the K-band rows are thin throughout, 54.94 - 58 GHz thick at all but the top
                 ~30 layers, and 52.28 / 53.86 GHz thick at 6 / 103 of the 179 layers (oracle, profile 0): a wave's steps
                 are voted thin, general, and mixed along one segment

The oracle runs once per (tables, level count) and is shared by the tests that need it."""
import functools

import numpy as np
import pytest

from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, spectroscopy as sp
from oracle import lbl_oracle as lo

pytestmark = pytest.mark.gpu

TOL_K = 1e-6
RTOL_ABS = 1e-9
NPROF = 4
FRQ = pr.HATPRO_FRQS
ANG7 = pr.BENCH_ELEVATIONS_7
CHECKED = (0, 3)                     # profiles held against the oracle


TABLES = {}                          # kept alive: the context caches device tables per record


def tables_of(name):
    if name not in TABLES:
        TABLES[name] = sp.get_model(name)
    return TABLES[name]


def profiles_of(nlev):
    return pr.synthetic_profiles(NPROF, 31, nlev=nlev)


@functools.lru_cache(maxsize=None)
def reference(name, nlev):
    """Oracle TB [7][14] and awet / adry [14][nlev] of the checked profiles."""
    m, P = tables_of(name), profiles_of(nlev)
    out = {}
    for i in CHECKED:
        tb = lo.tb_cloud_rte(m, P["z"][i], P["p"][i], P["t"][i], P["rh"][i], FRQ, ANG7)["tbtotal"].reshape(len(ANG7), len(FRQ))
        aw, ad = lo.absorption_profile(m, P["p"][i], P["t"][i], P["rh"][i], FRQ)
        tb.setflags(write=False); aw.setflags(write=False); ad.setflags(write=False)
        out[i] = (tb, aw, ad)
    return out


def run_case(gpu_ctx, name, nlev):
    m, P = tables_of(name), profiles_of(nlev)
    ref = reference(name, nlev)
    tb7, v7 = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], FRQ, ANG7)
    tb1, v1 = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], FRQ, np.array([90.0]))
    aw, ad = gpu_ctx.absorption_batch(m, P["p"], P["t"], P["rh"], FRQ)
    assert v7.tolist() == [1] * NPROF and v1.tolist() == [1] * NPROF
    for i in CHECKED:
        rtb, raw, rad = ref[i]
        d7, d1 = np.abs(tb7[i] - rtb).max(), np.abs(tb1[i, 0] - rtb[0]).max()
        ew, ed = np.abs(aw[i] / raw - 1).max(), np.abs(ad[i] / rad - 1).max()
        print(f"{name} nlev={nlev} profile {i}: |dTB| 7 elev {d7:.3e} K, zenith {d1:.3e} K; awet rel {ew:.3e}, adry rel {ed:.3e}")
        assert d7 <= TOL_K and d1 <= TOL_K
        assert np.allclose(aw[i], raw, rtol=RTOL_ABS, atol=1e-300) and np.allclose(ad[i], rad, rtol=RTOL_ABS, atol=1e-300)
    dz = np.abs(tb7[:, 0, :] - tb1[:, 0, :]).max()
    print(f"{name} nlev={nlev}: zenith of the 7-elevation call against the 1-elevation call {dz:.3e} K")
    assert dz <= 1e-9
    return P, tb7


@pytest.mark.parametrize("nlev", [20, 65, 180])
@pytest.mark.parametrize("name", ["R98", "R17", "R20", "R24"])
def test_models_and_level_counts(gpu_ctx, name, nlev):
    run_case(gpu_ctx, name, nlev)


@pytest.mark.parametrize("nlev", [20, 65, 180])
def test_nan_elevation_blanks_its_own_rows_only(gpu_ctx, nlev):
    """Rows of the NaN elevation are NaN, valid stays 1.  The other rows are NOT bit for bit those of the clean call, in this
    kernel or in the one before it: the lane of a NaN elevation votes "not thin" at every step (and counts as thin where
    the items are sorted), so lanes that share its wave take the other, algebraically equal form of the layer step.  They
    are held to the 1e-10 K that include/mwrt.h documents for a TB's dependence on its elevation-mates."""
    m, P = tables_of("R24"), profiles_of(nlev)
    clean, _ = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], FRQ, ANG7)
    for bad in (0, 3, 6):
        a = ANG7.copy(); a[bad] = np.nan
        keep = np.arange(len(a)) != bad
        tb, valid = gpu_ctx.tb_batch(m, P["z"], P["p"], P["t"], P["rh"], FRQ, a)
        assert valid.tolist() == [1] * NPROF
        assert np.isnan(tb[:, bad, :]).all() and not np.isnan(tb[:, keep, :]).any()
        d = np.abs(tb[:, keep, :] - clean[:, keep, :]).max()
        print(f"nlev={nlev} NaN elevation {bad}: other rows moved by {d:.3e} K")
        assert d <= 1e-10
