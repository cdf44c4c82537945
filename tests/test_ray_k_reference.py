"""tests/ray_k_reference.py (the exact derivative reference of the ray-traced K-matrix) against the oracle,
without a GPU:

* its slant paths equal ``lbl_oracle.ray_tracing``'s to 1e-12 relative and its TBs equal
  ``lbl_oracle.tb_cloud_rte(ray_tracing_on=True)``'s at the bar tests/test_tl_oracle.py holds the two oracles to;
* its rows equal central differences of the NumPy oracle (rh +- 1e-4, T +- 0.01 K at fixed rh) at levels 0, 1, 5 and 40,
  at 30, 10.2 and 4.2 degrees and three frequencies, at that file's bar for difference checks (1e-6 of the row's scale);
* the path tangents are there: with every path factor held the level-0 humidity entry at 22.24 GHz and 4.2 degrees is off
  by more than 10 % of the entry (a third, in fact), every level above by less than 2 %;
* the conditioning floor: d ds / d n formed in the oracle's running-sum order and in the device's direct-difference order
  differ by at most FLOOR of a row's largest entry, and the path terms are at most SHARE of their row's largest entry --
  the two numbers tests/test_jacobian_ray.py takes its row bar from."""
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kmatrix_variables_reference as kv  # noqa: E402
import ray_k_reference as rk  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import profiles as pr  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp  # noqa: E402
from oracle import lbl_oracle as lo  # noqa: E402

#: largest row-relative difference of d ds / d n (and d ds / d z) between the two summation orders, measured on the profile
#: below: 2.8e-10 at 60 degrees, 6e-11 at 30, 1.1e-11 at 10.2, 4e-12 at 4.2, 3e-12 at 1 (d ds / d z: below 1e-15)
FLOOR = 3e-10
#: largest ratio of a row's path term to the row's largest entry in the reference, same profile: measured 0.85 in the
#: temperature rows and 0.66 in the humidity rows (rows that are small themselves; 0.33 in the 22.24-GHz row at 4.2 degrees)
SHARE = 0.9
FRQ = np.array([22.24, 31.4, 51.26])
ANG = np.array([30.0, 10.2, 4.2])
TRACE_ANG = (60.0, 30.0, 10.2, 4.2, 1.0)


@pytest.fixture(scope="module")
def case():
    """profiles.synthetic_profiles(3, 73), profile 0, R24: the profile, its reference K-matrix and the frozen-path one."""
    P = pr.synthetic_profiles(3, 73)
    z, p, t, rh = (np.asarray(P[k][0], dtype=np.float64) for k in ("z", "p", "t", "rh"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # (R24 is carried as R20SD tables: said once per process)
        m = sp.get_model("R24")
    K = {k: v.detach().numpy() for k, v in rk.k_matrix_ray_rh(m, z, p, t, rh, FRQ, ANG).items()}
    Kf = {k: v.detach().numpy() for k, v in rk.k_matrix_ray_rh(m, z, p, t, rh, FRQ, ANG, frozen=True).items()}
    return dict(m=m, z=z, p=p, t=t, rh=rh, K=K, Kf=Kf)


def oracle_tb(c, t=None, rh=None):
    return lo.tb_cloud_rte(c["m"], c["z"], c["p"], c["t"] if t is None else t, c["rh"] if rh is None else rh, FRQ, ANG,
                           ray_tracing_on=True)["tbtotal"].reshape(len(ANG), len(FRQ))


def test_paths_and_tbs_equal_the_oracle(case):
    c = case
    n = lo.refractivity(c["p"], c["t"], lo.vapor(c["t"], c["rh"])[0])[2]
    for ang in TRACE_ANG + (90.0, 89.5):
        want = lo.ray_tracing(c["z"] - c["z"][0], n, ang, c["z"][0])
        for order in ("oracle", "direct"):
            ds, trapped = rk.ray_paths(torch.tensor(c["z"]), torch.tensor(n), [ang], order)
            assert not trapped.any()
            assert np.abs(ds[0].numpy() - want).max() <= 1e-12 * np.abs(want).max() and ds[0, 0] == 0.0, (ang, order)
            assert (np.abs(ds[0].numpy()[1:] / want[1:] - 1.0) <= 1e-12).all(), (ang, order)
    ref = oracle_tb(c)
    assert np.abs(c["K"]["tb"] - ref).max() <= 1e-12 * np.abs(ref).max()
    tb = rk.tb_rh(c["m"], c["z"], c["p"], c["t"], c["rh"], FRQ, ANG).numpy()
    assert np.abs(tb - ref).max() <= 1e-12 * np.abs(ref).max()


def test_a_trapped_ray_is_nan_for_its_elevation_only(case):
    c = case
    nlev = 33
    h = np.concatenate([[0.0, 0.1], np.linspace(0.4, 12.0, nlev - 2)])      # a 100-m surface layer
    z, p, t, rh = 0.1 + h, 1013.0 * np.exp(-h / 7.6), 288.0 - 6.0 * h, np.full(nlev, 0.05)
    t[1], rh[0] = t[0] + 8.0, 1.0
    for ang, trapped in ((0.2, True), (0.5, True), (1.0, False), (2.0, False), (4.2, False)):
        if trapped:
            with pytest.raises(ValueError, match="Ducting"):
                lo.tb_cloud_rte(c["m"], z, p, t, rh, FRQ, np.array([ang]), ray_tracing_on=True)
        else:
            lo.tb_cloud_rte(c["m"], z, p, t, rh, FRQ, np.array([ang]), ray_tracing_on=True)
    K = rk.k_matrix_ray_rh(c["m"], z, p, t, rh, FRQ, np.array([90.0, 4.2, 0.5]))
    assert torch.isnan(K["tb"][2]).all() and torch.isnan(K["dtb_dt"][2]).all() and torch.isfinite(K["tb"][:2]).all()
    assert torch.isfinite(K["dtb_dt"][:2]).all() and torch.isfinite(K["dtb_ddz"][:2]).all()


def test_rows_equal_oracle_differences(case):
    c = case
    es, des = kv.es_and_slope(c["t"])
    d_rh = c["K"]["dtb_de"] * es                                          # rh at fixed T
    d_t = c["K"]["dtb_dt"] + c["K"]["dtb_de"] * c["rh"] * des             # T at fixed rh
    for lev in (0, 1, 5, 40):
        for got, key, h in ((d_rh, "rh", 1e-4), (d_t, "t", 0.01)):
            up, dn = c[key].copy(), c[key].copy()
            up[lev] += h
            dn[lev] -= h
            fd = (oracle_tb(c, **{key: up}) - oracle_tb(c, **{key: dn})) / (2 * h)
            scale = np.abs(got).max(axis=-1)
            assert (np.abs(got[:, :, lev] - fd) <= 1e-6 * scale).all(), (lev, key, (np.abs(got[:, :, lev] - fd) / scale).max())


def test_thickness_row_equals_differences_of_the_reference(case):
    c = case
    for lev in (1, 5, 40):
        h = 1e-5
        up, dn = c["z"].copy(), c["z"].copy()
        up[lev:] += h
        dn[lev:] -= h
        fd = (lo.tb_cloud_rte(c["m"], up, c["p"], c["t"], c["rh"], FRQ, ANG, ray_tracing_on=True)["tbtotal"]
              - lo.tb_cloud_rte(c["m"], dn, c["p"], c["t"], c["rh"], FRQ, ANG, ray_tracing_on=True)["tbtotal"]).reshape(3, 3) / (2 * h)
        got = c["K"]["dtb_ddz"]
        assert (np.abs(got[:, :, lev] - fd) <= 1e-6 * np.abs(got).max(axis=-1)).all(), lev
    assert (c["K"]["dtb_ddz"][:, :, 0] == 0.0).all()


def test_path_tangents_are_present(case):
    c = case
    es, _ = kv.es_and_slope(c["t"])
    exact, frozen = c["K"]["dtb_de"][2, 0] * es, c["Kf"]["dtb_de"][2, 0] * es      # 4.2 degrees, 22.24 GHz, per unit rh
    print("d TB(22.24 GHz, 4.2 deg) / d rh at level 0: exact %.4f K, path held %.4f K" % (exact[0], frozen[0]))
    assert abs(exact[0] - frozen[0]) > 0.10 * abs(exact[0])
    assert abs(exact[0] - 1.776) < 2e-3 and abs(frozen[0] - 1.183) < 2e-3          # the oracle's central differences
    assert (np.abs(exact[1:] - frozen[1:]) < 0.02 * np.abs(exact[1:])).all()
    assert np.array_equal(c["K"]["tb"], c["Kf"]["tb"])


def _dds(z, n, ang, order, wrt):
    zt, nt = torch.tensor(z), torch.tensor(n)
    if wrt == "n":
        return torch.autograd.functional.jacobian(lambda x: rk.ray_paths(zt, x, [ang], order)[0][0], nt).numpy()
    dsz = torch.cat([torch.zeros(1, dtype=torch.float64), zt[1:] - zt[:-1]])
    return torch.autograd.functional.jacobian(
        lambda d: rk.ray_paths(zt[0] + torch.cumsum(d, dim=0), nt, [ang], order)[0][0], dsz).numpy()


def test_conditioning_floor_and_share(case):
    c = case
    n = lo.refractivity(c["p"], c["t"], lo.vapor(c["t"], c["rh"])[0])[2]
    worst = {"n": 0.0, "z": 0.0}
    for ang in TRACE_ANG:
        for wrt in ("n", "z"):
            a, b = _dds(c["z"], n, ang, "direct", wrt), _dds(c["z"], n, ang, "oracle", wrt)
            scale = np.abs(b).max(axis=-1, keepdims=True)
            worst[wrt] = max(worst[wrt], float((np.abs(a - b)[1:] / scale[1:]).max()))
    print("largest row-relative difference between the two orders:", worst)
    assert worst["n"] <= FLOOR and worst["z"] <= 1e-14, worst
    share = {row: float((np.abs(c["K"][path]) / np.abs(c["K"][row]).max(axis=-1, keepdims=True)).max())
             for row, path in (("dtb_dt", "path_dt"), ("dtb_de", "path_de"))}
    print("largest path term / largest entry of its row:", share)
    assert 0.25 <= max(share.values()) <= SHARE, share
