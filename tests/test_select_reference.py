"""tests/select_reference.py against closed forms, and its inputs against what an order comparison needs: over SHAPES x
profiles (each profile of a case is a seed of its own) x the two variance variants the smallest margin (best - runner-up) /
best of any round is >= MIN_MARGIN = 1e-6, ten thousand times the 1e-9 a device pick may give up and far above the bars on q,
so tests/test_oe_select.py may ask the device for the reference's order exactly."""
import numpy as np
import pytest

import nform_reference as nfr
import select_reference as sr


def test_one_state_element():
    """n = 1: q_i = k_i^2 s / se_i, and after picking j the variance is s se_j / (se_j + k_j^2 s)."""
    k = np.array([[0.5], [2.0], [-1.5], [0.0]])
    se = np.array([0.25, 1.0, 0.5, 0.25])
    s = 3.0
    r = sr.select_reference(k, se, np.array([[s]]), 4, sa_inv=np.array([[1.0 / s]]))
    q0 = k[:, 0] ** 2 * s / se
    assert r["status"] == 1 and r["count"] == 3 and r["order"].tolist() == [2, 1, 0, -1]
    np.testing.assert_allclose(r["q"][0], q0[2], rtol=1e-15)
    s1 = s * se[2] / (se[2] + k[2, 0] ** 2 * s)
    np.testing.assert_allclose(r["q"][1], k[1, 0] ** 2 * s1 / se[1], rtol=1e-15)
    s2 = s1 * se[1] / (se[1] + k[1, 0] ** 2 * s1)
    s3 = s2 * se[0] / (se[0] + k[0, 0] ** 2 * s2)
    np.testing.assert_allclose(float(r["S"][0, 0]), s3, rtol=1e-15)
    # dfs of one element: 1 - s_post / s_prior, gained pick by pick
    np.testing.assert_allclose(r["dfs_gain"].sum(), 1.0 - s3 / s, rtol=1e-14)
    assert r["q"][3] == 0.0 and r["dfs_gain"][3] == 0.0 and r["rank"].tolist() == [2, 1, 0, -1] and r["q_left"][3] == 0.0


def test_orthogonal_rows_on_a_diagonal_prior():
    """Rows along distinct axes never see each other: the order is the sort by k_i^2 s_i / se_i, and every q is its
    initial value."""
    rng = np.random.default_rng(5)
    n = 9
    s = rng.uniform(0.5, 4.0, n)
    amp = rng.uniform(0.2, 2.0, n)
    se = rng.uniform(0.1, 1.0, n)
    perm = rng.permutation(n)
    K = np.zeros((n, n))
    K[np.arange(n), perm] = amp
    r = sr.select_reference(K, se, np.diag(s), n)
    q0 = amp ** 2 * s[perm] / se
    assert r["order"].tolist() == np.argsort(-q0, kind="stable").tolist()
    np.testing.assert_allclose(r["q"], q0[r["order"]], rtol=1e-15)
    np.testing.assert_allclose(r["margin"][:-1], (r["q"][:-1] - r["q"][1:]) / r["q"][:-1], rtol=1e-12)
    assert r["margin"][-1] == 1.0


@pytest.mark.parametrize("nlev,nblk,m", [(8, 1, 20), (12, 2, 40), (33, 1, 16)])
def test_everything_picked_is_the_full_update(nlev, nblk, m):
    """All m picked: the bits add up to log2(det S0 / det S) / 2, the dfs gains to the dfs of nform_reference on the same K,
    and the last S is its posterior."""
    case = sr.make_case(nlev, nblk, m, nprof=2, se_per_profile=True)
    ref = nfr.solve_reference(case["k"], case["x"], case["xa"], case["sa_inv"], case["se"], case["y"], case["fx"])
    for i, r in enumerate(sr.select_batch(case, m)):
        assert r["status"] == 1 and r["count"] == m and sorted(r["order"].tolist()) == list(range(m))
        bits = 0.5 * np.log2(1.0 + r["q"]).sum()
        _, ld0 = np.linalg.slogdet(case["s0"])
        _, ld1 = np.linalg.slogdet(r["S"].astype(np.float64))
        np.testing.assert_allclose(bits, 0.5 * (ld0 - ld1) / np.log(2.0), rtol=1e-10)
        np.testing.assert_allclose(r["dfs_gain"].sum(), ref["dfs"][i], rtol=2 * nfr.TOL, atol=2 * nfr.TOL)
        scale = np.abs(ref["post_cov"][i]).max()
        assert np.abs(r["S"].astype(np.float64) - ref["post_cov"][i]).max() <= 2 * nfr.TOL * scale
        assert (r["q_left"] == r["q"][r["rank"]]).all()


def test_replay_of_the_greedy_order_is_the_greedy_run_and_a_worse_order_shows():
    case, greedy = sr.seeded(8, 1, 20, 20)
    g = greedy[0]
    assert sr.replay(case, 0, g["order"], g) is g
    again = sr.replay(case, 0, g["order"])
    np.testing.assert_array_equal(again["q"], g["q"])
    np.testing.assert_array_equal(again["best"], g["q"])
    swapped = g["order"].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    rep = sr.replay(case, 0, swapped)
    assert rep["q"][0] < rep["best"][0] and rep["best"][0] == g["q"][0]
    # the last S does not depend on the order
    assert np.abs((rep["S"] - g["S"]).astype(np.float64)).max() <= 1e-15 * np.abs(case["s0"]).max()


def test_masks_statuses_and_the_stop():
    case = sr.make_case(8, 1, 6, nprof=1)
    K = case["k"][0][0].copy()
    se = case["se"].copy()
    K[2] = 0.0                                                           # adds nothing: never picked
    K[4, 3] = np.nan                                                     # no candidate
    r = sr.select_reference(K, se, case["s0"], 6, keep=np.array([1, 1, 1, 1, 1, 0]), sa_inv=case["sa_inv"])
    assert r["status"] == 1 and r["count"] == 3 and sorted(r["order"][:3].tolist()) == [0, 1, 3] and (r["order"][3:] == -1).all()
    assert (r["q_left"][[2, 4, 5]] == 0.0).all() and (r["rank"][[2, 4, 5]] == -1).all()
    assert sr.select_reference(K, se, case["s0"], 2, candidate=np.zeros(6))["status"] == 3
    bad = se.copy()
    bad[1] = 0.0
    assert sr.select_reference(K, bad, case["s0"], 2)["status"] == 2
    bad[1] = np.nan                                                      # not a candidate any more
    assert sr.select_reference(K, bad, case["s0"], 2)["status"] == 1
    s0 = case["s0"].copy()
    s0[1, 0] = np.inf
    f = sr.select_reference(K, se, s0, 2)
    assert f["status"] == 0 and np.isnan(f["q"]).all() and np.isnan(f["q_left"]).all() and (f["order"] == -1).all()


def test_the_inputs_are_fit_for_an_order_comparison():
    worst = np.inf
    for shape in sr.SHAPES:
        for se_pp in (False, True):
            _, greedy = sr.seeded(*shape, se_pp)
            for r in greedy:
                assert r["status"] == 1 and r["count"] == shape[3]
                worst = min(worst, np.nanmin(r["margin"]))
    print("smallest margin", worst)
    assert worst >= sr.MIN_MARGIN
