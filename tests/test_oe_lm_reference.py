"""The NumPy reference of the damped step (tests/oe_lm_reference.py) checked against what it is derived from, without a GPU:
the m-form against Rodgers eq. 5.36 as printed (the n-form), gamma = 0 against the undamped reference, the cost along
gamma, and the conditioning every GPU tolerance of test_oe_lm.py rests on."""
import numpy as np
import pytest

import oe_lm_reference as lmr
import oe_reference as oer


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
@pytest.mark.parametrize("nlev,nblk,m", [(3, 3, 14), (33, 1, 17), (64, 2, 15)])
def test_m_form_equals_the_n_form_of_eq_5_36(nlev, nblk, m, se_full):
    case = oer.make_case(nlev, nblk, m, nprof=3, se_full=se_full)
    for gamma in lmr.GAMMAS:
        got = lmr.solve_reference(gamma=gamma, **case)
        assert got["status"].tolist() == [1] * 3
        ref = lmr.n_form_damped(gamma=gamma, **case)
        xa = np.broadcast_to(case["xa"].reshape(-1, nblk * nlev), ref.shape)
        scale = np.abs(ref - xa).max()
        err = np.abs(got["x_new"].reshape(3, -1) - ref).max() / scale
        print(nlev, nblk, m, se_full, gamma, err)
        assert err <= 1e-10, (gamma, err)


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_gamma_zero_is_the_undamped_step(se_full):
    case = oer.make_case(65, 2, 98, nprof=3, se_full=se_full)
    case["y"][1, 7] = np.nan
    got, ref = lmr.solve_reference(gamma=0.0, **case), oer.oe_step_reference(**case)
    assert got["status"].tolist() == ref["status"].tolist() and got["nobs"].tolist() == ref["nobs"].tolist() == [98, 97, 98]
    xa = case["xa"].reshape(1, -1)
    scale = np.abs(ref["x_new"].reshape(3, -1) - xa).max()
    assert np.abs(got["x_new"] - ref["x_new"]).max() <= 1e-12 * scale
    assert np.allclose(got["chi2"], ref["chi2"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("what", ["y", "k"])
@pytest.mark.parametrize("pattern", list(oer.SEAM_DROPS))
def test_seam_patterns_of_dropped_rows_are_the_rows_deleted(what, pattern):
    """The multi-row patterns the GPU suite drops at m = 65 (oe_reference.SEAM_DROPS), against the rows deleted by hand:
    the linearisation's kept rows and columns, and the damped trial of every gamma."""
    nlev, nblk, m = oer.SEAM_SHAPE
    dropped = oer.SEAM_DROPS[pattern]
    case = oer.make_case(nlev, nblk, m, nprof=2)
    bad = oer.drop_rows(case, what, dropped, 1)
    rows = ~np.isin(np.arange(m), dropped)
    cut = dict(case, k=[k[:, rows] for k in case["k"]], y=case["y"][:, rows], fx=case["fx"][:, rows], se=case["se"][rows])
    lin, lin_cut, lin_full = (lmr.prepare_reference(**c) for c in (bad, cut, case))
    assert lin["keep"].tolist() == [[1] * m, rows.astype(int).tolist()]
    assert np.array_equal(lin["g0"][1][np.ix_(rows, rows)], lin_cut["g0"][1]) and np.array_equal(lin["g0"][0], lin_full["g0"][0])
    assert not lin["g0"][1][~rows].any() and not lin["g0"][1][:, ~rows].any() and not lin["r"][1, ~rows].any()
    assert np.array_equal(lin["r"][1, rows], lin_cut["r"][1]) and np.array_equal(lin["kdx"][1, rows], lin_cut["kdx"][1])
    for gamma in lmr.GAMMAS:
        got, want, full = (lmr.solve_reference(gamma=gamma, **c) for c in (bad, cut, case))
        assert got["nobs"].tolist() == [m, m - len(dropped)] and got["status"].tolist() == [1, 1]
        assert got["cond"][1] <= full["cond"][1] * (1 + 1e-9) <= oer.COND_MAX        # a principal submatrix of G_gamma
        assert np.array_equal(got["x_new"][1], want["x_new"][1]) and got["chi2"][1] == want["chi2"][1]
        assert np.array_equal(got["x_new"][0], full["x_new"][0]) and got["chi2"][0] == full["chi2"][0]


def test_cost_of_the_damped_step_falls_as_gamma_falls_on_a_linear_model():
    """On F(x) = F(x0) + K (x - x0) the cost is a quadratic whose minimiser is the gamma = 0 step, and x+(gamma) moves
    monotonically along a path of non-increasing J as gamma -> 0 (the trust-region property of Levenberg-Marquardt)."""
    case = oer.make_case(33, 1, 17, nprof=4)
    sa_inv = np.linalg.inv(case["sa"])
    keep = np.ones((4, 17), dtype=np.uint8)
    k = case["k"][0]
    costs = []
    for gamma in (1e6, 1e3, 4.0, 0.25, 0.0):
        xn = lmr.solve_reference(gamma=gamma, **case)["x_new"]
        fx = case["fx"] + np.einsum("pml,pl->pm", k, (xn - case["x"])[:, 0])
        costs.append(lmr.cost_reference(xn, case["xa"], case["se"], case["y"], fx, keep, sa_inv)["cost"])
    start = lmr.cost_reference(case["x"], case["xa"], case["se"], case["y"], case["fx"], keep, sa_inv)["cost"]
    costs = np.array(costs)
    assert (costs[0] <= start).all()
    assert (np.diff(costs, axis=0) <= 0).all(), costs


def test_dropped_rows_of_the_linearisation_are_deleted_rows():
    case = oer.make_case(3, 3, 14, nprof=3)
    case["fx"][1, 4] = np.nan
    case["k"][2][2, 13, 1] = np.inf
    lin = lmr.prepare_reference(**case)
    assert lin["keep"].sum(axis=1).tolist() == [14, 13, 13] and lin["lin_status"].tolist() == [1, 1, 1]
    assert (lin["g0"][1][4] == 0).all() and (lin["g0"][1][:, 4] == 0).all() and lin["r"][1, 4] == 0 and lin["kdx"][2, 13] == 0
    case["x"][0, 0, 0] = np.nan
    assert lmr.prepare_reference(**case)["lin_status"].tolist() == [0, 1, 1]


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
@pytest.mark.parametrize("nlev,nblk,m", oer.SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in oer.SHAPES])
def test_seeded_cases_meet_the_conditioning_the_tolerance_assumes(nlev, nblk, m, se_full):
    nprof = 3 if nlev >= 180 else 4
    for xa_pp in (False, True):
        case = oer.make_case(nlev, nblk, m, nprof=nprof, se_full=se_full, xa_per_profile=xa_pp)
        for gamma in lmr.GAMMAS:
            out = lmr.solve_reference(gamma=gamma, **case)
            assert (out["status"] == 1).all() and out["cond"].max() <= oer.COND_MAX, (gamma, out["cond"])
    keep = np.ones((nprof, m), dtype=np.uint8)
    c = lmr.cost_reference(case["x"], case["xa"], case["se"], case["y"], case["fx"], keep, np.linalg.inv(case["sa"]))
    assert (c["status"] == 1).all() and c["cond"].max() <= 4.0, c["cond"]
