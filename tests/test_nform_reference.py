"""tests/nform_reference.py held against the m-form references, without a GPU: at gamma = 0 against
oe_reference.oe_step_reference (whose NumPy m-form has no m limit) at every shape, at gamma > 0 against
oe_lm_reference.solve_reference, dropped rows against rows deleted by hand, and the statuses.  The bar is nform_reference.TOL
in the units of nform_reference.solve_errors / oe_reference.block_errors; COND_MAX is asserted on the Jacobi-scaled C of
every case and profile."""
import numpy as np
import pytest

import nform_reference as nfr
import oe_lm_reference as lmr
import oe_reference as oer

IDS = [f"{a}-{b}-{c}" for a, b, c in nfr.SHAPES]
KEYS = ("k", "x", "xa", "se", "y", "fx")


def inputs(case):
    return dict({key: case[key] for key in KEYS}, sa_inv=nfr.sym_inv(case["sa"]))


def test_the_bar_is_what_the_docstring_derives():
    assert nfr.TOL == 64 * 128 * np.finfo(np.float64).eps * 1e4 and 1.8e-8 < nfr.TOL < 1.9e-8
    assert all(nlev * nblk <= 128 for nlev, nblk, _ in nfr.SHAPES)


@pytest.mark.parametrize("nlev,nblk,m", nfr.SHAPES, ids=IDS)
@pytest.mark.parametrize("xa_pp", [False, True], ids=["shared", "perprofile"])
def test_n_form_equals_the_m_form_step(nlev, nblk, m, xa_pp):
    case = nfr.make_case(nlev, nblk, m, nprof=3, xa_per_profile=xa_pp)
    ref = oer.oe_step_reference(**{key: case[key] for key in ("k", "x", "xa", "sa", "se", "y", "fx")})
    got = nfr.solve_reference(**inputs(case))
    assert got["status"].tolist() == ref["status"].tolist() == [1] * 3 and got["nobs"].tolist() == ref["nobs"].tolist()
    assert np.nanmax(got["cond"]) <= nfr.COND_MAX, got["cond"]
    err = oer.block_errors(got, ref, case)
    print((nlev, nblk, m), "cond", float(got["cond"].max()), err)
    assert max(err.values()) <= nfr.TOL, err
    # the posterior covariance: symmetric, its diagonal post_var
    for i in range(3):
        assert np.array_equal(got["post_cov"][i], got["post_cov"][i].T)
        assert np.array_equal(np.diag(got["post_cov"][i]), got["post_var"][i].reshape(-1))


@pytest.mark.parametrize("nlev,nblk,m", nfr.SHAPES, ids=IDS)
def test_damped_n_form_equals_the_damped_m_form(nlev, nblk, m):
    case = nfr.make_case(nlev, nblk, m, nprof=3, xa_per_profile=True)
    gamma = np.array(nfr.GAMMAS)
    ref = lmr.solve_reference(gamma=gamma, **{key: case[key] for key in ("k", "x", "xa", "sa", "se", "y", "fx")})
    got = nfr.solve_reference(gamma=gamma, **inputs(case))
    assert got["status"].tolist() == ref["status"].tolist() == [1] * 3 and np.nanmax(got["cond"]) <= nfr.COND_MAX
    assert np.isnan(got["chi2"]).all() and np.isnan(got["post_cov"]).all()       # defined at gamma = 0 only
    err = oer.block_errors(dict(x_new=got["x_new"]), ref, case)
    assert err["x_new"] <= nfr.TOL, err


@pytest.mark.parametrize("nlev,nblk,m", [(8, 1, 98), (43, 2, 154), (32, 4, 98)], ids=["8-1-98", "43-2-154", "32-4-98"])
def test_the_solve_on_a_stored_linearisation_equals_the_solve_from_the_inputs(nlev, nblk, m):
    """solve_linearisation forms chi2 by the header's formula, without K: held against the residual form to its bar."""
    case = nfr.make_case(nlev, nblk, m, nprof=3, se_per_profile=True)
    lin = nfr.prepare_reference(**{key: case[key] for key in KEYS})
    packed = np.array([nfr.tri_pack(h) for h in lin["h"]])
    for gamma in (None, np.array(nfr.GAMMAS)):
        ref = nfr.solve_reference(gamma=gamma, **inputs(case))
        got = nfr.solve_linearisation(packed, lin["g"], lin["rwr"], lin["lin_status"], case["x"], case["xa"], nfr.sym_inv(case["sa"]), gamma)
        assert got["status"].tolist() == ref["status"].tolist() == [1] * 3
        keys = ("x_new", "chi2", "dfs", "post_var", "post_cov") if gamma is None else ("x_new",)
        err = nfr.solve_errors({key: got[key].reshape(ref[key].shape) for key in keys}, ref, case)
        assert max(err.values()) <= nfr.TOL, err
        if gamma is not None:
            assert np.isnan(got["chi2"]).all() and np.isnan(got["post_cov"]).all()


def test_per_profile_variances_equal_one_profile_at_a_time():
    nlev, nblk, m = 43, 2, 154
    case = nfr.make_case(nlev, nblk, m, nprof=3, se_per_profile=True)
    assert case["se"].shape == (3, m) and not np.array_equal(case["se"][0], case["se"][1])
    got = nfr.solve_reference(**inputs(case))
    for i in range(3):
        one = dict(case, k=[b[i:i + 1] for b in case["k"]], x=case["x"][i:i + 1], y=case["y"][i:i + 1],
                   fx=case["fx"][i:i + 1], se=case["se"][i])
        ref = oer.oe_step_reference(**{key: one[key] for key in ("k", "x", "xa", "sa", "se", "y", "fx")})
        err = oer.block_errors(oer.one_profile(got, i), ref, one)
        assert max(err.values()) <= nfr.TOL, (i, err)


@pytest.mark.parametrize("what", ["y", "fx", "k", "se-inf", "se-nan"])
def test_dropped_rows_equal_rows_deleted(what):
    nlev, nblk, m = 32, 1, 98
    base = nfr.make_case(nlev, nblk, m, nprof=2, se_per_profile=True)
    for rows in ((0,), (m - 1,), (15, 16), tuple(range(1, m))):          # a chunk seam; all but one
        case = oer.copy_case(base)
        for row in rows:
            if what == "k":
                case["k"][0][1, row, (7 * row) % nlev] = np.nan
            elif what.startswith("se"):
                case["se"][1, row] = np.inf if what == "se-inf" else np.nan
            else:
                case[what][1, row] = np.nan
        got = nfr.solve_reference(**inputs(case))
        lin = nfr.prepare_reference(**{key: case[key] for key in KEYS})
        kept = np.setdiff1d(np.arange(m), rows)
        assert lin["keep"][1].tolist() == [int(i in kept) for i in range(m)] and lin["nobs"].tolist() == [m, m - len(rows)]
        cut = dict(base, k=[b[1:2, kept] for b in base["k"]], x=base["x"][1:2], y=base["y"][1:2, kept], fx=base["fx"][1:2, kept],
                   se=base["se"][1:2, kept])
        ref = nfr.solve_reference(**inputs(cut))
        err = nfr.solve_errors(oer.one_profile(got, 1), ref, cut)
        assert ref["status"].tolist() == [1] and ref["cond"][0] <= nfr.COND_MAX and max(err.values()) <= nfr.TOL, (what, rows, err)
        cost = nfr.cost_reference(case["x"], case["xa"], nfr.sym_inv(case["sa"]), case["se"], case["y"], case["fx"], lin["keep"])
        cost_cut = nfr.cost_reference(cut["x"], cut["xa"], nfr.sym_inv(case["sa"]), cut["se"], cut["y"], cut["fx"], np.ones((1, len(kept))))
        assert np.isfinite(cost["cost"]).all() and np.isclose(cost["cost"][1], cost_cut["cost"][0], rtol=1e-13, atol=0)


def test_statuses():
    nlev, nblk, m, nprof = 16, 2, 20, 6
    case = nfr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=True, xa_per_profile=True)
    case["x"][1, 0, 3] = np.nan                                      # 0: the state
    case["xa"][2, 1, 5] = np.inf                                     # 0: the prior state
    case["se"][3, 7] = -0.25                                         # 2: a kept row's variance
    case["y"][4] = np.nan                                            # 3: no usable row
    lin = nfr.prepare_reference(**{key: case[key] for key in KEYS})
    assert lin["lin_status"].tolist() == [1, 0, 0, 2, 3, 1] and lin["nobs"].tolist() == [m, 0, 0, m, 0, m]
    assert np.isnan(lin["h"][[1, 2, 3]]).all() and np.isnan(lin["rwr"][[1, 2, 3]]).all() and not lin["keep"][[1, 2, 4]].any()
    assert lin["keep"][3].all() and not lin["h"][4].any() and not lin["g"][4].any() and lin["rwr"][4] == 0.0
    got = nfr.solve_reference(**inputs(case))
    assert got["status"].tolist() == [1, 0, 0, 2, 3, 1]
    assert np.isnan(got["x_new"][[1, 2, 3]]).all() and np.array_equal(got["x_new"][4], case["xa"][4])
    assert got["chi2"][4] == 0.0 and got["dfs"][4] == 0.0
    assert np.allclose(got["post_cov"][4], case["sa"], rtol=1e-9, atol=1e-12)
    gamma = np.array([0.5, 0.5, 0.5, 0.5, 1.0, -1.0])
    got = nfr.solve_reference(gamma=gamma, **inputs(case))
    assert got["status"].tolist() == [1, 0, 0, 2, 3, 2]
    assert np.allclose(got["x_new"][4], case["xa"][4] + 0.5 * (case["x"][4] - case["xa"][4]), rtol=1e-15, atol=0)
    cost = nfr.cost_reference(case["x"], case["xa"], nfr.sym_inv(case["sa"]), case["se"], case["y"], case["fx"], lin["keep"])
    assert np.isposinf(cost["cost"][[1, 2]]).all() and cost["status"].tolist() == [1, 1, 1, 2, 1, 1]
    assert cost["obs"][4] == 0.0 and cost["cost"][4] == cost["prior"][4] > 0.0
