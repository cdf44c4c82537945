"""The NumPy reference of the optimal-estimation step (tests/oe_reference.py) held to independent algebra, without a GPU:
the m-form against the n-form, the diagnostics against their definitions, dropped rows against the rows deleted by hand,
and the recipe's conditioning (cond_2(G) <= 1e4 for every shape the GPU tests use -- the premise of their 1e-8 bar)."""
import numpy as np
import pytest

import oe_reference as oer

# the n-form inverts Sa: every shape of the recipe but those of n >= 2048, whose inverses add seconds and no new path
SMALL = [s for s in oer.SHAPES if s[0] <= 180]


@pytest.mark.parametrize("nlev,nblk,m", SMALL, ids=[f"{a}-{b}-{c}" for a, b, c in SMALL])
@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_m_form_equals_n_form(nlev, nblk, m, se_full):
    case = oer.make_case(nlev, nblk, m, nprof=2, se_full=se_full)
    ref = oer.oe_step_reference(**case)
    xn, post, dfs = oer.n_form_reference(**case)
    assert (ref["status"] == 1).all() and (ref["nobs"] == m).all()
    n = nblk * nlev
    xa = np.broadcast_to(case["xa"].reshape(-1, n), (2, n))
    scale = np.abs(xn - xa).max()
    err = np.abs(ref["x_new"].reshape(2, n) - xn).max() / scale
    print(nlev, nblk, m, "cross-form", err, "cond", ref["cond"].max())
    assert err <= 1e-10
    # dfs = tr(Sa K^T G^-1 K) = trace of the n-form averaging kernel; post_var = diagonal of the n-form posterior
    assert np.abs(ref["dfs"] - dfs).max() <= 1e-8 * max(1.0, np.abs(dfs).max())
    pv = np.array([np.diag(p) for p in post])
    assert np.abs(ref["post_var"].reshape(2, n) - pv).max() <= 1e-8 * np.diag(case["sa"]).max()


@pytest.mark.parametrize("nlev,nblk,m", oer.SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in oer.SHAPES])
def test_recipe_is_well_conditioned(nlev, nblk, m):
    for se_full in (False, True):
        case = oer.make_case(nlev, nblk, m, nprof=4, se_full=se_full)
        K = np.concatenate(case["k"], axis=2)
        S = case["se"] if se_full else np.diag(case["se"])
        cond = max(np.linalg.cond(k @ case["sa"] @ k.T + S) for k in K)
        assert cond <= oer.COND_MAX, cond


def test_dfs_is_the_trace_of_the_averaging_kernel():
    case = oer.make_case(33, 2, 17, nprof=2, se_full=True)
    ref = oer.oe_step_reference(**case)
    for i in range(2):
        K = np.concatenate([k[i] for k in case["k"]], axis=1)
        G = K @ case["sa"] @ K.T + case["se"]
        A = case["sa"] @ K.T @ np.linalg.solve(G, K)
        assert abs(np.trace(A) - ref["dfs"][i]) <= 1e-9 * max(1.0, ref["dfs"][i])
        assert 0.0 < ref["dfs"][i] < 17


@pytest.mark.parametrize("what", ["y", "fx", "k", "se"])
@pytest.mark.parametrize("row", [0, 8, 16] + list(oer.SEAM_DROPS))
def test_dropped_row_is_the_row_deleted(what, row):
    """One row of the 17-row case, or one of the multi-row patterns the GPU suites drop at the seams of m = 65
    (oe_reference.SEAM_DROPS: a whole tile, every row but one), against the rows deleted by hand."""
    (nlev, nblk, m), dropped = ((33, 2, 17), (row,)) if isinstance(row, int) else (oer.SEAM_SHAPE, oer.SEAM_DROPS[row])
    case = oer.make_case(nlev, nblk, m, nprof=2, se_full=(what == "se"))
    bad = oer.copy_case(case)
    for r in dropped:
        if what == "k":
            bad["k"][1][0, r, 5] = np.nan
        elif what == "se":
            bad["se"][r, (r + 3) % m] = np.inf
        else:
            bad[what][0, r] = np.nan
    if what in ("y", "k") and not isinstance(row, int):          # the helper the GPU suites use says the same
        via = oer.oe_step_reference(**oer.drop_rows(case, what, dropped, 0))
        assert via["nobs"].tolist() == [m - len(dropped), m]
    got = oer.oe_step_reference(**bad)
    rows = ~np.isin(np.arange(m), dropped)
    cut = dict(case, k=[k[:, rows] for k in case["k"]], y=case["y"][:, rows], fx=case["fx"][:, rows],
               se=case["se"][np.ix_(rows, rows)] if what == "se" else case["se"][rows])
    want = oer.oe_step_reference(**cut)
    full = oer.oe_step_reference(**case)
    assert np.nanmax(got["cond"]) <= np.nanmax(full["cond"]) * (1 + 1e-9) <= oer.COND_MAX   # a principal submatrix of G
    # a non-finite Se entry drops the row for every profile; the others drop it for profile 0 alone
    for i in range(2):
        src = want if (i == 0 or what == "se") else full
        assert got["nobs"][i] == src["nobs"][i] == (m - len(dropped) if src is want else m)
        for key in ("x_new", "post_var", "chi2", "dfs"):
            np.testing.assert_allclose(got[key][i], src[key][i], rtol=0, atol=1e-12 * max(1.0, np.abs(src[key][i]).max()))


def test_status_values():
    case = oer.make_case(3, 3, 14, nprof=4)
    case["k"][0][0] = np.nan                     # no usable observation
    case["x"][1, 2, 1] = np.nan                  # state not finite
    case["se"] = case["se"].copy()
    ref = oer.oe_step_reference(**case)
    assert ref["status"].tolist() == [3, 0, 1, 1]
    assert (ref["x_new"][0] == case["xa"]).all() and ref["chi2"][0] == 0 and ref["dfs"][0] == 0 and ref["nobs"][0] == 0
    assert (ref["post_var"][0].ravel() == np.diag(case["sa"])).all()
    assert np.isnan(ref["x_new"][1]).all() and np.isnan(ref["chi2"][1]) and np.isnan(ref["post_var"][1]).all()
    case["se"][:] = -1e6                         # G indefinite
    assert (oer.oe_step_reference(**case)["status"][2:] == 2).all()
