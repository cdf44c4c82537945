"""The n-form characterisation reference (tests/nform_char_reference.py) against the m-form one
(tests/oe_char_reference.py, Se = diag(se)): two different routes to the same gain, averaging kernel and error budget.

Bar, per profile: nform_reference.TOL + 64 m eps cond(G) -- the sum of the two references' own derived bounds (Cholesky and
its solves on C at cond <= COND_MAX, and on G at the condition number the m-form reference returns), in the units of
``char_errors``."""
import numpy as np
import pytest

import nform_char_reference as ncr
import nform_reference as nfr
import oe_char_reference as ocr
import oe_reference as oer

NPROF = 3


def both(nlev, nblk, m, se_pp, rows=None):
    case = nfr.make_case(nlev, nblk, m, nprof=NPROF, se_per_profile=se_pp, xa_per_profile=True)
    ins = {key: case[key] for key in ("k", "x", "xa", "se", "y", "fx")}
    nf = ncr.nform_char_reference(sa_inv=nfr.sym_inv(case["sa"]), rows=rows, **ins)
    mf = []
    for i in range(NPROF):                                               # the m-form reference takes one Se for the batch
        se_i = case["se"][i] if se_pp else case["se"]
        one = dict(k=[b[i:i + 1] for b in case["k"]], x=case["x"][i:i + 1], xa=case["xa"][i:i + 1], sa=case["sa"], se=se_i,
                   y=case["y"][i:i + 1], fx=case["fx"][i:i + 1])
        mf.append(ocr.oe_char_reference(rows=rows, **one))
    return case, nf, mf


@pytest.mark.parametrize("se_pp", [False, True])
@pytest.mark.parametrize("shape", nfr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_two_forms_agree(shape, se_pp):
    nlev, nblk, m = shape
    case, nf, mf = both(nlev, nblk, m, se_pp)
    sol = nfr.solve_reference(case["k"], case["x"], case["xa"], nfr.sym_inv(case["sa"]), case["se"], case["y"], case["fx"])
    dsa = np.diag(case["sa"]).reshape(nblk, nlev).max(axis=1)
    for i in range(NPROF):
        assert nf["status"][i] == mf[i]["status"][0] == 1
        assert nf["cond"][i] <= nfr.COND_MAX
        bar = nfr.TOL + 64 * m * nfr.EPS * mf[i]["cond"][0]
        got = {key: mf[i][key] for key in ("gain", "avk", "avk_diag", "dfs_block", "noise_var", "smooth_var", "post_cov")}
        err = ncr.char_errors(got, oer.one_profile(nf, i), case)
        print(shape, se_pp, i, err, bar)
        assert set(err) == {"gain", "avk", "avk_diag", "dfs_block", "noise_var", "smooth_var", "post_cov"}
        assert max(err.values()) <= bar, (err, bar)
        assert abs(nf["dfs_block"][i].sum() - sol["dfs"][i]) <= nfr.TOL * max(1.0, abs(sol["dfs"][i]))
        assert (nf["smooth_var"][i] >= -nfr.TOL * dsa[:, None]).all()
        np.testing.assert_array_equal(nf["keep"][i], mf[i]["keep"][0])


def test_a_dropped_row_has_no_gain_and_a_window_is_a_slice():
    nlev, nblk, m = 8, 2, 20
    case = nfr.make_case(nlev, nblk, m, nprof=NPROF)
    case = oer.drop_rows(case, "y", [3], 1)
    case = oer.drop_rows(case, "k", [7], 2)
    ins = {key: case[key] for key in ("k", "x", "xa", "se", "y", "fx")}
    sa_inv = nfr.sym_inv(case["sa"])
    full = ncr.nform_char_reference(sa_inv=sa_inv, **ins)
    assert full["status"].tolist() == [1, 1, 1] and full["nobs"].tolist() == [m, m - 1, m - 1]
    assert (full["gain"][1, 3] == 0.0).all() and (full["gain"][2, 7] == 0.0).all()
    assert np.isfinite(full["gain"]).all() and np.isfinite(full["avk"]).all()
    assert np.count_nonzero((full["gain"] == 0.0).all(axis=2)) == 2
    win = ncr.nform_char_reference(sa_inv=sa_inv, rows=(5, 6), **ins)
    for key in ("avk", "post_cov", "bound_avk"):
        np.testing.assert_array_equal(win[key], full[key][:, 5:11])
    for key in ("gain", "avk_diag", "dfs_block", "noise_var", "smooth_var"):
        np.testing.assert_array_equal(win[key], full[key])
    # the entry on a stored post_cov gives the gain of the solves
    again = ncr.gain_rows(case["k"], case["se"], full["keep"], full["post_cov_full"], full["status"])
    scale = np.abs(full["gain"]).max()
    assert np.abs(again - full["gain"]).max() <= nfr.TOL * scale


def test_the_statuses():
    nlev, nblk, m = 6, 2, 9
    case = nfr.make_case(nlev, nblk, m, nprof=4, se_per_profile=True)
    case = oer.copy_case(case)
    case["x"][0, 0, 1] = np.nan                                          # status 0
    case["se"][1, 4] = -1.0                                              # a kept row's variance <= 0: status 2
    case["y"][2, :] = np.nan                                             # no usable row: status 3
    ins = {key: case[key] for key in ("k", "x", "xa", "se", "y", "fx")}
    sa_inv = nfr.sym_inv(case["sa"])
    out = ncr.nform_char_reference(sa_inv=sa_inv, **ins)
    assert out["status"].tolist() == [0, 2, 3, 1] and out["lin_status"].tolist() == [0, 2, 3, 1]
    for i in (0, 1):
        for key in ("gain", "avk", "avk_diag", "dfs_block", "noise_var", "smooth_var", "post_cov"):
            assert np.isnan(out[key][i]).all(), (i, key)
    for key in ("gain", "avk", "avk_diag", "dfs_block", "noise_var"):
        assert (out[key][2] == 0.0).all(), key
    prior = np.linalg.inv(sa_inv)
    assert np.abs(out["post_cov"][2] - prior).max() <= nfr.TOL * np.abs(prior).max()
    np.testing.assert_array_equal(out["smooth_var"][2].ravel(), np.diag(out["post_cov"][2]))
    assert np.isfinite(out["gain"][3]).all()
    # a C that is not positive definite: status 2 from a good linearisation, 3 stays 3 with NaN in S^ and smooth_var
    bad = -sa_inv
    lin = nfr.prepare_reference(**ins)
    out = ncr.char_linearisation(lin["h"], lin["lin_status"], bad - 2.0 * lin["h"][3], nblk)
    assert out["status"].tolist() == [0, 2, 3, 2]
    assert np.isnan(out["post_cov"][2]).all() and np.isnan(out["smooth_var"][2]).all() and (out["avk"][2] == 0.0).all()
    assert np.isnan(out["avk"][3]).all()
