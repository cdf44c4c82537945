"""The NumPy reference of the characterisation (tests/oe_char_reference.py) held to independent forms, without a GPU: the
m-form gain, averaging kernel and posterior against the n-form's, the error budget against its definitions, the degrees
of freedom against the step's, a dropped row against the rows deleted by hand, and the status conventions."""
import numpy as np
import pytest

import oe_char_reference as ocr
import oe_reference as oer

# the finite cases of test_oe_reference.py's cross-form check
SMALL = [s for s in oer.SHAPES if s[0] <= 180]


def _copy(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else [b.copy() for b in v]) for k, v in case.items()}


@pytest.mark.parametrize("nlev,nblk,m", SMALL, ids=[f"{a}-{b}-{c}" for a, b, c in SMALL])
@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_m_form_products_equal_the_n_form(nlev, nblk, m, se_full):
    nprof = 2
    case = oer.make_case(nlev, nblk, m, nprof=nprof, se_full=se_full)
    ref = ocr.oe_char_reference(**case)
    step = oer.oe_step_reference(**case)
    _, post, _ = oer.n_form_reference(**case)
    assert (ref["status"] == 1).all() and (ref["nobs"] == m).all() and (ref["keep"] == 1).all()
    assert np.nanmax(ref["cond"]) <= oer.COND_MAX
    n = nblk * nlev
    S = case["se"] if se_full else np.diag(case["se"])
    Si = np.linalg.inv(S)
    K = np.concatenate(case["k"], axis=2)
    n_form = dict(gain=np.empty((nprof, m, n)), avk=np.empty((nprof, n, n)), post_cov=post)
    for i in range(nprof):
        n_form["gain"][i] = (post[i] @ K[i].T @ Si).T                    # S^ K^T Se^-1, stored transposed
        n_form["avk"][i] = post[i] @ (K[i].T @ Si @ K[i])
    err = ocr.char_errors(n_form, ref, case)
    print(nlev, nblk, m, "cross-form", err, "cond", ref["cond"].max())
    assert set(err) == {"gain", "avk", "post_cov"} and all(v <= 1e-10 for v in err.values()), err
    # the degrees of freedom per block add up to the step's, the two variances to its post_var
    assert np.abs(ref["dfs_block"].sum(axis=1) - step["dfs"]).max() <= 1e-10 * max(1.0, np.abs(step["dfs"]).max())
    dsa = np.diag(case["sa"]).reshape(nblk, nlev).max(axis=1)[None, :, None]
    assert (np.abs(ref["noise_var"] + ref["smooth_var"] - step["post_var"]) / dsa).max() <= 1e-10
    # ... and the smoothing error is what its definition says, formed explicitly
    for i in range(nprof):
        am = ref["avk"][i] - np.eye(n)
        explicit = np.einsum("jk,kl,jl->j", am, case["sa"], am).reshape(nblk, nlev)
        assert (np.abs(ref["smooth_var"][i] - explicit) / dsa[0]).max() <= 1e-10, i
        noise = np.einsum("ij,ik,kj->j", ref["gain"][i], S, ref["gain"][i]).reshape(nblk, nlev)
        assert (np.abs(ref["noise_var"][i] - noise) / dsa[0]).max() <= 1e-10, i
        assert np.abs(ref["avk_diag"][i].ravel() - np.diag(ref["avk"][i])).max() <= 4 * m * ocr.EPS * ref["bound_diag"][i].max()
        assert np.allclose(ref["bound_diag"][i], np.diag(ref["bound_avk"][i]), rtol=1e-13, atol=0)
    # the product entry's reference on the reference's own gain is the same A and S^
    a, _ = ocr.product_reference(ref["gain"], ref["keep"], K)
    s, _ = ocr.product_reference(ref["gain"], ref["keep"], ref["ksa"], sa=case["sa"])
    assert np.abs(a - ref["avk"]).max() <= 4 * m * ocr.EPS * ref["bound_avk"].max()
    assert np.abs(s - ref["post_cov"]).max() <= 4 * m * ocr.EPS * (np.abs(case["sa"]).max() + ref["bound_cov"].max())


@pytest.mark.parametrize("what", ["y", "fx", "k", "se"])
@pytest.mark.parametrize("row", [0, 8, 16] + list(oer.SEAM_DROPS))
def test_dropped_row_is_the_row_deleted(what, row):
    """One row of the 17-row case, or one of the multi-row patterns of oe_reference.SEAM_DROPS at m = 65."""
    (nlev, nblk, m), dropped = ((33, 2, 17), (row,)) if isinstance(row, int) else (oer.SEAM_SHAPE, oer.SEAM_DROPS[row])
    case = oer.make_case(nlev, nblk, m, nprof=2, se_full=(what == "se"))
    bad = _copy(case)
    for r in dropped:
        if what == "k":
            bad["k"][1][1, r, 5] = np.nan
        elif what == "se":
            bad["se"][r, (r + 3) % m] = np.inf
        else:
            bad[what][1, r] = np.nan
    ref = ocr.oe_char_reference(**bad)
    rows = ~np.isin(np.arange(m), dropped)
    row = list(dropped)
    small = _copy(case)
    small["k"] = [b[:, rows] for b in case["k"]]
    small["y"], small["fx"] = case["y"][:, rows], case["fx"][:, rows]
    small["se"] = case["se"][np.ix_(rows, rows)] if what == "se" else case["se"][rows]
    cut = ocr.oe_char_reference(**small)
    hit = [0, 1] if what == "se" else [1]
    for i in hit:
        assert ref["nobs"][i] == m - len(dropped) and ref["keep"][i].tolist() == rows.astype(int).tolist()
        assert (ref["gain"][i, row] == 0).all() and (ref["ksa"][i, row] == 0).all()
        assert np.array_equal(ref["gain"][i, rows], cut["gain"][i]) and np.array_equal(ref["ksa"][i, rows], cut["ksa"][i])
        for key in ("avk", "post_cov", "avk_diag", "noise_var", "smooth_var", "dfs_block"):
            assert np.array_equal(ref[key][i], cut[key][i]), (key, i)
    if what != "se":                                                     # the neighbour is the clean profile
        clean = ocr.oe_char_reference(**case)
        for key in ("gain", "avk", "post_cov", "dfs_block"):
            assert np.array_equal(ref[key][0], clean[key][0]), key


def test_status_conventions():
    case = oer.make_case(3, 3, 14, nprof=4)
    case["k"][0][0] = np.nan                     # no usable observation
    case["x"][1, 2, 1] = np.nan                  # state not finite
    ref = ocr.oe_char_reference(**case)
    assert ref["status"].tolist() == [3, 0, 1, 1] and ref["nobs"].tolist() == [0, 0, 14, 14]
    assert ref["keep"].sum(axis=1).tolist() == [0, 0, 14, 14]
    for key in ("gain", "ksa", "avk_diag", "noise_var", "dfs_block", "avk"):
        assert (ref[key][0] == 0).all() and np.isnan(ref[key][1]).all(), key
    assert np.array_equal(ref["smooth_var"][0].ravel(), np.diag(case["sa"])) and np.array_equal(ref["post_cov"][0], case["sa"])
    assert np.isnan(ref["smooth_var"][1]).all() and np.isnan(ref["post_cov"][1]).all()
    bad = _copy(case)
    bad["se"][5] = -1e9                          # an indefinite G
    ref = ocr.oe_char_reference(**bad)
    assert ref["status"].tolist() == [3, 0, 2, 2] and ref["nobs"].tolist() == [0, 0, 14, 14]
    assert (ref["keep"][2:] == 0).all()
    for key in ("gain", "ksa", "avk_diag", "noise_var", "smooth_var", "dfs_block", "avk", "post_cov"):
        assert np.isnan(ref[key][2:]).all(), key


def test_row_window_is_the_same_rows():
    case = oer.make_case(33, 2, 17, nprof=2)
    full = ocr.oe_char_reference(**case)
    for rows in ((0, 1), (65, 1), (32, 3), (10, 40)):
        win = ocr.oe_char_reference(**case, rows=rows)
        for key in ("avk", "post_cov", "bound_avk", "bound_cov"):
            assert win[key].shape == (2, rows[1], 66)
            # BLAS may sum a narrower product in another order: equal within the rounding of a length-17 sum
            atol = 4 * 17 * ocr.EPS * (np.abs(case["sa"]).max() + full["bound_cov"].max() + full["bound_avk"].max())
            assert np.abs(win[key] - full[key][:, rows[0]:rows[0] + rows[1]]).max() <= atol, (rows, key)
