"""tests/whiten_reference.py against the optimal-estimation references, without a GPU: the caps the bars of the GPU tests
rest on, and the invariance the feature rests on -- the whitened batch through the references with se = ones equals each
profile run alone with its own Se_p (step, damped trial and cost, gain and error budget after un-whitening)."""
import numpy as np
import pytest

import oe_char_reference as ocr
import oe_lm_reference as olr
import oe_reference as oer
import whiten_reference as whr

ALL_SHAPES = sorted(set(whr.SHAPES) | {whr.SEAM_SHAPE})
STEP_SHAPES = [s for s in ALL_SHAPES if s[1] > 0]
_cases = {}


def case(shape):
    if shape not in _cases:
        c = whr.make_case(shape)
        c["wref"] = whr.whiten_reference(c["k"], c["se_p"], c["y"], c["fx"])
        _cases[shape] = c
    return _cases[shape]


def with_drops(c, rows, prof=1):
    bad = oer.drop_rows({k: c[k] for k in ("k", "x", "xa", "sa", "se", "y", "fx")}, "y", rows, prof)
    bad["se_p"] = c["se_p"]
    return bad


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_the_recipe_meets_both_caps(shape):
    c = case(shape)
    w = c["wref"]
    assert (w["status"] == 1).all() and (w["cond"] <= whr.SE_COND_MAX).all(), w["cond"]
    if shape[1] > 0:
        step = oer.oe_step_reference(**{k: v for k, v in whr.whitened_case(c, w).items() if k in
                                        ("k", "x", "xa", "sa", "se", "y", "fx")})
        print(shape, "cond Se_p", w["cond"].max(), "cond G~", step["cond"].max())
        assert (step["status"] == 1).all() and (step["cond"] <= oer.COND_MAX).all(), step["cond"]


def test_the_seam_drops_meet_the_caps():
    c = case(whr.SEAM_SHAPE)
    for name, rows in whr.SEAM_DROPS.items():
        bad = with_drops(c, rows)
        w = whr.whiten_reference(bad["k"], bad["se_p"], bad["y"], bad["fx"])
        assert w["status"][1] == (3 if name == "all" else 1) and np.nanmax(w["cond"]) <= whr.SE_COND_MAX, name
        assert w["keep"][1].sum() == 65 - len(rows) and not w["keep"][1][list(rows)].any()


def _args(c):
    return {k: c[k] for k in ("k", "x", "xa", "sa", "se", "y", "fx")}


def _invariance(c, label):
    w = whr.whiten_reference(c["k"], c["se_p"], c["y"], c["fx"])
    wc = whr.whitened_case(c, w)
    nprof = c["y"].shape[0]
    step = oer.oe_step_reference(**_args(wc))
    char = ocr.oe_char_reference(**_args(wc), products=False)
    gain = whr.apply_reference(w["l"], w["keep"], char["gain"], 1)          # back to d x^ / d y
    sa_inv = np.linalg.inv(c["sa"])
    trial = c["x"] + 0.01
    f_trial = c["fx"] + 0.3
    f_white = whr.apply_reference(w["l"], w["keep"], f_trial, 0)
    cost = olr.cost_reference(trial, c["xa"], wc["se"], wc["y"], f_white, w["keep"], sa_inv)
    solve = olr.solve_reference(**_args(wc), gamma=4.0)
    worst = {}
    for p in range(nprof):
        own = whr.own_case(c, p)
        ref = oer.oe_step_reference(**_args(own))
        assert ref["status"][0] == step["status"][p] and ref["nobs"][0] == step["nobs"][p], (label, p)
        if ref["status"][0] != 1:
            continue
        err = oer.block_errors(oer.one_profile(step, p), ref, own)
        cref = ocr.oe_char_reference(**_args(own), products=False)
        got = {k: (gain if k == "gain" else char[k])[p:p + 1] for k in ("gain", "avk_diag", "dfs_block", "noise_var", "smooth_var")}
        assert np.array_equal(char["keep"][p], cref["keep"][0])
        err.update(ocr.char_errors(got, cref, own))
        sref = olr.solve_reference(**_args(own), gamma=4.0)
        assert sref["status"][0] == solve["status"][p]
        err["lm_x_new"] = oer.block_errors(dict(x_new=solve["x_new"][p:p + 1]), sref, own)["x_new"]
        err["lm_chi2"] = abs(solve["chi2"][p] - sref["chi2"][0]) / max(1.0, abs(sref["chi2"][0]))
        jref = olr.cost_reference(trial[p:p + 1], own["xa"], own["se"], own["y"], f_trial[p:p + 1], cref["keep"], sa_inv)
        err["cost"] = abs(cost["cost"][p] - jref["cost"][0]) / max(1.0, abs(jref["cost"][0]))
        for k, v in err.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(label, worst)
    assert worst and max(worst.values()) <= oer.TOL, (label, worst)


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=str)
def test_the_whitened_batch_is_each_profile_with_its_own_se(shape):
    _invariance(case(shape), shape)


@pytest.mark.parametrize("name", sorted(whr.SEAM_DROPS))
def test_the_invariance_holds_with_rows_dropped(name):
    _invariance(with_drops(case(whr.SEAM_SHAPE), whr.SEAM_DROPS[name]), name)


def test_a_variance_vector_is_its_diagonal_matrix():
    shape = (20, 4, 40)
    c = whr.make_case(shape, se_full=False)
    w = whr.whiten_reference(c["k"], c["se_p"], c["y"], c["fx"])
    full = np.stack([np.diag(v) for v in c["se_p"]])
    w2 = whr.whiten_reference(c["k"], full, c["y"], c["fx"])
    for key in ("l", "y_out", "fx_out"):
        assert np.array_equal(w[key], w2[key])
    assert np.allclose(w["y_out"], c["y"] / np.sqrt(c["se_p"]), rtol=4 * whr.EPS, atol=0)


def test_an_indefinite_se_is_status_2_for_its_profile_alone():
    c = dict(case((3, 3, 5)))
    se = c["se_p"].copy()
    se[2] = -se[2]
    w = whr.whiten_reference(c["k"], se, c["y"], c["fx"])
    assert list(w["status"]) == [1, 1, 2, 1] and np.isnan(w["l"][2]).all() and np.isnan(w["k_out"][0][2]).all()
    assert not w["keep"][2].any() and np.array_equal(w["y_out"][[0, 1, 3]], c["wref"]["y_out"][[0, 1, 3]])
