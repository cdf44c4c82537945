"""The solves of the optimal-estimation family on the GPU against the 50-digit reference of tests/oe_exact_reference.py, up the
conditioning ladder of that module: cond_2 of what is factored from <= 1e4 to 1e9 .. 1e11.

The bar of an output in a case is max(8 c_out eps cond_case, 64 (m + n) eps) in the family's own unit; c_out is the NumPy
float64 reference's error against the exact one over eps cond, pooled over the family's ladder (oe_exact_reference.pooled,
computed once per session from the two references; nothing in it comes from the device).  Every status is 1 and every
output finite on every rung.  The figures of a run are in profiles/oe_conditioning_errors.json (tools/oe_conditioning_errors.py).

At the singular end (m-form): a profile whose G is exactly singular answers with status 2 and NaN throughout, or with
status 1 and finite numbers throughout, and its neighbours never see it."""
import numpy as np
import pytest

import oe_exact_reference as ex
import oe_reference as oer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _check(family, key, err, label):
    pooled = ex.pooled(family)
    entry = ex.FAMILIES[family][1](key)
    bad = []
    for i in range(ex.NPROF):
        for out, v in err[i].items():
            bar = ex.bar(family, key, out, i)
            print(label, "profile", i, out, "cond %.2e" % entry["cond"][i], "error %.3e" % v, "bar %.3e" % bar,
                  "in eps cond: device %.3g, c_out %.3g" % (v / (ex.EPS * entry["cond"][i]), pooled[out]))
            if not v <= bar:
                bad.append((i, out, v, bar))
    assert not bad, (label, bad)


@pytest.mark.parametrize("key", ex.mform_cases(), ids=ex.case_id)
def test_m_form_up_the_ladder(gpu_ctx, key):
    import oe_conditioning_device as ocd
    err, got = ocd.mform_device_errors(gpu_ctx, key)
    gamma = key[3]
    keys = ex.MFORM_OUT if gamma is None else ("x_new", "chi2")
    assert ocd.finite_and_ok(got, keys), (key, got["status"])
    assert got["nobs"].tolist() == [key[0][2]] * ex.NPROF
    if "gain" in got:
        assert ocd.finite_and_ok(got, ex.GAIN_OUT, status_keys=("gain_status",)) and (got["keep"] == 1).all(), key
        assert set(ex.GAIN_OUT) <= set(err[0])
    _check("mform", key, err, ex.case_id(key))


@pytest.mark.parametrize("key", ex.nform_cases(), ids=ex.case_id)
def test_n_form_up_the_ladder(gpu_ctx, key):
    import oe_conditioning_device as ocd
    err, got = ocd.nform_device_errors(gpu_ctx, key)
    keys = ex.NFORM_OUT if key[2] is None else ("x_new",)
    assert ocd.finite_and_ok(got, keys + ("h", "g", "rwr"), status_keys=("status", "lin_status")), (key, got["status"])
    assert (got["keep"] == 1).all() and got["nobs"].tolist() == [key[0][2]] * ex.NPROF
    _check("nform", key, err, ex.case_id(key))


@pytest.mark.parametrize("key", ex.whiten_cases(), ids=ex.case_id)
def test_whitening_up_the_ladder(gpu_ctx, key):
    import oe_conditioning_device as ocd
    err, got = ocd.whiten_device_errors(gpu_ctx, key)
    assert (got["status"] == 1).all() and (got["keep"] == 1).all(), (key, got["status"])
    assert all(np.isfinite(got[k]).all() for k in ("l", "y_out", "fx_out")) and all(np.isfinite(b).all() for b in got["k_out"])
    _check("whiten", key, err, ex.case_id(key))


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_a_singular_g_is_all_or_nothing(gpu_ctx, se_full):
    """Profile 1 of three has two identical K rows with Se = 0 on both (rows 40 and 41 of m = 65): G is singular exactly."""
    from test_oe_step import OUT_KEYS, run_device
    nlev, nblk, m = 65, 2, 65
    base = oer.make_case(nlev, nblk, m, nprof=3, se_full=se_full)
    case = oer.copy_case(base)
    for b in case["k"]:
        b[1, 41] = b[1, 40]
    # Se is shared, so the two rows lose their noise in every profile; the neighbours' rows differ and their G stays regular
    if se_full:
        case["se"][40:42, :] = 0.0
        case["se"][:, 40:42] = 0.0
    else:
        case["se"][40:42] = 0.0
    got = run_device(gpu_ctx, case)
    floats = ("x_new", "chi2", "dfs", "post_var")
    assert got["status"][1] in (1, 2) and got["nobs"][1] == m
    if got["status"][1] == 2:
        assert all(np.isnan(got[k][1]).all() for k in floats)
    else:
        assert all(np.isfinite(got[k][1]).all() for k in floats)
    # the neighbours: bit for bit what a run without the singular profile gives (same shared Se, profile 1 as seeded)
    alone = dict(case, k=[np.where(np.arange(3)[:, None, None] == 1, bb, b) for b, bb in zip(case["k"], base["k"])])
    ref = run_device(gpu_ctx, alone)
    for i in (0, 2):
        assert ref["status"][i] == 1 and all(np.isfinite(ref[k][i]).all() for k in floats)
        for key in OUT_KEYS:
            assert np.array_equal(got[key][i], ref[key][i]), (i, key)
