"""mwrt_oe_nform_prepare_device, mwrt_oe_nform_solve_device and mwrt_oe_nform_cost_device (include/mwrt.h) on
the GPU against tests/nform_reference.py, whose docstring derives the bars: TOL = 64 * 128 * eps * 1e4 = 1.8e-8 for the
solve's outputs in the units of nform_reference.solve_errors (cond <= COND_MAX on the Jacobi-scaled C asserted per case and
profile), 64 m eps for H, g and r^T W r in the units of nform_reference.prepare_errors, 64 (m + n) eps for the cost.  No mask,
no floor.  Shapes are nform_reference.SHAPES; what they reach is asserted by
test_nform_kernel_resources.py::test_the_shapes_keep_both_sides_of_every_edge."""
import numpy as np
import pytest

import nform_reference as nfr
import oe_reference as oer
from mwr_fast_forward_operators_and_lbls_amd import _native
from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nform_device import Dev, _cur, _dev, reference, seeded  # noqa: E402

EPS = np.finfo(np.float64).eps
LIN_KEYS = ("h", "g", "rwr", "keep", "nobs", "lin_status")
SOLVE_KEYS = ("x_new", "status", "chi2", "dfs", "post_var", "post_cov")
COST_KEYS = ("cost", "cost_obs", "cost_prior", "cost_status")


def check_prepare(got, lin, m, label):
    for key in ("keep", "nobs", "lin_status"):
        assert got[key].tolist() == lin[key].tolist(), (label, key)
    err = nfr.prepare_errors(got, lin)
    print(label, "prepare", err)
    assert max(err.values()) <= 64 * m * EPS, (label, err)
    for i in np.flatnonzero(lin["lin_status"] == 3):
        assert not got["h"][i].any() and not got["g"][i].any() and got["rwr"][i] == 0.0, label
    for i in np.flatnonzero((lin["lin_status"] == 0) | (lin["lin_status"] == 2)):
        assert np.isnan(got["h"][i]).all() and np.isnan(got["g"][i]).all() and np.isnan(got["rwr"][i]), label


def check_solve(got, sol, case, label, diagnostics):
    assert got["status"].tolist() == sol["status"].tolist(), label
    ok = sol["status"] == 1
    assert ok.any() and sol["cond"][ok].max() <= nfr.COND_MAX, (label, sol["cond"])
    keys = ("x_new", "chi2", "dfs", "post_var", "post_cov") if diagnostics else ("x_new",)
    err = nfr.solve_errors({key: got[key] for key in keys}, sol, case)
    print(label, "solve", err)
    for key in keys:
        assert np.isfinite(got[key][ok]).all(), (label, key)
    assert max(err.values()) <= nfr.TOL, (label, err)
    bad = (sol["status"] == 0) | (sol["status"] == 2)
    for key in keys:
        assert np.isnan(got[key][bad]).all(), (label, key)
    if diagnostics:
        for i in np.flatnonzero(ok):
            assert np.array_equal(got["post_cov"][i], got["post_cov"][i].T), label
            assert np.array_equal(np.diag(got["post_cov"][i]), got["post_var"][i].reshape(-1)), label


def check_cost(got, cost, m, n, label):
    assert got["cost_status"].tolist() == cost["status"].tolist(), label
    fin = np.isfinite(cost["cost"])
    bar = 64 * (m + n) * EPS * cost["scale"][fin]
    for key, ref in (("cost", "cost"), ("cost_obs", "obs"), ("cost_prior", "prior")):
        e = np.abs(got[key][fin] - cost[ref][fin])
        assert (e <= bar).all(), (label, key, float((e / bar).max()))
        assert np.array_equal(got[key][~fin], cost[ref][~fin], equal_nan=True), (label, key)
    assert np.array_equal(got["cost"][fin], got["cost_obs"][fin] + got["cost_prior"][fin]), label


@pytest.mark.parametrize("nlev,nblk,m", nfr.SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in nfr.SHAPES])
@pytest.mark.parametrize("se_pp,xa_pp", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["shared-shared", "seperprofile-shared", "shared-xaperprofile", "perprofile-perprofile"])
def test_prepare_solve_and_cost_against_the_reference(gpu_ctx, nlev, nblk, m, se_pp, xa_pp):
    nprof = 4
    case, gamma, (lin, sol, cost), (_, damped, _) = seeded(nlev, nblk, m, se_pp, xa_pp, nprof)
    label = (nlev, nblk, m, se_pp, xa_pp)
    assert lin["lin_status"].tolist() == [1] * nprof and sol["status"].tolist() == [1] * nprof
    d = Dev(case)
    got = d.run(gpu_ctx)                                                 # gamma = 0 as a NULL pointer, every optional output
    check_prepare(got, lin, m, label)
    check_solve(got, sol, case, label, True)
    check_cost(got, cost, m, nblk * nlev, label)
    d.reset()
    again = d.run(gpu_ctx, gamma=gamma)                                  # gamma = (0, 0.5, 1e3, 0) across the profiles
    check_solve(again, damped, case, label + (tuple(gamma),), False)
    for key in ("chi2", "dfs", "post_var", "post_cov"):
        assert (again[key] == -7.0).all(), key                           # not asked for: not touched
    zero = np.flatnonzero(gamma == 0.0)
    assert np.array_equal(again["x_new"][zero], got["x_new"][zero])      # gamma = 0 given is gamma = 0 by default


def test_x_new_does_not_depend_on_the_optional_outputs(gpu_ctx):
    for shape in ((32, 1, 98), (43, 2, 154), (128, 1, 513)):
        case = seeded(*shape, True, False, 4)[0]
        full = Dev(case).run(gpu_ctx)
        bare = Dev(case).run(gpu_ctx, optional=False)
        assert np.array_equal(full["x_new"], bare["x_new"]) and np.array_equal(full["status"], bare["status"])
        assert (bare["chi2"] == -7.0).all() and (bare["post_cov"] == -7.0).all()


@pytest.mark.parametrize("what", ["y", "fx", "k", "se-inf", "se-nan"])
def test_dropped_rows_equal_rows_deleted(gpu_ctx, what):
    """Profile 1 loses the first row, the last, the two rows at a chunk seam (15 | 16) and every row but one."""
    nlev, nblk, m, nprof = 32, 1, 98, 4
    base = seeded(nlev, nblk, m, True, False, nprof)[0]
    clean = Dev(base).run(gpu_ctx)
    for rows in ((0,), (m - 1,), (15, 16), tuple(range(1, m))):
        case = oer.copy_case(base)
        for row in rows:
            if what == "k":
                case["k"][0][1, row, (7 * row) % nlev] = np.nan
            elif what.startswith("se"):
                case["se"][1, row] = np.inf if what == "se-inf" else np.nan
            else:
                case[what][1, row] = np.nan
        lin, sol, cost = reference(case)
        assert sol["nobs"].tolist() == [m, m - len(rows), m, m] and sol["status"].tolist() == [1] * nprof
        got = Dev(case).run(gpu_ctx)
        label = (what, rows[:3])
        check_prepare(got, lin, m, label)
        check_solve(got, sol, case, label, True)
        check_cost(got, cost, m, nlev * nblk, label)
        for i in (0, 2, 3):                                              # the neighbours never see it: bit for bit
            for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
                assert np.array_equal(got[key][i], clean[key][i]), (what, rows[:3], i, key)


def test_status_values_and_untouched_neighbours(gpu_ctx):
    nlev, nblk, m, nprof = 16, 2, 20, 7
    base = nfr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=True, xa_per_profile=True)
    clean = Dev(base).run(gpu_ctx)
    case = oer.copy_case(base)
    case["x"][1, 0, 3] = np.nan                                          # 0: the state
    case["xa"][2, 1, 5] = np.inf                                         # 0: the prior state
    case["se"][3, 7] = -0.25                                             # 2: a kept row's variance
    for b in case["k"]:
        b[4] = np.nan                                                    # 3: what an invalid profile of the Jacobian call looks like
    case["fx"][4] = np.nan
    case["se"][5, 2] = 0.0                                               # 2 as well
    lin, sol, cost = reference(case)
    assert lin["lin_status"].tolist() == [1, 0, 0, 2, 3, 2, 1] and sol["status"].tolist() == [1, 0, 0, 2, 3, 2, 1]
    got = Dev(case).run(gpu_ctx)
    check_prepare(got, lin, m, "statuses")
    check_solve(got, sol, case, "statuses", True)
    check_cost(got, cost, m, nlev * nblk, "statuses")
    assert got["nobs"].tolist() == [m, 0, 0, m, 0, m, m] and not got["keep"][[1, 2, 4]].any() and got["keep"][[3, 5]].all()
    # nothing observed: xa exactly, chi2 and dfs 0, the posterior is the prior as the inverse of Sa^-1 gives it
    assert np.array_equal(got["x_new"][4], case["xa"][4]) and got["chi2"][4] == 0.0 and got["dfs"][4] == 0.0
    scale = np.abs(sol["post_cov"][4]).max()
    assert np.abs(got["post_cov"][4] - sol["post_cov"][4]).max() <= nfr.TOL * scale
    assert np.array_equal(np.diag(got["post_cov"][4]), got["post_var"][4].reshape(-1))
    assert got["cost_obs"][4] == 0.0 and got["cost"][4] == got["cost_prior"][4] > 0.0
    assert np.isposinf([got["cost"][1], got["cost_obs"][1], got["cost_prior"][1], got["cost"][2]]).all()
    assert np.isnan([got["cost"][3], got["cost_obs"][5], got["cost_prior"][5]]).all()
    for i in (0, 6):
        for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
            assert np.array_equal(got[key][i], clean[key][i]), (i, key)
    # damped: the pull towards the prior where nothing is observed; a gamma that is negative or not finite is status 2
    gamma = np.array([0.5, 0.5, 0.5, 0.5, 1.0, 0.5, -1.0])
    _, damped, _ = reference(case, gamma)
    got = Dev(case).run(gpu_ctx, gamma=gamma)
    assert got["status"].tolist() == damped["status"].tolist() == [1, 0, 0, 2, 3, 2, 2]
    assert np.array_equal(got["x_new"][4], case["xa"][4] + 0.5 * (case["x"][4] - case["xa"][4]))
    assert np.isnan(got["x_new"][[1, 2, 3, 5, 6]]).all()
    check_solve(got, damped, case, "statuses, damped", False)
    for g in (np.inf, np.nan):
        assert Dev(base).run(gpu_ctx, gamma=np.where(np.arange(nprof) == 2, g, 1.0))["status"].tolist() == [1, 1, 2, 1, 1, 1, 1]
    # the state not finite at the solve alone, after a clean linearisation
    d = Dev(base)
    gpu_ctx.oe_nform_prepare_device(**d.prepare_args())
    d.x[3, 1, 0] = float("nan")
    gpu_ctx.oe_nform_solve_device(**d.solve_args())
    torch.cuda.synchronize()
    got = d.host()
    assert got["status"].tolist() == [1, 1, 1, 0, 1, 1, 1] and np.isnan(got["x_new"][3]).all() and np.isnan(got["post_cov"][3]).all()
    # an indefinite C: status 2
    d = Dev(base)
    gpu_ctx.oe_nform_prepare_device(**d.prepare_args())
    d.out["h"][2] = -1e12
    gpu_ctx.oe_nform_solve_device(**d.solve_args())
    torch.cuda.synchronize()
    got = d.host()
    assert got["status"].tolist() == [1, 1, 2, 1, 1, 1, 1] and np.isnan(got["x_new"][2]).all() and np.isnan(got["dfs"][2])
    # a trial whose forward run failed in a kept row: +inf, to be rejected; in a dropped row it is not looked at
    d = Dev(base)
    first = d.run(gpu_ctx)
    d.fx[2, 7] = float("nan")
    d.out["keep"][4, 11] = 0
    d.fx[4, 11] = float("inf")
    gpu_ctx.oe_nform_cost_device(**d.cost_args())
    torch.cuda.synchronize()
    again = d.host()
    assert np.isposinf(again["cost"][2]) and np.isposinf(again["cost_obs"][2]) and again["cost_status"][2] == 1
    assert np.isfinite(again["cost"][4]) and again["cost"][4] < first["cost"][4] and again["cost_prior"][4] == first["cost_prior"][4]
    for i in (0, 1, 3, 5, 6):
        assert again["cost"][i] == first["cost"][i]


@pytest.mark.parametrize("gamma", [None, 0.5], ids=["undamped", "damped"])
def test_inactive_profiles_keep_their_sentinels(gpu_ctx, gamma):
    case = seeded(43, 2, 154, True, True, 4)[0]
    full = Dev(case).run(gpu_ctx, gamma=gamma)
    d = Dev(case)
    blank = d.host()
    active = _dev(np.array([1, 0, 1, 0], dtype=np.uint8))
    got = d.run(gpu_ctx, gamma=gamma, active=active)
    for key in LIN_KEYS + SOLVE_KEYS + COST_KEYS:
        for i in (0, 2):
            assert np.array_equal(got[key][i], full[key][i]), (key, i)
        for i in (1, 3):
            assert np.array_equal(got[key][i], blank[key][i]), (key, i)


def test_outputs_do_not_depend_on_the_batch(gpu_ctx):
    nlev, nblk, m = 8, 1, 98
    big = nfr.make_case(nlev, nblk, m, nprof=300, se_per_profile=True)
    keys = LIN_KEYS + SOLVE_KEYS + COST_KEYS
    got300 = Dev(big).run(gpu_ctx)
    again = Dev(big).run(gpu_ctx)
    for key in keys:
        assert np.array_equal(got300[key], again[key]), key
    assert (got300["status"] == 1).all() and (got300["lin_status"] == 1).all() and (got300["cost_status"] == 1).all()

    def sub(lo, hi):
        part = dict(big, k=[b[lo:hi] for b in big["k"]], x=big["x"][lo:hi], y=big["y"][lo:hi], fx=big["fx"][lo:hi],
                    se=big["se"][lo:hi])
        return Dev(part).run(gpu_ctx)

    for nprof in (1, 5):
        got = sub(0, nprof)
        for key in keys:
            assert np.array_equal(got[key], got300[key][:nprof]), (nprof, key)
    got = sub(299, 300)                                                  # the last profile of the large batch as a batch of one
    for key in keys:
        assert np.array_equal(got[key][0], got300[key][299]), key


def test_more_observations_than_the_m_form_takes(gpu_ctx):
    """m = 141: mwrt_oe_step_device refuses it with its limit in the text; the n-form entries serve it."""
    nlev, nblk, m, nprof = 33, 1, 141, 4
    case, _, (lin, sol, cost), _ = seeded(nlev, nblk, m, False, False, nprof)
    d = Dev(case)
    sa = _dev(case["sa"])
    with pytest.raises(MwrtError) as ei:
        gpu_ctx.oe_step_device(nprof, nlev, m, [b.data_ptr() for b in d.k], d.x.data_ptr(), d.xa.data_ptr(), sa.data_ptr(),
                               d.se.data_ptr(), d.y.data_ptr(), d.fx.data_ptr(), d.out["x_new"].data_ptr(),
                               d.out["status"].data_ptr(), stream=_cur())
    assert ei.value.code == -5 and str(_native.OE_MAX_M) in str(ei.value)
    got = d.run(gpu_ctx)
    assert got["status"].tolist() == [1] * nprof and got["nobs"].tolist() == [m] * nprof
    check_solve(got, sol, case, "m = 141", True)


def test_argument_refusals_and_an_empty_batch(gpu_ctx):
    case = nfr.make_case(3, 3, 14, nprof=2)
    d = Dev(case)
    rec = _native.MwrtOeNform

    def code(entry, base, **change):
        with pytest.raises(MwrtError) as ei:
            getattr(gpu_ctx, entry)(**dict(base, **change))
        return ei.value.code, str(ei.value)

    gamma = _dev(np.zeros(2))
    for entry, base in (("oe_nform_prepare_device", d.prepare_args()), ("oe_nform_solve_device", d.solve_args()),
                        ("oe_nform_cost_device", d.cost_args())):
        getattr(gpu_ctx, entry)(**base)                                  # the unchanged call is accepted
        assert code(entry, base, d_x=None)[0] == -1 and code(entry, base, reserved=1)[0] == -1
        assert code(entry, base, nlev=0)[0] == -1 and code(entry, base, m=0)[0] == -1 and code(entry, base, nprof=-1)[0] == -1
        assert code(entry, base, struct_size=rec.d_k.offset - 1)[0] == -1
        c, text = code(entry, base, nlev=43)                             # n = 129
        assert c == -5 and str(_native.OE_NFORM_MAX_N) in text
        getattr(gpu_ctx, entry)(**dict(base, nprof=0))                   # nothing to do is not an error
    c, text = code("oe_nform_solve_device", d.solve_args(gamma))
    assert c == -1 and "gamma = 0 only" in text
    # optional outputs beyond a shorter record are not written: a solve whose record ends after d_status
    d.reset()
    gpu_ctx.oe_nform_prepare_device(**d.prepare_args())
    gpu_ctx.oe_nform_solve_device(**dict(d.solve_args(), struct_size=rec.d_chi2.offset))
    torch.cuda.synchronize()
    got = d.host()
    assert got["status"].tolist() == [1, 1] and (got["chi2"] == -7.0).all() and (got["post_cov"] == -7.0).all()
