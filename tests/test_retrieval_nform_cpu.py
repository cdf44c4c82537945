"""retrieval.OneDVar(form="n") without a GPU: the seams to the native library are replaced as in
tests/test_retrieval_se_cpu.py, the three n-form seams by the NumPy reference of tests/nform_reference.py.  What is checked
is the module's own work: ``step``, ``retrieve`` and ``retrieve_lm`` give what ``form="m"`` gives on the same case, to bars
scaled from nform_reference.TOL, in the same number of iterations; with ``form="m"`` nothing reaches the new seams; the
constructor's refusals; ``se=`` in both per-profile shapes; a case of m = 154 observations; the posterior covariance."""
import numpy as np
import pytest

import nform_reference as nfr
import oe_reference as oer

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd import retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402
from test_retrieval_basis_cpu import N, R, eofs  # noqa: E402
from test_retrieval_instrument_cpu import ELEV, FRQ, M, NLEV, NPROF, make, setup  # noqa: E402
from test_retrieval_se_cpu import SeStandins, observations, se_batch  # noqa: E402

# two forms of one step differ by the rounding of two factorisations: twice the bar of either
BAR = 2 * nfr.TOL


class NfStandins(SeStandins):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.nf_prepares, self.nf_solves, self.nf_costs = [], [], []
        for name in ("oe_nform_prepare", "oe_nform_solve", "oe_nform_cost"):
            monkeypatch.setattr(retrieval, "_native_" + name, getattr(self, name))

    @staticmethod
    def _sel(active, nprof):
        return np.ones(nprof, dtype=bool) if active is None else active.numpy().astype(bool)

    def oe_nform_prepare(self, k_blocks, x, xa, se, y, fx, lin, active, stream):
        nprof, nblk, nlev = x.shape
        m = y.shape[1]
        self.nf_prepares.append(dict(k=list(k_blocks), se=se, y=y.clone(), fx=fx.clone(), xa=xa, active=active))
        ref = nfr.prepare_reference([k.numpy().reshape(nprof, m, nlev) for k in k_blocks], x.numpy(), xa.numpy(), se.numpy(),
                                    y.numpy(), fx.numpy())
        sel = self._sel(active, nprof)
        lin["h"][sel] = torch.as_tensor(np.array([nfr.tri_pack(h) for h in ref["h"]]))[sel]
        for key in ("g", "rwr", "keep", "nobs", "lin_status"):
            lin[key][sel] = torch.as_tensor(ref[key])[sel]

    def oe_nform_solve(self, x, xa, sa_inv, lin, gamma, out, active, stream):
        nprof, nblk, nlev = x.shape
        self.nf_solves.append(dict(x=x.clone(), gamma=None if gamma is None else gamma.clone(), asked=sorted(out), sa_inv=sa_inv))
        assert gamma is None or not {"chi2", "dfs", "post_var", "post_cov"} & set(out)      # the entry refuses that
        ref = nfr.solve_linearisation(lin["h"].numpy(), lin["g"].numpy(), lin["rwr"].numpy(), lin["lin_status"].numpy(),
                                      x.numpy(), xa.numpy(), sa_inv.numpy(), None if gamma is None else gamma.numpy())
        sel = self._sel(active, nprof)
        for key, v in out.items():
            v[sel] = torch.as_tensor(ref[key]).reshape(v.shape)[sel]

    def oe_nform_cost(self, x, xa, sa_inv, se, y, fx, keep, cost, active, stream):
        self.nf_costs.append(dict(se=se))
        ref = nfr.cost_reference(x.numpy(), xa.numpy(), sa_inv.numpy(), se.numpy(), y.numpy(), fx.numpy(), keep.numpy())
        sel = self._sel(active, x.shape[0])
        cost[sel] = torch.as_tensor(ref["cost"])[sel]


def errors(got, ref, xa, sa):
    """oe_reference.block_errors of two result dicts of tensors (x_new [nprof][nblk][nlev])."""
    as_np = lambda d: {k: (None if v is None else v.numpy()) for k, v in d.items() if k in ("x_new", "chi2", "dfs", "post_var", "status")}   # noqa: E731
    return oer.block_errors(as_np(got), as_np(ref), dict(xa=np.asarray(xa), sa=np.asarray(sa)))


def result_errors(r_n, r_m, s):
    """Two Retrievals: x in units of the largest move from the prior (with the leading EOFs of this Sa, all of them in the
    temperature block, the humidity block stays at xa in both), post_var of max diag Sa per block, chi2 and dfs of max(1, |ref|)."""
    move = (r_m.x - torch.as_tensor(s["xa"])).abs().max()
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1.0)).max())   # noqa: E731
    return dict(x=float((r_n.x - r_m.x).abs().max() / move), post_var=post_var_error(r_n.post_var, r_m.post_var, s), chi2=rel(r_n.chi2, r_m.chi2), dfs=rel(r_n.dfs, r_m.dfs))


def post_var_error(got, want, s):
    """post_var [...][2][NLEV] (tensors or arrays) in units of max diag Sa per block."""
    dsa = np.diag(s["sa"]).reshape(2, NLEV).max(axis=1)
    diff = np.abs(np.asarray(got) - np.asarray(want)).reshape(-1, 2, NLEV)
    return float((diff.max(axis=(0, 2)) / dsa).max())


def pair(s, **kw):
    return make(s, **kw), make(s, form="n", **kw)


def test_with_form_m_nothing_reaches_the_new_seams(monkeypatch):
    st = NfStandins(monkeypatch)
    s = setup()
    ov = make(s)
    assert ov.form == "m"
    y = observations(st, s)
    ov.step(s["z"], s["p"], s["x_true"], y)
    ov.retrieve(s["z"], s["p"], y, max_iter=2)
    ov.retrieve_lm(s["z"], s["p"], y, max_iter=2)
    assert st.nf_prepares == [] and st.nf_solves == [] and st.nf_costs == []
    with pytest.raises(ValueError, match="post_cov=True.*form='n'"):
        ov.step(s["z"], s["p"], s["x_true"], y, post_cov=True)


def test_step_equals_form_m(monkeypatch):
    st = NfStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    y[1, 0, 2] = float("nan")                                            # one observation missing
    ov_m, ov_n = pair(s)
    x_m, d_m = ov_m.step(s["z"], s["p"], s["x_true"], y)
    steps = len(st.step_calls)
    x_n, d_n = ov_n.step(s["z"], s["p"], s["x_true"], y)
    assert len(st.step_calls) == steps and len(st.nf_prepares) == 1 and len(st.nf_solves) == 1      # prepare + solve, no m-form step
    assert st.nf_prepares[0]["se"] is ov_n.se and st.nf_prepares[0]["xa"] is ov_n.xa and st.nf_solves[0]["gamma"] is None
    assert st.nf_solves[0]["asked"] == ["chi2", "dfs", "post_var", "status", "x_new"]
    assert [tuple(k.shape) for k in st.nf_prepares[0]["k"]] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2
    assert d_n["status"].tolist() == d_m["status"].tolist() == [1] * NPROF and d_n["nobs"].tolist() == d_m["nobs"].tolist()
    assert d_n["nobs"].tolist() == [M, M - 1, M] and torch.equal(d_n["fx"], d_m["fx"]) and torch.equal(d_n["valid"], d_m["valid"])
    err = errors(dict(d_n, x_new=x_n), dict(d_m, x_new=x_m), s["xa"], s["sa"])
    assert max(err.values()) <= BAR, err
    assert set(d_n) == set(d_m)
    # without post_var, and with post_cov: the posterior covariance of this linear problem
    x2, d2 = ov_n.step(s["z"], s["p"], s["x_true"], y, post_var=False, post_cov=True)
    assert torch.equal(x2, x_n) and d2["post_var"] is None and d2["post_cov"].shape == (NPROF, N, N)
    assert st.nf_solves[-1]["asked"] == ["chi2", "dfs", "post_cov", "status", "x_new"]
    rows = st.rows(FRQ, ELEV)
    K = np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)
    post = np.linalg.inv(K.T @ K / 0.25 + np.linalg.inv(s["sa"]))
    assert np.abs(d2["post_cov"][0].numpy() - post).max() <= BAR * np.abs(post).max()
    assert post_var_error(d_n["post_var"][0], np.diag(post).reshape(2, NLEV), s) <= BAR


def test_step_with_a_basis_equals_form_m_and_needs_no_gain_or_product(monkeypatch):
    st = NfStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    sb = eofs(s)
    ov_m, ov_n = pair(s, basis=sb)
    c = torch.as_tensor(np.random.default_rng(3).standard_normal((NPROF, R)) * 0.2)
    c_m, d_m = ov_m.step(s["z"], s["p"], c, y)
    gains, products = len(st.gain_calls), len(st.product_calls)
    c_n, d_n = ov_n.step(s["z"], s["p"], c, y)
    assert (len(st.gain_calls), len(st.product_calls)) == (gains, products) == (1, 1)
    assert [tuple(k.shape) for k in st.nf_prepares[0]["k"]] == [(NPROF, M, R)] and c_n.shape == (NPROF, R)
    assert st.nf_solves[0]["asked"] == ["chi2", "dfs", "post_cov", "status", "x_new"] and "post_cov" not in d_n
    assert torch.equal(st.nf_solves[0]["sa_inv"], ov_n.sa_inv) and tuple(ov_n.sa_inv.shape) == (R, R)
    as3 = lambda v: v.reshape(NPROF, 1, R)                               # noqa: E731
    err = errors(dict(x_new=as3(c_n), chi2=d_n["chi2"], dfs=d_n["dfs"], status=d_n["status"]),
                 dict(x_new=as3(c_m), chi2=d_m["chi2"], dfs=d_m["dfs"], status=d_m["status"]), np.zeros((1, R)), sb.sa_c.numpy())
    assert max(err.values()) <= BAR, err
    # post_var is the level-space diag(B S^_c B^T)
    assert d_n["post_var"].shape == (NPROF, 2, NLEV)
    assert post_var_error(d_n["post_var"], d_m["post_var"], s) <= BAR
    x2, d2 = ov_n.step(s["z"], s["p"], c, y, post_cov=True)
    assert d2["post_cov"].shape == (NPROF, R, R)
    want = torch.einsum("kj,pji,ki->pk", sb.b, d2["post_cov"], sb.b).reshape(NPROF, 2, NLEV)
    assert torch.equal(d2["post_var"], want)


@pytest.mark.parametrize("with_basis", [False, True], ids=["levels", "basis"])
def test_retrieve_equals_form_m_in_as_many_iterations(monkeypatch, with_basis):
    st = NfStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    ov_m, ov_n = pair(s, **({"basis": eofs(s)} if with_basis else {}))
    r_m = ov_m.retrieve(s["z"], s["p"], y, max_iter=6, tol=1e-6)
    r_n = ov_n.retrieve(s["z"], s["p"], y, max_iter=6, tol=1e-6)
    assert r_n.iterations.tolist() == r_m.iterations.tolist() and r_n.converged.tolist() == r_m.converged.tolist() == [True] * NPROF
    assert r_n.status.tolist() == r_m.status.tolist() and r_n.nobs.tolist() == r_m.nobs.tolist()
    assert max(result_errors(r_n, r_m, s).values()) <= 6 * BAR           # at most six steps' worth
    if with_basis:
        assert (r_n.coeff - r_m.coeff).abs().max() <= 6 * BAR * r_m.coeff.abs().max() and len(st.product_calls) == 1


@pytest.mark.parametrize("with_basis", [False, True], ids=["levels", "basis"])
def test_retrieve_lm_equals_form_m_in_as_many_iterations(monkeypatch, with_basis):
    st = NfStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    y[2, 1, 1] = float("nan")
    ov_m, ov_n = pair(s, **({"basis": eofs(s)} if with_basis else {}))
    # the default tol: no accept / reject decision of this case hangs on the last bits of J, which differ between the forms
    r_m = ov_m.retrieve_lm(s["z"], s["p"], y, max_iter=12)
    steps = len(st.step_calls)
    r_n = ov_n.retrieve_lm(s["z"], s["p"], y, max_iter=12)
    assert len(st.step_calls) == steps                                   # the final diagnostics: an undamped n-form solve
    assert st.nf_solves[-1]["gamma"] is None and all(c["gamma"] is not None for c in st.nf_solves[:-1])
    assert st.nf_prepares[-1]["active"] is None                          # ... on a linearisation of every profile
    assert r_n.iterations.tolist() == r_m.iterations.tolist() and r_n.converged.tolist() == r_m.converged.tolist()
    assert r_m.converged.all() and int(r_m.iterations.max()) >= 3
    assert torch.equal(r_n.gamma, r_m.gamma) and r_n.nobs.tolist() == r_m.nobs.tolist() == [M, M, M - 1]
    assert torch.allclose(r_n.cost, r_m.cost, rtol=1e-9, atol=0)
    assert max(result_errors(r_n, r_m, s).values()) <= 12 * BAR


def test_per_profile_se_in_both_shapes(monkeypatch):
    st = NfStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    ov_m, ov_n = pair(s)
    var = torch.as_tensor(0.25 * (1.0 + np.random.default_rng(8).uniform(0.0, 2.0, (NPROF, M))))
    x_m, d_m = ov_m.step(s["z"], s["p"], s["x_true"], y, se=var)        # the m-form whitens
    whitens = len(st.whiten_calls)
    x_n, d_n = ov_n.step(s["z"], s["p"], s["x_true"], y, se=var)
    # [nprof][m] goes straight in: no whitening, the entry's se_per_profile
    assert len(st.whiten_calls) == whitens == 1 and torch.equal(st.nf_prepares[-1]["se"], var) and "whiten_status" not in d_n
    assert max(errors(dict(d_n, x_new=x_n), dict(d_m, x_new=x_m), s["xa"], s["sa"]).values()) <= BAR
    # [nprof][m][m] goes through the existing whitening, then variances of 1
    full = se_batch()
    x_m, d_m = ov_m.step(s["z"], s["p"], s["x_true"], y, se=full)
    x_n, d_n = ov_n.step(s["z"], s["p"], s["x_true"], y, se=full)
    assert len(st.whiten_calls) == whitens + 2 and (st.nf_prepares[-1]["se"] == 1.0).all() and st.nf_prepares[-1]["se"].shape == (M,)
    assert torch.equal(st.nf_prepares[-1]["y"], st.whiten_calls[-1]["out"]["y"]) and d_n["whiten_status"].tolist() == [1] * NPROF
    assert max(errors(dict(d_n, x_new=x_n), dict(d_m, x_new=x_m), s["xa"], s["sa"]).values()) <= BAR
    # both in retrieve_lm: the cost is that of Se_p
    for se in (var, full):
        r_m = ov_m.retrieve_lm(s["z"], s["p"], y, max_iter=8, se=se)
        r_n = ov_n.retrieve_lm(s["z"], s["p"], y, max_iter=8, se=se)
        assert r_n.iterations.tolist() == r_m.iterations.tolist() and torch.allclose(r_n.cost, r_m.cost, rtol=1e-9, atol=0)
        assert (r_n.x - r_m.x).abs().max() <= 8 * BAR * (r_m.x - torch.as_tensor(s["xa"])).abs().max()
    assert st.nf_costs[-1]["se"].shape == (M,) and any(c["se"].shape == (NPROF, M) for c in st.nf_costs)
    # an indefinite Se_p: status 2 and NaN, as with form="m"
    bad = full.clone()
    bad[1] = -bad[1]
    x_n, d_n = ov_n.step(s["z"], s["p"], s["x_true"], y, se=bad)
    assert d_n["status"].tolist() == [1, 2, 1] and d_n["whiten_status"].tolist() == [1, 2, 1]
    assert torch.isnan(x_n[1]).all() and torch.isnan(d_n["post_var"][1]).all() and torch.isnan(d_n["chi2"][1])


def test_more_observations_than_the_m_form_takes(monkeypatch):
    """14 channels x 11 elevations = 154 observations, also through an instrument."""
    st = NfStandins(monkeypatch)
    s = setup()
    frq = np.linspace(22.0, 58.0, 14)
    elev = np.linspace(10.0, 90.0, 11)
    m = frq.size * elev.size
    assert m == 154
    se = np.full(m, 0.25)
    rng = np.random.default_rng(12)
    x_true, xa = s["x_true"], torch.as_tensor(s["xa"])
    noise = 0.5 * rng.standard_normal((NPROF, m))
    for inst in (None, Instrument(frq, elev, beam=3.5, band=0.23, n_beam=3, n_band=2)):
        ov = retrieval.OneDVar("R24", frq, elev, torch.as_tensor(s["sa"]), torch.as_tensor(se), variables=JacVariables.of(humidity="rh"),
                               blocks=("t", "h"), xa=xa, form="n", instrument=inst)
        assert ov.m == m
        # the linear problem in what the update sees: the operator's rows, or the instrument's channel rows
        grid = (frq, elev) if inst is None else (inst.frq_q, inst.elev_q)
        w = np.eye(m) if inst is None else inst.dense()
        rows = st.rows(*grid)
        K = w @ np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)
        y = st.forward(x_true[:, 0], x_true[:, 1], *grid).numpy() @ w.T + noise
        fxa = w @ st.forward(xa[None, 0], xa[None, 1], *grid).numpy()[0]
        post = np.linalg.inv(K.T @ K / 0.25 + np.linalg.inv(s["sa"]))
        want = s["xa"].reshape(-1)[None] + (y - fxa[None]) @ (post @ K.T / 0.25).T
        res = ov.retrieve(s["z"], s["p"], torch.as_tensor(y).reshape(NPROF, elev.size, frq.size), max_iter=4, tol=1e-6)
        assert res.status.tolist() == [1] * NPROF and res.nobs.tolist() == [m] * NPROF and res.converged.all()
        assert st.nf_prepares[-1]["y"].shape == (NPROF, m)
        got = res.x.numpy().reshape(NPROF, N)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want - s["xa"].reshape(-1)[None]).max()
        assert post_var_error(res.post_var, np.broadcast_to(np.diag(post).reshape(2, NLEV), (NPROF, 2, NLEV)), s) <= BAR


def test_constructor_and_call_refusals(monkeypatch):
    NfStandins(monkeypatch)
    s = setup()
    with pytest.raises(ValueError, match="form must be 'm'.*or 'n'"):
        make(s, form="x")
    # the constructor's se must be variances: the message names the two alternatives
    full = dict(s, se=0.25 * np.eye(M))
    make(full)                                                           # fine with form="m"
    with pytest.raises(ValueError) as ei:
        make(full, form="n")
    assert "per-profile full covariance" in str(ei.value) and "se= of" in str(ei.value) and "form='m'" in str(ei.value)
    # the update's state size: nblk nlev without a basis, r with one
    nlev = 65
    xa = torch.zeros((2, nlev), dtype=torch.float64)
    sa = torch.eye(2 * nlev, dtype=torch.float64)
    kw = dict(variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=xa)
    retrieval.OneDVar("R24", FRQ, ELEV, sa, torch.as_tensor(s["se"]), **kw)
    with pytest.raises(ValueError, match="at most 128 elements, got 130"):
        retrieval.OneDVar("R24", FRQ, ELEV, sa, torch.as_tensor(s["se"]), form="n", **kw)
    small = retrieval.StateBasis.from_covariance(sa, 128)
    retrieval.OneDVar("R24", FRQ, ELEV, None, torch.as_tensor(s["se"]), form="n", basis=small, **kw)       # r = 128 of n = 130
    with pytest.raises(ValueError, match="at most 128 elements, got 129"):
        retrieval.OneDVar("R24", FRQ, ELEV, None, torch.as_tensor(s["se"]), form="n", basis=retrieval.StateBasis.from_covariance(sa, 129), **kw)
    coarse = dict(kw, xa=torch.zeros((2, 43), dtype=torch.float64))      # a coarse full state is allowed
    assert retrieval.OneDVar("R24", FRQ, ELEV, torch.eye(86, dtype=torch.float64), torch.as_tensor(s["se"]), form="n", **coarse).form == "n"
    ov = make(s, form="n")
    y = torch.full((NPROF, ELEV.size, FRQ.size), 255.0, dtype=torch.float64)
    with pytest.raises(ValueError) as ei:
        ov.characterise(s["z"], s["p"], s["x_true"], y)
    assert "form='m'" in str(ei.value) and "post_cov=True" in str(ei.value)
    with pytest.raises(ValueError, match=r"se: expected a float64 tensor \[3\]\[6\] or \[3\]\[6\]\[6\]"):
        ov.step(s["z"], s["p"], s["x_true"], y, se=torch.ones(M, dtype=torch.float64))
