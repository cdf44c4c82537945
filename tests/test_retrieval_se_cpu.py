"""retrieval.OneDVar with a per-profile observation-error covariance (``se=``), without a GPU: the seams to the native library
are replaced as in tests/test_retrieval_basis_cpu.py, the damped entries as in tests/test_retrieval_lm_cpu.py and the two
whitening seams by tests/whiten_reference.py.  What is checked is the module's own work: without ``se=`` nothing reaches
the seams that did not before and the whitening seams are never called; with it the update sees ones(m) and the whitened K,
y and F; whitening comes behind the instrument's reduction and the basis projection; ``retrieve_lm`` whitens the trial's F
with the linearisation's factor; ``characterise`` hands back the un-whitened gain; and a linear problem with two very
different Se_p lands on each profile's own posterior mean, which the batch-mean Se misses."""
import numpy as np
import pytest

import oe_char_reference as ocr
import whiten_reference as whr

torch = pytest.importorskip("torch")

import test_retrieval_lm_cpu as lmt  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd import retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402
from test_retrieval_basis_cpu import BasisStandins, N, R, eofs  # noqa: E402
from test_retrieval_instrument_cpu import ELEV, FRQ, M, NLEV, NPROF, make, setup  # noqa: E402

WHITEN = retrieval._native_obs_whiten                                    # the real seam: its shape checks


class SeStandins(BasisStandins):
    _k = staticmethod(lmt.Standins._k)

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.whiten_calls, self.apply_calls, self.cost_calls, self.prepare_calls, self.solves, self.prepares = [], [], [], [], [], []
        for name in ("obs_whiten", "obs_whiten_apply", "oe_lm_prepare", "oe_lm_solve", "oe_cost"):
            monkeypatch.setattr(retrieval, "_native_" + name, getattr(self, name))

    def obs_whiten(self, k_blocks, se, y, fx, stream):
        self.order.append("whiten")
        nprof, m = y.shape
        ref = whr.whiten_reference([k.numpy().reshape(nprof, m, k.shape[-1]) for k in k_blocks], se.numpy(), y.numpy(), fx.numpy())
        out = dict(k=[torch.as_tensor(o).reshape(k.shape) for o, k in zip(ref["k_out"], k_blocks)], y=torch.as_tensor(ref["y_out"]),
                   fx=torch.as_tensor(ref["fx_out"]), l=torch.as_tensor(ref["l"]), keep=torch.as_tensor(ref["keep"]),
                   status=torch.as_tensor(ref["status"]))
        self.whiten_calls.append(dict(k=list(k_blocks), se=se, y=y.clone(), fx=fx.clone(), out=out, stream=stream))
        return out

    def obs_whiten_apply(self, l, keep, mode, vec, block, stream):
        self.order.append("apply%d" % mode)
        self.apply_calls.append(dict(l=l, keep=keep, mode=mode, vec=None if vec is None else vec.clone(),
                                     block=None if block is None else block.clone()))
        run = lambda v: None if v is None else torch.as_tensor(whr.apply_reference(l.numpy(), keep.numpy(), v.numpy(), mode))   # noqa: E731
        return run(vec), run(block)

    def oe_lm_prepare(self, k_blocks, x, xa, sa, se, y, fx, lin, active, stream):
        self.prepare_calls.append(dict(k=list(k_blocks), se=se, y=y.clone(), fx=fx.clone()))
        lmt.Standins.oe_lm_prepare(self, k_blocks, x, xa, sa, se, y, fx, lin, active, stream)

    def oe_lm_solve(self, k_blocks, x, xa, sa, se, gamma, lin, out, active, stream):
        lmt.Standins.oe_lm_solve(self, k_blocks, x, xa, sa, se, gamma, lin, out, active, stream)
        self.solves[-1]["se"] = se

    def oe_cost(self, x, xa, se, y, fx, keep, sa_inv, cost, active, stream):
        self.cost_calls.append(dict(x=x.clone(), se=se, y=y.clone(), fx=fx.clone(), keep=keep))
        lmt.Standins.oe_cost(self, x, xa, se, y, fx, keep, sa_inv, cost, active, stream)


def se_batch(nprof=NPROF, seed=4):
    """A full Se_p per profile: correlated, growing with the profile index."""
    rng = np.random.default_rng(seed)
    out = np.empty((nprof, M, M))
    for p in range(nprof):
        j = rng.standard_normal((M, 3)) * 0.3
        out[p] = (0.1 + 0.4 * p) * np.eye(M) + j @ j.T
    return torch.as_tensor(out)


def observations(st, s, seed=6):
    rng = np.random.default_rng(seed)
    fx = st.forward(s["x_true"][:, 0], s["x_true"][:, 1] * 0 + 0.5, FRQ, ELEV)
    return (fx + torch.as_tensor(0.3 * rng.standard_normal(tuple(fx.shape)))).reshape(NPROF, ELEV.size, FRQ.size)


def test_without_se_the_seams_see_what_they_saw(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    ov = make(s)
    y = observations(st, s)
    x_new, d = ov.step(s["z"], s["p"], s["x_true"], y)
    res = ov.retrieve(s["z"], s["p"], y, max_iter=2)
    lm = ov.retrieve_lm(s["z"], s["p"], y, max_iter=2)
    ch = ov.characterise(s["z"], s["p"], res.x, y)
    assert st.whiten_calls == [] and st.apply_calls == [] and st.order == []
    yv = y.reshape(NPROF, M)
    for c in st.step_calls:
        assert c["args"][1] is ov.xa and c["args"][2] is ov.sa and c["args"][3] is ov.se and torch.equal(c["y"], yv)
        assert [tuple(k.shape) for k in c["k"]] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2
    c = st.step_calls[0]
    assert torch.equal(c["fx"], st.forward(s["x_true"][:, 0], st.k_calls[0]["args"][4], FRQ, ELEV)) and torch.equal(d["fx"], c["fx"])
    assert "whiten_status" not in d and x_new.shape == (NPROF, 2, NLEV)
    assert all(c["se"] is ov.se and torch.equal(c["y"], yv) for c in st.prepare_calls + st.cost_calls)
    assert all(c["se"] is ov.se for c in st.solves) and len(st.prepare_calls) >= 1 and len(st.cost_calls) >= 2
    # the trial's F reached the cost as the forward model gave it
    trial = st.cost_calls[1]
    assert torch.equal(trial["fx"], st.forward(trial["x"][:, 0], ov.physical(s["z"], s["p"], trial["x"])[2], FRQ, ELEV))
    assert st.gain_calls[0]["xa"] is ov.xa and ch.gain.shape == (NPROF, M, N) and lm.status.tolist() == [1] * NPROF


def test_with_se_the_update_sees_ones_and_the_whitened_linearisation(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    ov = make(s)
    y = observations(st, s)
    y[1, 0, 1] = float("nan")                                            # profile 1 loses a row
    se_p = se_batch()
    x_new, d = ov.step(s["z"], s["p"], s["x_true"], y, se=se_p)
    assert len(st.whiten_calls) == 1 and st.apply_calls == []
    w = st.whiten_calls[0]
    # the whitening got the K-matrix call's rows as it wrote them, the per-profile Se, y and the physical F
    assert [tuple(k.shape) for k in w["k"]] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2 and w["se"] is se_p
    fx = st.forward(s["x_true"][:, 0], st.k_calls[0]["args"][4], FRQ, ELEV)
    assert torch.equal(w["fx"], fx) and torch.equal(w["y"].nan_to_num(-1.0), y.reshape(NPROF, M).nan_to_num(-1.0))
    # the update got ones(m) and what the whitening wrote; the prior is untouched
    c = st.step_calls[0]
    se_seen = c["args"][3]
    assert tuple(se_seen.shape) == (M,) and (se_seen == 1.0).all() and se_seen.dtype == torch.float64
    assert c["args"][1] is ov.xa and c["args"][2] is ov.sa
    assert all(torch.equal(a, b) for a, b in zip(c["k"], w["out"]["k"]))
    assert torch.equal(c["y"].nan_to_num(-1.0), w["out"]["y"].nan_to_num(-1.0)) and torch.equal(c["fx"].nan_to_num(-1.0), w["out"]["fx"].nan_to_num(-1.0))
    rows = st.rows(FRQ, ELEV)
    K = np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)
    L0 = np.linalg.cholesky(se_p[0].numpy())
    got = np.concatenate([k[0].numpy().reshape(M, NLEV) for k in c["k"]], axis=1)
    assert np.abs(got - np.linalg.solve(L0, K)).max() <= 1e-12 * np.abs(K).max()
    # the diagnostics: the physical F, the whitening's verdict, the step's own row count
    assert torch.equal(d["fx"], fx) and d["whiten_status"].tolist() == [1] * NPROF and d["nobs"].tolist() == [M, M - 1, M]
    # ... and the step is that of each profile alone with its own Se_p as the shared se
    for p in range(NPROF):
        own = make(dict(s, se=se_p[p].numpy()))
        x_own, d_own = own.step(s["z"][p:p + 1], s["p"][p:p + 1], s["x_true"][p:p + 1], y[p:p + 1])
        scale = (x_own - ov.xa).abs().amax()
        assert (x_new[p] - x_own[0]).abs().max() <= 1e-10 * scale
        assert abs(d["chi2"][p] - d_own["chi2"][0]) <= 1e-10 * max(1.0, d_own["chi2"][0]) and abs(d["dfs"][p] - d_own["dfs"][0]) <= 1e-10
        assert (d["post_var"][p] - d_own["post_var"][0]).abs().max() <= 1e-10 * np.diag(s["sa"]).max()
    # variances [nprof][m] go the same way
    var = torch.as_tensor(np.random.default_rng(8).uniform(0.1, 2.0, (NPROF, M)))
    ov.step(s["z"], s["p"], s["x_true"], y, se=var)
    assert st.whiten_calls[-1]["se"] is var and (st.step_calls[-1]["args"][3] == 1.0).all()
    assert np.abs(st.step_calls[-1]["y"][0].numpy() - (y[0].reshape(M) / var[0].sqrt()).numpy()).max() <= 1e-12 * 300


def test_instrument_and_basis_reduce_then_project_then_whiten(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    inst = Instrument(FRQ, ELEV, beam=3.5, band=[0.23, 0.23, 2.0], n_beam=3, n_band=2)
    sb = eofs(s)
    ov = make(s, instrument=inst, basis=sb)
    y = torch.full((NPROF, ELEV.size, FRQ.size), 255.0, dtype=torch.float64)
    se_p = se_batch()
    ov.step(s["z"], s["p"], torch.zeros((NPROF, R), dtype=torch.float64), y, post_var=False, se=se_p)
    assert st.order == ["reduce", "project", "whiten"]
    # the whitening got the r columns of K B, not the n of K
    assert [tuple(k.shape) for k in st.whiten_calls[0]["k"]] == [(NPROF, M, R)]
    grid = st.rows(inst.frq_q, inst.elev_q)
    kb = inst.dense() @ np.concatenate([grid["t"].numpy(), grid["h"].numpy()], axis=1) @ sb.b.numpy()
    want = np.linalg.solve(np.linalg.cholesky(se_p[2].numpy()), kb)
    got = st.step_calls[0]["k"][0][2].numpy()
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max() and (st.step_calls[0]["args"][3] == 1.0).all()
    # post_var in level space runs the gain entry on the same whitened block, with ones
    st.order.clear()
    _, d = ov.step(s["z"], s["p"], torch.zeros((NPROF, R), dtype=torch.float64), y, se=se_p)
    assert st.order == ["reduce", "project", "whiten"] and d["post_var"].shape == (NPROF, 2, NLEV)
    assert torch.equal(st.gain_calls[-1]["k"][0], st.step_calls[-1]["k"][0])


def test_retrieve_lm_whitens_the_trial_with_the_factor_of_the_linearisation(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    ov = make(s)
    y = observations(st, s)
    se_p = se_batch()
    res = ov.retrieve_lm(s["z"], s["p"], y, max_iter=3, se=se_p)
    assert res.status.tolist() == [1] * NPROF and len(st.whiten_calls) >= 1
    assert all(a["mode"] == 0 and a["block"] is None for a in st.apply_calls) and len(st.apply_calls) == len(st.solves)
    # the first trial: whitened with the l and keep the first linearisation's whitening wrote
    w, a = st.whiten_calls[0], st.apply_calls[0]
    assert a["l"] is w["out"]["l"] and a["keep"] is w["out"]["keep"]
    trial = st.cost_calls[1]                                             # [0] is J at x, [1] J at the first trial
    f_phys = st.forward(trial["x"][:, 0], ov.physical(s["z"], s["p"], trial["x"])[2], FRQ, ELEV)
    assert torch.equal(a["vec"], f_phys)
    assert np.abs(trial["fx"].numpy() - whr.apply_reference(w["out"]["l"].numpy(), w["out"]["keep"].numpy(), f_phys.numpy(), 0)).max() == 0
    for c in st.prepare_calls + st.cost_calls:
        assert (c["se"] == 1.0).all() and tuple(c["se"].shape) == (M,) and torch.equal(c["y"], w["out"]["y"])
    assert all((c["se"] == 1.0).all() for c in st.solves)
    assert torch.equal(st.prepare_calls[0]["fx"], w["out"]["fx"]) and all(
        torch.equal(a, b) for a, b in zip(st.prepare_calls[0]["k"], w["out"]["k"]))
    # a linear problem: the damped loop ends where each profile alone ends with its own Se_p
    res = ov.retrieve_lm(s["z"], s["p"], y, max_iter=30, tol=1e-9, se=se_p)
    for p in range(NPROF):
        own = make(dict(s, se=se_p[p].numpy())).retrieve_lm(s["z"][p:p + 1], s["p"][p:p + 1], y[p:p + 1], max_iter=30, tol=1e-9)
        assert (res.x[p] - own.x[0]).abs().max() <= 1e-7 * (own.x[0] - ov.xa).abs().max()
        assert abs(res.cost[p] - own.cost[0]) <= 1e-9 * max(1.0, own.cost[0])


def test_characterise_returns_the_gain_of_the_physical_observations(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    ov = make(s)
    y = observations(st, s)
    y[2, 1, 0] = float("nan")
    se_p = se_batch()
    ch = ov.characterise(s["z"], s["p"], s["x_true"], y, avk=True, post_cov=True, se=se_p)
    assert st.order == ["whiten", "apply1"] and st.apply_calls[0]["vec"] is None
    assert st.apply_calls[0]["l"] is st.whiten_calls[0]["out"]["l"]
    rows = st.rows(FRQ, ELEV)
    k = [np.broadcast_to(rows[b].numpy()[None], (NPROF, M, NLEV)) for b in ("t", "h")]
    fx = st.forward(s["x_true"][:, 0], st.k_calls[0]["args"][4], FRQ, ELEV).numpy()
    for p in range(NPROF):
        ref = ocr.oe_char_reference([b[p:p + 1] for b in k], s["x_true"][p:p + 1].numpy(), s["xa"], s["sa"], se_p[p].numpy(),
                                    y.reshape(NPROF, M)[p:p + 1].numpy(), fx[p:p + 1])
        for key in ("gain", "avk_diag", "dfs_block", "noise_var", "smooth_var", "avk", "post_cov"):
            got = getattr(ch, key)[p].numpy()
            assert np.abs(got - ref[key][0]).max() <= 1e-10 * max(np.abs(ref[key][0]).max(), 1e-300), (p, key)
        assert ch.keep[p].tolist() == ref["keep"][0].tolist() and ch.nobs[p] == ref["nobs"][0]
    assert (ch.gain[2, 3] == 0).all()                                    # row (1, 0) of profile 2 was dropped


def test_two_profiles_with_very_different_se_reach_their_own_posterior_means(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup(nprof=2)
    ov = make(s)
    rows = st.rows(FRQ, ELEV)
    K = np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)    # [m][n]
    rng = np.random.default_rng(12)
    j = rng.standard_normal((2, M, 2))
    se_p = np.stack([0.01 * np.eye(M) + 0.005 * j[0] @ j[0].T, 25.0 * np.eye(M) + 4.0 * j[1] @ j[1].T])
    xa = s["xa"].reshape(-1)
    x_true = torch.as_tensor(s["xa"][None] + 0.3 * rng.standard_normal((2, 2, NLEV)) * np.array([2.0, 0.1])[None, :, None])
    f = lambda x: st.forward(x[:, 0], ov.physical(s["z"][:len(x)], s["p"][:len(x)], x)[2], FRQ, ELEV).numpy()   # noqa: E731
    y = f(x_true) + np.stack([np.linalg.cholesky(se_p[p]) @ rng.standard_normal(M) for p in range(2)])
    fxa = f(torch.as_tensor(s["xa"][None]))[0]
    sa_inv = np.linalg.inv(s["sa"])

    def mean(se):
        si = np.linalg.inv(se)
        return xa + np.linalg.solve(K.T @ si @ K + sa_inv, K.T @ si @ (y_p - fxa))

    want = np.empty((2, N))
    miss = np.empty((2, N))
    for p in range(2):
        y_p = y[p]
        want[p], miss[p] = mean(se_p[p]), mean(se_p.mean(axis=0))
    assert (want.reshape(2, 2, NLEV)[:, 1] > 0).all()                    # no clamp in the way
    sigma = np.sqrt(np.diag(s["sa"]))
    assert (np.abs(miss - want) / sigma[None]).max(axis=1).min() > 1e-3  # the reference itself: the batch mean misses both
    yt = torch.as_tensor(y).reshape(2, ELEV.size, FRQ.size)
    res = ov.retrieve(s["z"], s["p"], yt, max_iter=5, tol=1e-9, se=torch.as_tensor(se_p))
    assert res.converged.all() and res.status.tolist() == [1, 1]
    err = np.abs(res.x.numpy().reshape(2, N) - want)
    assert (err / np.abs(want - xa[None]).max(axis=1, keepdims=True)).max() <= 1e-10
    mean_ov = make(dict(s, se=se_p.mean(axis=0)))
    res_mean = mean_ov.retrieve(s["z"], s["p"], yt, max_iter=5, tol=1e-9)
    assert ((np.abs(res_mean.x.numpy().reshape(2, N) - want) / sigma[None]).max(axis=1) > 1e-3).all()


def test_an_indefinite_se_ends_as_status_2_with_nan(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    y = observations(st, s)
    se_p = se_batch()
    se_p[1] = -se_p[1]
    for kw in ({}, {"basis": eofs(s)}):
        ov = make(s, **kw)
        x0 = s["x_true"] if not kw else torch.zeros((NPROF, R), dtype=torch.float64)
        x_new, d = ov.step(s["z"], s["p"], x0, y, se=se_p)
        assert d["status"].tolist() == [1, 2, 1] and d["whiten_status"].tolist() == [1, 2, 1] and d["nobs"].tolist() == [M, 0, M]
        assert x_new[1].isnan().all() and d["chi2"][1].isnan() and d["dfs"][1].isnan() and d["post_var"][1].isnan().all()
        assert x_new[[0, 2]].isfinite().all() and d["post_var"][[0, 2]].isfinite().all() and d["fx"].isfinite().all()
        for res in (ov.retrieve(s["z"], s["p"], y, max_iter=3, se=se_p), ov.retrieve_lm(s["z"], s["p"], y, max_iter=3, se=se_p)):
            assert res.status.tolist() == [1, 2, 1] and not res.converged[1] and res.chi2[1].isnan() and res.post_var[1].isnan().all()
            assert res.x.isfinite().all() and res.iterations[1] <= 1     # frozen where it started
        ch = ov.characterise(s["z"], s["p"], x0, y, avk=True, se=se_p)
        assert ch.status.tolist() == [1, 2, 1] and ch.gain[1].isnan().all() and ch.avk[1].isnan().all() and ch.noise_var[1].isnan().all()
        assert ch.gain[[0, 2]].isfinite().all() and not ch.keep[1].any()


def test_shape_errors_name_the_expected_shapes(monkeypatch):
    SeStandins(monkeypatch)
    s = setup()
    ov = make(s)
    y = torch.full((NPROF, M), 255.0, dtype=torch.float64)
    good = se_batch()
    want = r"se: expected a float64 tensor \[%d\]\[%d\] or \[%d\]\[%d\]\[%d\]" % (NPROF, M, NPROF, M, M)
    for bad in (good[:2], good[:, :, :5], good.to(torch.float32), torch.ones(M, dtype=torch.float64), good.numpy()):
        for call in (lambda se: ov.step(s["z"], s["p"], s["x_true"], y, se=se),
                     lambda se: ov.retrieve(s["z"], s["p"], y, se=se), lambda se: ov.retrieve_lm(s["z"], s["p"], y, se=se),
                     lambda se: ov.characterise(s["z"], s["p"], s["x_true"], y, se=se)):
            with pytest.raises(ValueError, match=want):
                call(bad)
    f64 = torch.float64
    with pytest.raises(ValueError, match=r"k_blocks\[0\]: expected float64 \[3\]\[6\]\[4\]"):
        WHITEN([torch.zeros((3, 5, 4), dtype=f64)], torch.ones((3, 6), dtype=f64), torch.zeros((3, 6), dtype=f64), torch.zeros((3, 6), dtype=f64), None)
    with pytest.raises(ValueError, match=r"se: expected float64 \[3\]\[6\] or \[3\]\[6\]\[6\]"):
        WHITEN([torch.zeros((3, 6, 4), dtype=f64)], torch.ones((6,), dtype=f64), torch.zeros((3, 6), dtype=f64), torch.zeros((3, 6), dtype=f64), None)
    with pytest.raises(ValueError, match="representation_error needs a basis"):
        ov.representation_error(s["z"], s["p"], s["x_true"])


def test_representation_error_is_k_s_res_k_transposed(monkeypatch):
    st = SeStandins(monkeypatch)
    s = setup()
    sb = eofs(s)
    b, lam = sb.b.numpy(), np.diag(sb.sa_c.numpy())
    s_res = s["sa"] - (b * lam[None]) @ b.T
    assert np.abs(sb.sa_res.numpy() - 0.5 * (s_res + s_res.T)).max() <= 1e-13 * np.abs(s["sa"]).max()
    assert torch.equal(sb.sa_res, sb.sa_res.T) and np.linalg.eigvalsh(sb.sa_res.numpy()).min() >= -1e-12 * lam[0]
    assert retrieval.StateBasis(sb.b, sb.sa_c).sa_res is None
    for kw, grid in (({}, (FRQ, ELEV)), ({"instrument": Instrument(FRQ, ELEV, beam=3.5, band=[0.23, 0.23, 2.0], n_beam=3, n_band=2)}, None)):
        ov = make(s, basis=sb, **kw)
        st.order.clear()
        st.whiten_calls.clear()
        got = ov.representation_error(s["z"], s["p"], s["x_true"])
        assert "project" not in st.order and st.whiten_calls == [] and got.shape == (NPROF, M, M)
        inst = kw.get("instrument")
        rows = st.rows(*grid) if inst is None else st.rows(inst.frq_q, inst.elev_q)
        K = np.concatenate([rows["t"].numpy(), rows["h"].numpy()], axis=1)
        K = K if inst is None else inst.dense() @ K
        want = K @ sb.sa_res.numpy() @ K.T
        assert np.abs(got.numpy() - want[None]).max() <= 1e-12 * np.abs(want).max()
        # ready to add to a noise covariance and pass as se=
        se_p = got + torch.eye(M, dtype=torch.float64)[None] * 0.25
        c_new, d = ov.step(s["z"], s["p"], torch.zeros((NPROF, R), dtype=torch.float64), torch.full((NPROF, M), 255.0, dtype=torch.float64),
                           post_var=False, se=se_p)
        assert d["status"].tolist() == [1] * NPROF and d["whiten_status"].tolist() == [1] * NPROF
