"""retrieval.OneDVar with an instrument, without a GPU: the seams to the native library are replaced as in
tests/test_retrieval_cpu.py -- the K-matrix call by a small linear forward model on whatever (frequency, elevation) grid it is
asked for, the update by the NumPy reference of tests/oe_reference.py, the instrument's reduction by the NumPy reference of
tests/obs_reference.py.  What is checked is the module's own work: with ``instrument=None`` nothing reaches the seams that
did not before; with an instrument the K-matrix call runs on the quadrature grid, the update sees channel rows, and a
linear problem lands on the analytic posterior mean in channel space."""
import numpy as np
import pytest

import obs_reference as obr
import oe_reference as oer

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd import retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument  # noqa: E402

NPROF, NLEV = 3, 6
FRQ, ELEV = np.array([22.24, 31.4, 53.86]), np.array([90.0, 30.0])
M = FRQ.size * ELEV.size


class Standins:
    """F(node) = 250 + sum_b A_b(node) . v_b with v = (t - 270, rh); the rows A_b of a node are a smooth function of its
    frequency and elevation, so the same model answers on any grid."""

    def __init__(self, monkeypatch):
        rng = np.random.default_rng(5)
        self.base = {b: rng.uniform(0.2, 1.0, NLEV) * s for b, s in (("t", 0.3), ("h", 8.0))}
        self.k_calls, self.step_calls, self.obs_calls = [], [], []
        monkeypatch.setattr(retrieval, "_native_k_matrix", self.k_matrix)
        monkeypatch.setattr(retrieval, "_native_oe_step", self.oe_step)
        monkeypatch.setattr(retrieval, "_native_obs_apply", self.obs_apply)

    def rows(self, frq, elev):
        """{block: [nang * nf][nlev]} on a grid, angle-major."""
        lev = np.arange(NLEV)
        shape = 1.0 / np.sin(np.radians(elev))[:, None, None] * (1.0 + 0.02 * (frq[None, :, None] - 30.0)) \
            * np.exp(-lev[None, None, :] * (frq[None, :, None] / 120.0))
        return {b: torch.as_tensor((shape * a[None, None, :]).reshape(-1, NLEV)) for b, a in self.base.items()}

    def forward(self, t, rh, frq, elev):
        a = self.rows(frq, elev)
        return 250.0 + (t - 270.0) @ a["t"].T + rh @ a["h"].T

    def k_matrix(self, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
        self.k_calls.append(dict(args=(model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream)))
        a = self.rows(frq, elev)
        nprof = t.shape[0]
        rows = {b: a[b][None].expand(nprof, -1, -1).reshape(nprof, elev.size, frq.size, NLEV).contiguous() for b in want}
        return self.forward(t, rh, frq, elev).reshape(nprof, elev.size, frq.size), torch.ones(nprof, dtype=torch.uint8), rows

    def oe_step(self, k_blocks, x, xa, sa, se, y, fx, want_post_var, stream):
        self.step_calls.append(dict(k=[k.clone() for k in k_blocks], y=y.clone(), fx=fx.clone(), args=(x, xa, sa, se, stream)))
        nprof, nblk, nlev = x.shape
        m = y.shape[1]
        ref = oer.oe_step_reference([k.numpy().reshape(nprof, m, nlev) for k in k_blocks], x.numpy(), xa.numpy(), sa.numpy(),
                                    se.numpy(), y.numpy(), fx.numpy())
        out = {k: torch.as_tensor(ref[k]) for k in ("x_new", "status", "chi2", "dfs", "nobs", "post_var")}
        if not want_post_var:
            out["post_var"] = None
        return out

    def obs_apply(self, inst, tb, k_blocks, stream):
        self.obs_calls.append(dict(tb=tb, k=k_blocks))
        nang, nch = inst.elev.size, inst.frq.size
        run = lambda x, tail: torch.as_tensor(obr.apply_reference(      # noqa: E731
            inst.row_ptr, inst.col, inst.w, x.numpy().reshape((x.shape[0], inst.m_in) + tail))[0]).reshape((-1, nang, nch) + tail)
        return (None if tb is None else run(tb, ()),
                None if k_blocks is None else [run(k, (k.shape[-1],)) for k in k_blocks])


def setup(nprof=NPROF, seed=1):
    rng = np.random.default_rng(seed)
    sig = np.array([2.0, 0.1])
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 2.0)
    sa = np.zeros((2 * NLEV, 2 * NLEV))
    for b in range(2):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig[b] ** 2 * corr
    xa = np.stack([np.linspace(285, 250, NLEV), np.linspace(0.7, 0.2, NLEV)])
    z = torch.as_tensor(np.tile(np.linspace(0.1, 8.0, NLEV), (nprof, 1)))
    p = torch.as_tensor(np.tile(1000.0 * np.exp(-np.linspace(0.1, 8.0, NLEV) / 8.0), (nprof, 1)))
    x_true = xa[None] + rng.standard_normal((nprof, 2, NLEV)) * sig[None, :, None] * 0.5
    return dict(sa=sa, se=np.full(M, 0.25), xa=xa, z=z, p=p, x_true=torch.as_tensor(x_true))


def make(s, **kw):
    return retrieval.OneDVar("R24", FRQ, ELEV, torch.as_tensor(s["sa"]), torch.as_tensor(s["se"]),
                             variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=torch.as_tensor(s["xa"]), **kw)


def test_without_an_instrument_the_seams_see_what_they_saw(monkeypatch):
    st = Standins(monkeypatch)
    s = setup()
    ov = make(s)
    assert ov.instrument is None and ov.m == M
    y = torch.full((NPROF, ELEV.size, FRQ.size), 255.0, dtype=torch.float64)
    x_new, d = ov.step(s["z"], s["p"], s["x_true"], y)
    tb, valid = ov.forward(s["z"], s["p"], s["x_true"])
    k_blocks, fx = ov._linearise(s["z"], s["p"], s["x_true"])
    assert st.obs_calls == [] and len(st.k_calls) == 3 and len(st.step_calls) == 1
    for call in st.k_calls:                                              # the positional arguments of today, on the centre grid
        model, z, p, t, rh, dl, di, frq, elev, variables, want, stream = call["args"]
        assert model == "R24" and frq is ov.frq and elev is ov.elev and variables is ov.variables and want == ("t", "h")
        assert dl is None and di is None and stream is None
        assert torch.equal(z, s["z"]) and torch.equal(p, s["p"]) and torch.equal(t, s["x_true"][:, 0])
    # the update got the K-matrix call's own tensors: 4-D rows, TBs flattened to [nprof][m]
    c = st.step_calls[0]
    assert [tuple(k.shape) for k in c["k"]] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2 and c["fx"].shape == (NPROF, M)
    assert torch.equal(c["fx"], st.forward(s["x_true"][:, 0], st.k_calls[0]["args"][4], FRQ, ELEV))
    assert c["args"][1] is ov.xa and c["args"][2] is ov.sa and c["args"][3] is ov.se
    assert tb.shape == (NPROF, ELEV.size, FRQ.size) and torch.equal(fx, tb.reshape(NPROF, M)) and torch.equal(d["fx"], fx)
    assert [tuple(k.shape) for k in k_blocks] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2 and valid.tolist() == [1] * NPROF


def test_with_an_instrument_the_update_sees_channel_rows(monkeypatch):
    st = Standins(monkeypatch)
    s = setup()
    inst = Instrument(FRQ, ELEV, beam=3.5, band=[0.23, 0.23, 2.0], n_beam=3, n_band=2)
    ov = make(s, instrument=inst)
    assert ov.m == inst.m_out == M and inst.m_in == 6 * 6
    y = torch.full((NPROF, ELEV.size, FRQ.size), 255.0, dtype=torch.float64)
    x_new, d = ov.step(s["z"], s["p"], s["x_true"], y)
    # the K-matrix seam was asked for the quadrature grid, everything else as before
    args = st.k_calls[0]["args"]
    assert args[7] is inst.frq_q and args[8] is inst.elev_q and args[10] == ("t", "h") and args[0] == "R24"
    # the reduction got the TBs and both blocks, and the update got dense() @ the stand-in's rows
    assert len(st.obs_calls) == 1 and st.obs_calls[0]["tb"].shape == (NPROF, 6, 6) and len(st.obs_calls[0]["k"]) == 2
    c = st.step_calls[0]
    grid = st.rows(inst.frq_q, inst.elev_q)
    w = inst.dense()
    for got, b in zip(c["k"], ("t", "h")):
        want = w @ grid[b].numpy()                                       # [m_out][nlev]
        assert got.shape == (NPROF, ELEV.size, FRQ.size, NLEV)
        assert np.abs(got.numpy().reshape(NPROF, M, NLEV) - want[None]).max() <= 1e-13 * np.abs(want).max()
    tb_grid = st.forward(s["x_true"][:, 0], st.k_calls[0]["args"][4], inst.frq_q, inst.elev_q).numpy()
    assert c["fx"].shape == (NPROF, M) and np.abs(c["fx"].numpy() - tb_grid @ w.T).max() <= 1e-12 * 300.0
    assert c["y"].shape == (NPROF, M) and d["fx"].shape == (NPROF, M) and x_new.shape == (NPROF, 2, NLEV)
    # the channel rows differ from the centre rows: the beam and the band do something in this stand-in
    centre = st.rows(FRQ, ELEV)["t"].numpy()
    assert np.abs(c["k"][0].numpy().reshape(NPROF, M, NLEV)[0] - centre).max() > 1e-3 * np.abs(centre).max()


def test_forward_asks_for_no_k_reduction(monkeypatch):
    st = Standins(monkeypatch)
    s = setup()
    inst = Instrument(FRQ, ELEV, beam=3.5, band=0.23)
    ov = make(s, instrument=inst)
    tb, valid = ov.forward(s["z"], s["p"], s["x_true"])
    assert len(st.obs_calls) == 1 and st.obs_calls[0]["k"] is None and st.obs_calls[0]["tb"] is not None
    assert tb.shape == (NPROF, ELEV.size, FRQ.size) and valid.shape == (NPROF,)
    k_blocks, fx = ov._linearise(s["z"], s["p"], s["x_true"])
    assert len(st.obs_calls) == 2 and len(st.obs_calls[1]["k"]) == 2 and torch.equal(fx, tb.reshape(NPROF, M))
    assert [tuple(k.shape) for k in k_blocks] == [(NPROF, ELEV.size, FRQ.size, NLEV)] * 2


def test_linear_problem_reaches_the_posterior_mean_in_channel_space(monkeypatch):
    st = Standins(monkeypatch)
    s = setup()
    inst = Instrument(FRQ, ELEV, beam=3.5, band=0.23, n_beam=3, n_band=3)
    ov = make(s, instrument=inst)
    w = inst.dense()
    grid = st.rows(inst.frq_q, inst.elev_q)
    K = w @ np.concatenate([grid["t"].numpy(), grid["h"].numpy()], axis=1)          # the channel Jacobian [m][n]
    rh_true = ov.physical(s["z"], s["p"], s["x_true"])[2]
    y = st.forward(s["x_true"][:, 0], rh_true, inst.frq_q, inst.elev_q).numpy() @ w.T \
        + 0.3 * np.random.default_rng(9).standard_normal((NPROF, M))
    xa = s["xa"].reshape(-1)
    xa_t = torch.as_tensor(s["xa"][None])
    fxa = (st.forward(xa_t[:, 0], ov.physical(s["z"][:1], s["p"][:1], xa_t)[2], inst.frq_q, inst.elev_q).numpy() @ w.T)[0]
    post = np.linalg.inv(K.T @ K / 0.25 + np.linalg.inv(s["sa"]))
    want = xa[None] + (y - fxa[None]) @ (post @ K.T / 0.25).T
    x_new, d = ov.step(s["z"], s["p"], s["x_true"] + 0.3, torch.as_tensor(y).reshape(NPROF, ELEV.size, FRQ.size))
    assert np.abs(x_new.numpy().reshape(NPROF, -1) - want).max() <= 1e-10 * np.abs(want - xa[None]).max()
    assert np.abs(d["post_var"].numpy().reshape(NPROF, -1) - np.diag(post)[None]).max() <= 1e-10 * np.diag(s["sa"]).max()
    # a retrieval that ignores the instrument lands elsewhere: the centre Jacobian is not the channel Jacobian
    plain = make(s)
    x_plain, _ = plain.step(s["z"], s["p"], s["x_true"] + 0.3, torch.as_tensor(y).reshape(NPROF, ELEV.size, FRQ.size))
    assert np.abs(x_plain.numpy().reshape(NPROF, -1) - want).max() > 1e-3 * np.abs(want - xa[None]).max()
    res = ov.retrieve(s["z"], s["p"], torch.as_tensor(y), max_iter=5, tol=1e-6)
    assert res.iterations.tolist() == [2] * NPROF and res.converged.all()
    assert np.abs(res.x.numpy().reshape(NPROF, -1) - want).max() <= 1e-9 * np.abs(want - xa[None]).max()
