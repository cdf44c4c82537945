"""Host logic of OneDVar.retrieve_lm without a GPU: every place the method reaches the native library is replaced in this
file -- the K-matrix call by a saturating forward model on CPU tensors, F = 250 + a tanh(A v / a), and the step, prepare,
solve and cost calls by the NumPy references of tests/oe_reference.py and tests/oe_lm_reference.py (which honour the
`active` masks as the device does: a masked profile's outputs are left as they are).

The saturation is what damping is for: with a = 8 K and truths 3 sigma from the prior the undamped Gauss-Newton step
overshoots into the flat part of tanh for some profiles and ends with a cost above the one it started from."""
import numpy as np
import pytest

import oe_lm_reference as lmr
import oe_reference as oer

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd import retrieval  # noqa: E402
from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables  # noqa: E402

NLEV, NANG, NF = 6, 2, 3
M = NANG * NF
FRQ, ELEV = np.array([22.24, 31.4, 53.86]), np.array([90.0, 30.0])
# saturation amplitude [K], the truths' distance from the prior [sigma], batch: chosen (with setup's seed) by running the
# undamped loop on the CPU over a = 4, 8, 16, distances 2, 3, 4 and seeds 1 .. 3; at (8, 3, seed 2) one profile of the 20
# ends above its starting cost and does not converge
SAT, FAR, NPROF = 8.0, 3.0, 20


class Standins:
    def __init__(self, monkeypatch, sat=SAT, seed=3):
        rng = np.random.default_rng(seed)
        self.A = {b: torch.as_tensor(rng.uniform(0.2, 1.0, (M, NLEV)) * s) for b, s in (("t", 0.3), ("h", 8.0))}
        self.sat = sat
        self.solves, self.prepares, self.k_calls, self.steps = [], [], 0, 0
        for name in ("k_matrix", "oe_step", "oe_lm_prepare", "oe_lm_solve", "oe_cost"):
            monkeypatch.setattr(retrieval, "_native_" + name, getattr(self, name))

    def forward(self, t, rh):
        lin = (t - 270.0) @ self.A["t"].T + rh @ self.A["h"].T
        if self.sat is None:
            return 250.0 + lin, torch.ones_like(lin)
        return 250.0 + self.sat * torch.tanh(lin / self.sat), 1.0 / torch.cosh(lin / self.sat) ** 2

    def k_matrix(self, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
        self.k_calls += 1
        tb, slope = self.forward(t, rh)
        rows = {b: (slope[:, :, None] * self.A[b][None]).reshape(-1, NANG, NF, NLEV).contiguous() for b in want}
        return tb.reshape(-1, NANG, NF), torch.ones(t.shape[0], dtype=torch.uint8), rows

    @staticmethod
    def _k(k_blocks, nprof, nlev):
        return [k.numpy().reshape(nprof, M, nlev) for k in k_blocks]

    def oe_step(self, k_blocks, x, xa, sa, se, y, fx, want_post_var, stream):
        self.steps += 1
        nprof, nblk, nlev = x.shape
        ref = oer.oe_step_reference(self._k(k_blocks, nprof, nlev), x.numpy(), xa.numpy(), sa.numpy(), se.numpy(), y.numpy(), fx.numpy())
        return {k: torch.as_tensor(ref[k]) for k in ("x_new", "status", "chi2", "dfs", "nobs", "post_var")}

    def oe_lm_prepare(self, k_blocks, x, xa, sa, se, y, fx, lin, active, stream):
        nprof, nblk, nlev = x.shape
        ref = lmr.prepare_reference(self._k(k_blocks, nprof, nlev), x.numpy(), xa.numpy(), sa.numpy(), se.numpy(), y.numpy(), fx.numpy())
        sel = active.numpy().astype(bool)
        self.prepares.append(sel.copy())
        lin["g0"][sel] = torch.as_tensor(np.array([lmr.tri_pack(g) for g in ref["g0"]]))[sel]
        for key in ("r", "kdx", "keep", "lin_status"):
            lin[key][sel] = torch.as_tensor(ref[key])[sel]

    def oe_lm_solve(self, k_blocks, x, xa, sa, se, gamma, lin, out, active, stream):
        nprof, nblk, nlev = x.shape
        sel = active.numpy().astype(bool)
        self.solves.append(dict(x=x.clone(), gamma=gamma.clone(), active=sel.copy(), lin={k: v.clone() for k, v in lin.items()}))
        # the trial from the stored linearisation: y - F(x) = r on its rows, NaN (dropped) elsewhere
        r, keep = lin["r"].numpy(), lin["keep"].numpy().astype(bool)
        ref = lmr.solve_reference(self._k(k_blocks, nprof, nlev), x.numpy(), xa.numpy(), sa.numpy(), se.numpy(),
                                  np.where(keep, r, np.nan), np.zeros_like(r), gamma.numpy())
        out["x_new"][sel] = torch.as_tensor(ref["x_new"])[sel]
        out["status"][sel] = torch.as_tensor(ref["status"])[sel]

    def oe_cost(self, x, xa, se, y, fx, keep, sa_inv, cost, active, stream):
        ref = lmr.cost_reference(x.numpy(), xa.numpy(), se.numpy(), y.numpy(), fx.numpy(), keep.numpy(), sa_inv.numpy())
        sel = active.numpy().astype(bool)
        cost[sel] = torch.as_tensor(ref["cost"])[sel]


def setup(nprof=NPROF, far=FAR, seed=2):
    rng = np.random.default_rng(seed)
    sig = np.array([2.0, 0.1])
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 2.0)
    sa = np.zeros((2 * NLEV, 2 * NLEV))
    for b in range(2):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig[b] ** 2 * corr
    se = np.full(M, 0.25)
    xa = np.stack([np.linspace(275, 265, NLEV), np.linspace(0.7, 0.2, NLEV)])
    z = torch.as_tensor(np.tile(np.linspace(0.1, 8.0, NLEV), (nprof, 1)))
    p = torch.as_tensor(np.tile(1000.0 * np.exp(-np.linspace(0.1, 8.0, NLEV) / 8.0), (nprof, 1)))
    sign = rng.choice([-1.0, 1.0], size=(nprof, 2, 1))
    x_true = xa[None] + far * sign * sig[None, :, None] * rng.uniform(0.6, 1.0, (nprof, 2, NLEV))
    return dict(sa=sa, se=se, xa=xa, z=z, p=p, x_true=torch.as_tensor(x_true), sig=sig)


def make(s):
    return retrieval.OneDVar("R24", FRQ, ELEV, torch.as_tensor(s["sa"]), torch.as_tensor(s["se"]),
                             variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=torch.as_tensor(s["xa"]))


def cost_of(st, s, x, y):
    """J per profile, in NumPy, from the stand-in's forward model (every row kept)."""
    fx = st.forward(x[:, 0], x[:, 1])[0].numpy()
    r = y.numpy().reshape(len(x), M) - fx
    dx = x.numpy().reshape(len(x), -1) - s["xa"].reshape(-1)[None]
    return (r ** 2 / s["se"]).sum(axis=1) + np.einsum("ij,jk,ik->i", dx, np.linalg.inv(s["sa"]), dx)


def test_damping_descends_where_the_undamped_iteration_ends_above_its_start(monkeypatch):
    st = Standins(monkeypatch)
    s = setup()
    ov = make(s)
    y = st.forward(s["x_true"][:, 0], s["x_true"][:, 1])[0]
    x0 = torch.as_tensor(np.broadcast_to(s["xa"], (NPROF, 2, NLEV)).copy())
    j0 = cost_of(st, s, x0, y)
    plain = ov.retrieve(s["z"], s["p"], y, max_iter=20)
    j_plain = cost_of(st, s, plain.x, y)
    worse = int((j_plain > j0).sum())
    print("undamped: profiles ending above their starting cost:", worse, "unconverged:", int((~plain.converged).sum()))
    assert worse >= 1                                                    # the inputs do what the test is about

    res = ov.retrieve_lm(s["z"], s["p"], y, max_iter=40)
    # J at every state a profile held, recomputed here: non-increasing, ending below the start
    js = np.array([cost_of(st, s, rec["x"], y) for rec in st.solves] + [cost_of(st, s, res.x, y)])
    assert (np.diff(js, axis=0) <= 0).all(), js
    assert (js[-1] < js[0]).all() and np.array_equal(js[0], j0)
    assert np.allclose(res.cost.numpy(), js[-1], rtol=1e-12, atol=0)
    print("damped: unconverged:", int((~res.converged).sum()), "trials per profile:", res.iterations.tolist())
    assert res.converged.all()
    assert st.steps == int(plain.iterations.max()) + 1                   # retrieve's steps and the one diagnostics call
    assert res.status.tolist() == [1] * NPROF and (res.dfs > 0).all() and res.gamma.shape == (NPROF,)


def test_rejections_keep_the_state_and_gamma_follows_the_rule(monkeypatch):
    st = Standins(monkeypatch)
    s = setup()
    ov = make(s)
    y = st.forward(s["x_true"][:, 0], s["x_true"][:, 1])[0]
    up, down = 7.0, 3.0
    res = ov.retrieve_lm(s["z"], s["p"], y, max_iter=40, gamma0=0.5, up=up, down=down)
    assert (st.solves[0]["gamma"] == 0.5).all() and st.solves[0]["active"].all()
    n_rej = n_acc = n_frozen = 0
    recs = st.solves + [dict(x=res.x, gamma=res.gamma, active=np.zeros(NPROF, bool), lin=None)]
    for a, b in zip(recs, recs[1:]):
        for i in range(NPROF):
            ga, gb = float(a["gamma"][i]), float(b["gamma"][i])
            same_x = torch.equal(a["x"][i], b["x"][i])
            if not a["active"][i]:                                       # frozen: nothing of it changes
                assert gb == ga and same_x and not b["active"][i]
                n_frozen += 1
            elif gb == ga * up:                                          # rejected: x and its linearisation bit for bit
                assert same_x
                if b["lin"] is not None:
                    for key in ("g0", "r", "kdx", "keep", "lin_status"):
                        assert torch.equal(a["lin"][key][i], b["lin"][key][i]), (i, key)
                n_rej += 1
            else:                                                        # accepted
                assert gb == ga / down, (i, ga, gb)
                n_acc += 1
    print("accepted", n_acc, "rejected", n_rej, "frozen profile-iterations", n_frozen)
    assert n_rej >= 1 and n_acc >= NPROF and n_frozen >= 1
    # a linearisation is asked for only where the state changed: the first covers all, none of the later ones does
    assert st.prepares[0].all() and all(not sel.all() for sel in st.prepares[1:])
    assert torch.equal(res.gamma, recs[-1]["gamma"])


def test_gamma_beyond_its_limit_freezes_the_profile_as_failed(monkeypatch):
    st = Standins(monkeypatch)
    s = setup(nprof=3)
    ov = make(s)
    y = st.forward(s["x_true"][:3, 0], s["x_true"][:3, 1])[0]
    y[1] = 1e6                                                           # whatever the trial, J cannot fall below J(xa) ...
    x0 = torch.as_tensor(np.broadcast_to(s["xa"], (3, 2, NLEV)).copy())
    x0[2, 0, 0] = float("nan")                                           # ... and a state that cannot be linearised
    res = ov.retrieve_lm(s["z"], s["p"], y, x0=x0, max_iter=30, gamma_max=1e3)
    assert res.converged.tolist() == [True, False, False]
    assert res.iterations.tolist()[2] == 0 and res.status.tolist()[2] == 0
    assert float(res.gamma[1]) > 1e3 and torch.equal(res.x[1], x0[1])    # every trial of profile 1 was rejected
    assert res.iterations.tolist()[1] == 4                               # gamma 1, 10, 100, 1000, then beyond the limit


def test_a_linear_problem_lands_on_the_posterior_mean(monkeypatch):
    st = Standins(monkeypatch, sat=None)
    s = setup(nprof=4, far=1.0)
    ov = make(s)
    y = st.forward(s["x_true"][:, 0], s["x_true"][:, 1])[0] + 0.3 * torch.as_tensor(np.random.default_rng(9).standard_normal((4, M)))
    K = torch.cat([st.A["t"], st.A["h"]], dim=1).numpy()
    xa = s["xa"].reshape(-1)
    fxa = st.forward(torch.as_tensor(s["xa"][None, 0]), torch.as_tensor(s["xa"][None, 1]))[0].numpy()[0]
    post = np.linalg.inv(K.T @ K / 0.25 + np.linalg.inv(s["sa"]))
    want = xa[None] + (y.numpy() - fxa[None]) @ (post @ K.T / 0.25).T
    res = ov.retrieve_lm(s["z"], s["p"], y, max_iter=40, tol=1e-7)
    assert res.converged.all()
    # on a quadratic cost every trial that still moves the state descends, so gamma falls by `down` per trial (only at the
    # minimum itself, where J changes in its last bits, may a trial be rejected) and the damped steps close on the mean
    assert (res.gamma <= 1e-3).all() and (res.iterations >= 3).all()
    assert np.abs(res.x.numpy().reshape(4, -1) - want).max() <= 1e-6 * np.abs(want - xa[None]).max()
    assert np.abs(res.post_var.numpy().reshape(4, -1) - np.diag(post)[None]).max() <= 1e-10 * np.diag(s["sa"]).max()
