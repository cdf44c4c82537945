"""OneDVar with a reduced basis end to end on the GPU: the real K-matrix call, mwrt_basis_project_device and
mwrt_basis_expand_device, and the optimal-estimation entries on the one block K B.  20 levels, two blocks (three with
liquid), 14 frequencies x 2 elevations, 4 profiles.

The bar of the r = n identity is the project's derived one (oe_reference.TOL): 1e-8 of max |x+ - xa| per block, with
cond_2(G) <= 1e4 asserted on the reference's G, built on the host from the K-matrix call's rows."""
import numpy as np
import pytest

import oe_reference as oer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NPROF, NLEV = 4, 20
FRQ = np.array([22.24, 23.04, 23.84, 25.44, 26.24, 27.84, 31.4, 51.26, 52.28, 53.86, 54.94, 56.66, 57.3, 58.0])
ELEV = np.array([90.0, 19.2])
M = FRQ.size * ELEV.size
SE = 0.25


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


def _setup(blocks=("t", "h"), basis=None, with_sa=True):
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    P = pr.synthetic_profiles(NPROF, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, NLEV)).astype(int)               # 20 of the 180 levels, ground to ~12 km
    P = {k: np.ascontiguousarray(v[:, pick]) for k, v in P.items()}
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 4.0)
    nblk = len(blocks)
    sa = np.zeros((nblk * NLEV, nblk * NLEV))
    for b, sig in enumerate((2.0, 0.05, 0.05)[:nblk]):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig ** 2 * corr
    prior = torch.stack([t, rh] + [torch.zeros_like(t)] * (nblk - 2), dim=1).contiguous()
    ov = retrieval.OneDVar("R24", FRQ, ELEV, _dev(sa) if with_sa else None, _dev(np.full(M, SE)),
                           variables=JacVariables.of(humidity="rh"), blocks=blocks, xa=prior.clone(),
                           basis=basis(sa) if basis is not None else None)
    return ov, z, p, prior, sa


def _eofs(r):
    from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis
    return lambda sa: StateBasis.from_covariance(torch.as_tensor(sa), r)


def test_step_with_all_eigenvectors_equals_the_full_state_step(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd import retrieval
    n = 2 * NLEV
    full, z, p, prior, sa = _setup()
    red, *_ = _setup(basis=_eofs(n), with_sa=False)
    b = red.basis.b.numpy()
    rng = np.random.default_rng(5)
    c = rng.standard_normal((NPROF, n)) * np.sqrt(np.diag(red.basis.sa_c.numpy()))[None, :] * 0.3
    x = red.expand(_dev(c))                                              # the same state, in both forms
    assert (x[:, 1] > 0).all()                                           # no clamp in the way: x is xa + B c exactly
    y = _dev(250.0 + 20.0 * rng.standard_normal((NPROF, ELEV.size, FRQ.size)))
    y[2, 1, 0] = float("nan")                                            # one observation missing
    x_full, d_full = full.step(z, p, x, y)
    c_new, d_red = red.step(z, p, _dev(c), y)
    x_red = red.expand(c_new)
    torch.cuda.synchronize()
    # the reference's G, for its condition number: the K-matrix call's rows on the host
    zz, t, rh, _, _ = full.physical(z, p, x)
    tb, valid, rows = retrieval._native_k_matrix("R24", zz, p, t, rh, None, None, FRQ, ELEV, full.variables, ("t", "h"), _cur())
    torch.cuda.synchronize()
    case = dict(k=[rows[k].cpu().numpy().reshape(NPROF, M, NLEV) for k in ("t", "h")], x=x.cpu().numpy(),
                xa=prior.cpu().numpy(), sa=sa, se=np.full(M, SE), y=y.cpu().numpy().reshape(NPROF, M),
                fx=tb.cpu().numpy().reshape(NPROF, M))
    ref = oer.oe_step_reference(**case)
    print("cond_2(G) per profile:", ref["cond"].tolist())
    assert valid.cpu().tolist() == [1] * NPROF and (ref["cond"] <= oer.COND_MAX).all(), ref["cond"]
    assert d_full["status"].cpu().tolist() == d_red["status"].cpu().tolist() == [1] * NPROF
    assert d_red["nobs"].cpu().tolist() == [M, M, M - 1, M]
    got = dict(x_new=x_red.cpu().numpy(), chi2=d_red["chi2"].cpu().numpy(), dfs=d_red["dfs"].cpu().numpy(),
               post_var=d_red["post_var"].cpu().numpy())
    want = dict(x_new=x_full.cpu().numpy(), chi2=d_full["chi2"].cpu().numpy(), dfs=d_full["dfs"].cpu().numpy(),
                post_var=d_full["post_var"].cpu().numpy(), status=d_full["status"].cpu().numpy())
    err = oer.block_errors(got, want, case)
    print("reduced step with r = n against the full-state step on the device:", err)
    assert all(v <= oer.TOL for v in err.values()), err
    # and both against the host reference
    err_ref = oer.block_errors(got, ref, case)
    print("... against the reference:", err_ref)
    assert all(v <= oer.TOL for v in err_ref.values()), err_ref
    assert c_new.shape == (NPROF, n) and np.abs(b.T @ b - np.eye(n)).max() <= 1e-13


def _cost_and_rms(ov, z, p, y, c):
    """Per profile J = r^T Se^-1 r + (c - c_a)^T sa_c^-1 (c - c_a) at the coefficients c, and the RMS of r over the batch."""
    r = (ov.forward(z, p, ov.clamp(ov.expand(c)))[0] - y).cpu().numpy().reshape(NPROF, -1)
    lam = np.diag(ov.basis.sa_c.cpu().numpy())
    dc = c.cpu().numpy() - ov.basis.c_a.cpu().numpy().reshape(-1, lam.size)
    return (r ** 2 / SE).sum(axis=1) + (dc ** 2 / lam[None, :]).sum(axis=1), float(np.sqrt((r ** 2).mean()))


@pytest.mark.parametrize("method", ["retrieve", "retrieve_lm"])
def test_eight_coefficients_close_on_noise_free_observations(gpu_ctx, method):
    r = 8
    ov, z, p, prior, sa = _setup(basis=_eofs(r))
    rng = np.random.default_rng(6)
    c_true = _dev(rng.standard_normal((NPROF, r)) * np.sqrt(np.diag(ov.basis.sa_c.numpy()))[None, :] * 0.7)
    x_true = ov.clamp(ov.expand(c_true))                                 # a truth inside the span of B
    y, valid = ov.forward(z, p, x_true)
    assert valid.cpu().tolist() == [1] * NPROF
    run = getattr(ov, method)
    full = run(z, p, y, max_iter=12)
    n_it = int(full.iterations.max())
    assert full.converged.all() and 2 <= n_it < 12
    zero = torch.zeros((NPROF, r), dtype=torch.float64, device="cuda")
    cost, rms = (list(v) for v in zip(_cost_and_rms(ov, z, p, y, zero)))
    for it in range(1, n_it + 1):                                        # the state after `it` iterations
        res = run(z, p, y, max_iter=it)
        j, e = _cost_and_rms(ov, z, p, y, res.coeff)
        cost.append(j)
        rms.append(e)
    print(method, "TB residual RMS per iteration:", rms)
    print(method, "cost J per iteration and profile:", [c.tolist() for c in cost])
    assert torch.equal(res.coeff, full.coeff) and torch.equal(res.x, full.x)
    assert rms[0] > np.sqrt(SE)                                          # the prior does not already fit
    assert all((b <= a).all() for a, b in zip(cost, cost[1:])), cost     # the cost never rises
    assert rms[-1] < np.sqrt(SE), rms
    assert (full.status == 1).all() and (full.nobs == M).all() and (full.x[:, 1] >= 0).all()
    assert full.x.shape == (NPROF, 2, NLEV) and full.coeff.shape == (NPROF, r) and full.post_var.shape == (NPROF, 2, NLEV)
    assert torch.equal(full.x, ov.clamp(ov.expand(full.coeff)))
    assert (full.dfs > 0).all() and (full.dfs <= r).all()
    # the level-space variance lies between 0 and what the basis carries of the prior, diag(B sa_c B^T)
    carried = torch.einsum("kj,ji,ki->k", ov._b, ov.basis.sa_c.to("cuda"), ov._b).reshape(2, NLEV)
    assert (full.post_var >= 0).all() and (full.post_var <= carried * (1 + 1e-12)).all()


def test_characterise_in_coefficient_space(gpu_ctx):
    r = 8
    ov, z, p, prior, sa = _setup(basis=_eofs(r))
    rng = np.random.default_rng(7)
    c = _dev(rng.standard_normal((NPROF, r)) * np.sqrt(np.diag(ov.basis.sa_c.numpy()))[None, :] * 0.3)
    y = _dev(250.0 + 20.0 * rng.standard_normal((NPROF, M)))
    ch = ov.characterise(z, p, c, y, avk=True, post_cov=True)
    _, d = ov.step(z, p, c, y)
    torch.cuda.synchronize()
    assert ch.status.cpu().tolist() == [1] * NPROF and ch.gain.shape == (NPROF, M, r) and ch.avk.shape == (NPROF, r, r)
    assert ch.dfs_block.shape == (NPROF, 1) and ch.avk_diag.shape == (NPROF, 1, r) and torch.equal(ch.coeff, c)
    dfs = ch.dfs_block.sum(dim=1)
    assert (dfs <= r).all() and (dfs > 0).all()
    assert torch.allclose(dfs, d["dfs"], rtol=oer.TOL, atol=0)           # the sum over blocks is the step's dfs
    assert torch.allclose(torch.diagonal(ch.avk, dim1=1, dim2=2).sum(dim=1), dfs, rtol=oer.TOL, atol=0)
    # the step's level-space post_var is the diagonal of B S^_c B^T
    want = torch.einsum("kj,pji,ki->pk", ov._b, ch.post_cov, ov._b).reshape(NPROF, 2, NLEV)
    assert torch.allclose(d["post_var"], want, rtol=1e-10, atol=0)


def test_one_column_retrieves_the_scale_of_a_liquid_profile(gpu_ctx):
    from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis
    shape = np.zeros(NLEV)
    shape[3:6] = 0.1                                                     # g m-3 in three levels: the cloud of scale 1
    b = np.zeros((3 * NLEV, 1))
    b[2 * NLEV:, 0] = shape
    sigma = 2.0
    basis = lambda sa: StateBasis(torch.as_tensor(b), torch.as_tensor([[sigma ** 2]]).to(torch.float64), c_a=torch.ones(1, dtype=torch.float64))  # noqa: E731
    ov, z, p, prior, _ = _setup(blocks=("t", "h", "liq"), basis=basis, with_sa=False)
    c_true = _dev(np.array([[0.5], [1.0], [1.5], [2.0]]))
    y, valid = ov.forward(z, p, ov.expand(c_true))
    assert valid.cpu().tolist() == [1] * NPROF
    tol = 1e-3
    res = ov.retrieve(z, p, y, max_iter=12, tol=tol)
    k_c, _ = ov._linearise(z, p, res.coeff.reshape(NPROF, 1, 1))
    torch.cuda.synchronize()
    assert res.converged.all() and (res.status == 1).all()
    # at the fixed point (c^ - c_true) (1 + sigma^2 sum K K~ / Se) = c_a - c_true with K~ the mean slope between c^ and the
    # truth; a factor 2 for K~ against K at c^, and the convergence criterion tol sigma on top
    info = sigma ** 2 * (k_c[0].reshape(NPROF, M) ** 2).sum(dim=1) / SE
    bound = 2.0 * (1.0 - c_true[:, 0]).abs() / (1.0 + info) + tol * sigma
    err = (res.coeff[:, 0] - c_true[:, 0]).abs()
    print("scale factor retrieved:", res.coeff[:, 0].cpu().tolist(), "error:", err.cpu().tolist(), "bound:", bound.cpu().tolist())
    assert (err <= bound).all()
    assert torch.equal(res.x[:, :2], prior[:, :2])                       # no column reaches T or humidity
    assert torch.allclose(res.x[:, 2], res.coeff * _dev(shape)[None, :], rtol=1e-14, atol=0)
    assert (res.dfs > 0.9).all() and (res.dfs <= 1.0 + 1e-9).all()     # one coefficient, all but fully determined
