"""selection.rank_observations end to end on the GPU: the real K-matrix call, the basis projection and
mwrt_oe_select_device, on the small synthetic case of tests/test_retrieval_nform.py (6 profiles, 40 levels, 14 channels at
2 elevations, m = 28), with the r = 8 basis of EOFs and without a basis (n = 80).  With all m picked the selection has
assimilated every observation one at a time, so its running dfs must end at the dfs of the characterisation of the n-form
step and its last S must be that step's posterior: to twice nform_reference.TOL, two routes to one posterior differing by
the rounding of a factorisation on one side and of m rank-one updates on the other."""
import numpy as np
import pytest

import nform_reference as nfr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_retrieval_nform import ELEV2, FRQ, NLEV, NPROF, R, SE, SIGMA, _dev, _post_var_err  # noqa: E402

BAR = 2 * nfr.TOL
M = FRQ.size * ELEV2.size


def _setup(basis):
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis
    P = pr.synthetic_profiles(NPROF, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, NLEV)).astype(int)
    z, p, t, rh = (_dev(np.ascontiguousarray(P[k][:, pick])) for k in ("z", "p", "t", "rh"))
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 8.0)
    sa = np.zeros((2 * NLEV, 2 * NLEV))
    for b, sig in enumerate(SIGMA):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig ** 2 * corr
    prior = torch.stack([t, rh], dim=1).contiguous()
    ov = retrieval.OneDVar("R24", FRQ, ELEV2, None if basis else _dev(sa), _dev(np.full(M, SE)),
                           variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=prior.clone(),
                           basis=StateBasis.from_covariance(torch.as_tensor(sa), R) if basis else None, form="n")
    return ov, z, p, prior


@pytest.mark.parametrize("basis", [True, False], ids=["basis", "levels"])
def test_all_picked_is_the_step(gpu_ctx, basis):
    from mwr_fast_forward_operators_and_lbls_amd import selection
    ov, z, p, prior = _setup(basis)
    x = torch.zeros((NPROF, R), dtype=torch.float64, device="cuda") if basis else prior.clone()
    y, valid = ov.forward(z, p, prior)
    assert valid.cpu().tolist() == [1] * NPROF
    y = y + _dev(np.random.default_rng(9).standard_normal(tuple(y.shape)) * np.sqrt(SE))
    sel = selection.rank_observations(ov, z, p, x, post_cov=True)
    ch = ov.characterise_nform(z, p, x, y, gain=False)
    _, d = ov.step(z, p, x, y, post_cov=True)
    torch.cuda.synchronize()
    assert sel.status.cpu().tolist() == [1] * NPROF and sel.count.cpu().tolist() == [M] * NPROF
    assert ch.status.cpu().tolist() == [1] * NPROF and d["status"].cpu().tolist() == [1] * NPROF
    order = sel.order.cpu().numpy()
    assert all(sorted(row.tolist()) == list(range(M)) for row in order) and sel.order.shape == (NPROF, M)
    assert torch.equal(sel.elev_index, sel.order // FRQ.size) and torch.equal(sel.freq_index, sel.order % FRQ.size)
    dfs = ch.dfs_block.sum(dim=1)
    err = dict(dfs=float(((sel.cum_dfs[:, -1] - dfs).abs() / dfs.abs().clamp(min=1.0)).max()),
               post_cov=float((sel.post_cov - d["post_cov"]).abs().max() / d["post_cov"].abs().max()))
    if basis:
        assert sel.post_var.shape == (NPROF, 1, R)
        err["post_var"] = float((sel.post_var.reshape(NPROF, R) - torch.diagonal(d["post_cov"], dim1=1, dim2=2)).abs().max()
                                / ov.basis.sa_c.max())
    else:
        err["post_var"] = _post_var_err(sel.post_var, d["post_var"])
    print("all picked against the step:", err, "dfs", dfs.cpu().tolist())
    assert max(err.values()) <= BAR, err
    # the picks are worth less and less, and the bits are those of q
    q = sel.q.cpu().numpy()
    assert (q > 0).all() and (np.diff(sel.cum_dfs.cpu().numpy(), axis=1) >= 0).all()
    assert torch.equal(sel.info_bits, 0.5 * torch.log2(1.0 + sel.q))
    # ranking fewer is the head of ranking all
    head = selection.rank_observations(ov, z, p, x, nsel=5)
    assert torch.equal(head.order, sel.order[:, :5]) and torch.equal(head.q, sel.q[:, :5])
    assert int(sel.first(M).sum()) == NPROF * M and sel.first(5).sum() == 5 * NPROF
