"""OneDVar(form="n") end to end on the GPU: the real K-matrix call, the instrument's reduction, the basis
projection and the n-form entries.  6 profiles, 40 levels, an r = 8 basis of EOFs, 14 channels.

form="n" is held against form="m" at 2 elevations (m = 28) to twice nform_reference.TOL -- two forms of one step differ by
the rounding of two factorisations -- in the units of oe_reference.block_errors (post_var of max diag Sa per block), and
after k iterations to k times that; at 11 elevations (m = 154) only the n-form
runs, and every profile must reach status 1."""
import numpy as np
import pytest

import nform_reference as nfr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NPROF, NLEV, R = 6, 40, 8
FRQ = np.array([22.24, 23.04, 23.84, 25.44, 26.24, 27.84, 31.4, 51.26, 52.28, 53.86, 54.94, 56.66, 57.3, 58.0])
ELEV2 = np.array([90.0, 19.2])
ELEV11 = np.array([90.0, 60.0, 42.0, 30.0, 24.0, 19.2, 15.0, 12.0, 10.2, 8.4, 7.2])
SE = 0.25
SIGMA = (2.0, 0.05)                           # prior standard deviation per block
BAR = 2 * nfr.TOL


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _setup(elev, form, **kw):
    from mwr_fast_forward_operators_and_lbls_amd import profiles as pr, retrieval
    from mwr_fast_forward_operators_and_lbls_amd._native import JacVariables
    from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis
    P = pr.synthetic_profiles(NPROF, config_id=2, nlev=180)
    pick = np.round(np.linspace(0, 150, NLEV)).astype(int)               # 40 of the 180 levels, ground to ~12 km
    P = {k: np.ascontiguousarray(v[:, pick]) for k, v in P.items()}
    z, p, t, rh = (_dev(P[k]) for k in ("z", "p", "t", "rh"))
    lev = np.arange(NLEV)
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / 8.0)
    sa = np.zeros((2 * NLEV, 2 * NLEV))
    for b, sig in enumerate(SIGMA):
        sa[b * NLEV:(b + 1) * NLEV, b * NLEV:(b + 1) * NLEV] = sig ** 2 * corr
    prior = torch.stack([t, rh], dim=1).contiguous()
    m = FRQ.size * elev.size
    ov = retrieval.OneDVar("R24", FRQ, elev, None, _dev(np.full(m, SE)), variables=JacVariables.of(humidity="rh"),
                           blocks=("t", "h"), xa=prior.clone(), basis=StateBasis.from_covariance(torch.as_tensor(sa), R), form=form, **kw)
    return ov, z, p


def _truth(ov, seed=6):
    rng = np.random.default_rng(seed)
    c_true = _dev(rng.standard_normal((NPROF, R)) * np.sqrt(np.diag(ov.basis.sa_c.numpy()))[None, :] * 0.7)
    return c_true, ov.clamp(ov.expand(c_true))


def _rel(a, b, scale):
    return float((a - b).abs().max() / scale)


def _post_var_err(a, b):
    """post_var [nprof][2][nlev] in units of max diag Sa per block."""
    return max(_rel(a[:, blk], b[:, blk], sig ** 2) for blk, sig in enumerate(SIGMA))


def test_form_n_equals_form_m_at_two_elevations(gpu_ctx):
    ov_m, z, p = _setup(ELEV2, "m")
    ov_n, _, _ = _setup(ELEV2, "n")
    c_true, x_true = _truth(ov_m)
    y, valid = ov_m.forward(z, p, x_true)
    assert valid.cpu().tolist() == [1] * NPROF
    y = y + _dev(np.random.default_rng(9).standard_normal(tuple(y.shape)) * np.sqrt(SE))
    y[2, 1, 0] = float("nan")                                            # one observation missing
    c0 = torch.zeros((NPROF, R), dtype=torch.float64, device="cuda")
    c_m, d_m = ov_m.step(z, p, c0, y)
    c_n, d_n = ov_n.step(z, p, c0, y, post_cov=True)
    torch.cuda.synchronize()
    m = FRQ.size * ELEV2.size
    assert d_n["status"].cpu().tolist() == d_m["status"].cpu().tolist() == [1] * NPROF
    assert d_n["nobs"].cpu().tolist() == d_m["nobs"].cpu().tolist() == [m, m, m - 1, m, m, m]
    sigma2 = float(ov_m.basis.sa_c.max())
    err = dict(c=_rel(c_n, c_m, c_m.abs().max()), chi2=_rel(d_n["chi2"], d_m["chi2"], max(1.0, float(d_m["chi2"].max()))),
               dfs=_rel(d_n["dfs"], d_m["dfs"], max(1.0, float(d_m["dfs"].max()))), post_var=_post_var_err(d_n["post_var"], d_m["post_var"]))
    print("step, form n against form m:", err)
    assert max(err.values()) <= BAR, err
    assert d_n["post_cov"].shape == (NPROF, R, R) and float(d_n["post_cov"].abs().max()) <= sigma2 * (1 + 1e-9)
    want = torch.einsum("kj,pji,ki->pk", ov_n._b, d_n["post_cov"], ov_n._b).reshape(NPROF, 2, NLEV)
    assert torch.equal(d_n["post_var"], want)
    for method in ("retrieve", "retrieve_lm"):
        r_m = getattr(ov_m, method)(z, p, y, max_iter=12)
        r_n = getattr(ov_n, method)(z, p, y, max_iter=12)
        torch.cuda.synchronize()
        assert r_n.iterations.cpu().tolist() == r_m.iterations.cpu().tolist() and r_n.converged.all() and r_m.converged.all()
        assert r_n.status.cpu().tolist() == [1] * NPROF and r_n.nobs.cpu().tolist() == r_m.nobs.cpu().tolist()
        its = int(r_m.iterations.max())
        err = dict(c=_rel(r_n.coeff, r_m.coeff, r_m.coeff.abs().max()), x=_rel(r_n.x, r_m.x, (r_m.x - ov_m.xa).abs().max()),
                   chi2=_rel(r_n.chi2, r_m.chi2, max(1.0, float(r_m.chi2.max()))), dfs=_rel(r_n.dfs, r_m.dfs, max(1.0, float(r_m.dfs.max()))),
                   post_var=_post_var_err(r_n.post_var, r_m.post_var))
        print(method, "form n against form m after", its, "iterations:", err)
        # every iteration adds at most one step's difference: the iteration contracts towards its fixed point, so what an
        # earlier step left is not amplified
        assert max(err.values()) <= its * BAR, err
        if method == "retrieve_lm":
            assert torch.allclose(r_n.cost, r_m.cost, rtol=1e-9, atol=0) and torch.equal(r_n.gamma, r_m.gamma)
    with pytest.raises(ValueError, match="form='m'"):
        ov_n.characterise(z, p, r_n.coeff, y)


@pytest.mark.parametrize("how", ["plain", "instrument", "ray_tracing"])
def test_form_n_serves_eleven_elevations(gpu_ctx, how):
    """m = 154: beyond MWRT_OE_MAX_M, which form="m" is refused at."""
    from mwr_fast_forward_operators_and_lbls_amd._native import MwrtError
    from mwr_fast_forward_operators_and_lbls_amd.instrument import Instrument
    kw = {}
    if how == "instrument":
        kw["instrument"] = Instrument(FRQ, ELEV11, beam=3.5, band=0.23, n_beam=3, n_band=2)
    if how == "ray_tracing":
        kw["ray_tracing"] = True
    ov, z, p = _setup(ELEV11, "n", **kw)
    m = FRQ.size * ELEV11.size
    assert ov.m == m == 154
    c_true, x_true = _truth(ov)
    y, valid = ov.forward(z, p, x_true)
    assert valid.cpu().tolist() == [1] * NPROF and y.shape == (NPROF, ELEV11.size, FRQ.size)
    res = ov.retrieve(z, p, y, max_iter=12)
    torch.cuda.synchronize()
    assert res.status.cpu().tolist() == [1] * NPROF and res.nobs.cpu().tolist() == [m] * NPROF and res.converged.all()
    r = (ov.forward(z, p, res.x)[0] - y).cpu().numpy()
    print(how, "iterations:", res.iterations.cpu().tolist(), "TB residual RMS:", float(np.sqrt((r ** 2).mean())))
    assert float(np.sqrt((r ** 2).mean())) < np.sqrt(SE)                 # noise-free observations of a truth in the span
    assert (res.dfs > 0).all() and (res.dfs <= R).all() and (res.post_var >= 0).all() and torch.isfinite(res.chi2).all()
    if how == "plain":
        lm = ov.retrieve_lm(z, p, y, max_iter=12)
        assert lm.status.cpu().tolist() == [1] * NPROF and lm.converged.all()
        ov_m, _, _ = _setup(ELEV11, "m")
        with pytest.raises(MwrtError) as ei:
            ov_m.step(z, p, res.coeff, y)
        assert ei.value.code == -5 and "140" in str(ei.value)
