"""tests/basis_reference.py held to exact rational arithmetic on small cases, and the algebra the reduced basis rests on,
with tests/oe_reference.py: a step in the coefficients on (K B, sa_c) is the full-state m-form step with Sa = B sa_c B^T, and
with all n eigenvectors of Sa it is the full-state step with Sa itself.

The bar of the identities is the project's derived one (oe_reference.TOL): 1e-8 of max |x+ - xa| per block, with
cond_2(G) <= 1e4 asserted on the reference's G of every profile."""
from fractions import Fraction

import numpy as np
import pytest

import basis_reference as bar
import oe_reference as oer

torch = pytest.importorskip("torch")

from mwr_fast_forward_operators_and_lbls_amd.retrieval import StateBasis  # noqa: E402


@pytest.mark.parametrize("shape", [(2, 3, 5, 1, 4), (1, 2, 17, 2, 3), (2, 1, 1, 4, 1)])
def test_reference_against_exact_rational_sums(shape):
    c = bar.make_case(*shape)
    nprof, m, nlev, nblk, r = shape
    n = nblk * nlev
    got, scale = bar.project_reference(c["k"], c["b"])
    k = np.concatenate(c["k"], axis=2)
    for p in range(nprof):
        for i in range(m):
            for j in range(r):
                exact = sum(Fraction(float(k[p, i, l])) * Fraction(float(c["b"][l, j])) for l in range(n))
                assert abs(Fraction(float(got[p, i, j])) - exact) <= Fraction(n * bar.U) * Fraction(float(scale[p, i, j])), (p, i, j)
    assert (scale[:, m - 1] == 0).all() and (got[:, m - 1] == 0).all()      # the zero row of the recipe
    for x_ref in (c["x_ref"], np.stack([c["x_ref"] + i for i in range(nprof)])):
        x, s = bar.expand_reference(c["b"], c["c"], x_ref)
        xr = np.broadcast_to(x_ref.reshape(-1, n), (nprof, n))
        for p in range(nprof):
            for q in range(n):
                exact = Fraction(float(xr[p, q])) + sum(Fraction(float(c["b"][q, j])) * Fraction(float(c["c"][p, j])) for j in range(r))
                # r products and r additions onto x_ref: gamma_(r + 1)
                assert abs(Fraction(float(x[p, q])) - exact) <= Fraction((r + 1) * bar.U) * Fraction(float(s[p, q])), (p, q)


def _blockwise(got, ref, xa, nblk):
    """Largest |got - ref| per block in units of that block's max |ref - xa|; a block the basis leaves at xa (no column of
    B reaches it) has to stay there exactly."""
    nprof = ref.shape[0]
    got, ref, xa = (np.broadcast_to(a, ref.shape).reshape(nprof, nblk, -1) for a in (got, ref, xa))
    worst = 0.0
    for i in range(nprof):
        for b in range(nblk):
            scale = np.abs(ref[i, b] - xa[i, b]).max()
            if scale == 0.0:
                assert np.array_equal(got[i, b], ref[i, b]), (i, b)
            else:
                worst = max(worst, float(np.abs(got[i, b] - ref[i, b]).max() / scale))
    return worst


@pytest.mark.parametrize("nlev,nblk,m,r", [(33, 1, 17, 8), (20, 2, 40, 8), (65, 2, 98, 32), (20, 2, 14, 1)])
def test_step_in_coefficients_equals_the_full_step_with_the_projected_prior(nlev, nblk, m, r):
    case = oer.make_case(nlev, nblk, m, nprof=2)
    n = nblk * nlev
    sb = StateBasis.from_covariance(torch.as_tensor(case["sa"]), r)
    b, sa_c = sb.b.numpy(), sb.sa_c.numpy()
    xa = case["xa"].reshape(n)
    c = (case["x"].reshape(2, n) - xa) @ b                                # B^T B = I: the coefficients of the part inside the span
    x = xa + c @ b.T
    full = oer.oe_step_reference(case["k"], x.reshape(2, nblk, nlev), case["xa"], b @ sa_c @ b.T, case["se"], case["y"], case["fx"])
    k_c, _ = bar.project_reference(case["k"], b)
    red = oer.oe_step_reference([k_c], c[:, None, :], np.zeros((1, r)), sa_c, case["se"], case["y"], case["fx"])
    assert full["status"].tolist() == red["status"].tolist() == [1, 1]
    assert (full["cond"] <= oer.COND_MAX).all() and (red["cond"] <= oer.COND_MAX).all(), (full["cond"], red["cond"])
    x_red = bar.expand_reference(b, red["x_new"].reshape(2, r), xa)[0]
    err = _blockwise(x_red, full["x_new"].reshape(2, n), xa, nblk)
    print("x_ref + B c+ against the full step with Sa = B sa_c B^T:", err)
    assert err <= oer.TOL
    assert np.abs(red["chi2"] - full["chi2"]).max() <= oer.TOL * max(1.0, np.abs(full["chi2"]).max())
    assert np.abs(red["dfs"] - full["dfs"]).max() <= oer.TOL * max(1.0, np.abs(full["dfs"]).max())
    # diag(B S^_c B^T) is the full step's posterior variance
    pv = np.stack([np.diag(b @ (sa_c - z) @ b.T) for z in _reduction(k_c, sa_c, case["se"])])
    assert np.abs(pv - full["post_var"].reshape(2, n)).max() <= oer.TOL * np.diag(case["sa"]).max()


def _reduction(k_c, sa_c, se):
    """Sa_c K^T G^-1 K Sa_c per profile (what the posterior covariance of the coefficients takes off sa_c)."""
    for k in k_c:
        w = k @ sa_c
        yield w.T @ np.linalg.solve(w @ k.T + np.diag(se), w)


@pytest.mark.parametrize("nlev,nblk,m", [(33, 1, 17), (20, 2, 14), (20, 4, 40)])
def test_all_eigenvectors_give_the_full_state_step(nlev, nblk, m):
    case = oer.make_case(nlev, nblk, m, nprof=2)
    n = nblk * nlev
    sb = StateBasis.from_covariance(torch.as_tensor(case["sa"]), n)
    b, sa_c = sb.b.numpy(), sb.sa_c.numpy()
    assert np.abs(b @ sa_c @ b.T - case["sa"]).max() <= 1e-12 * np.abs(case["sa"]).max()
    xa = case["xa"].reshape(n)
    c = (case["x"].reshape(2, n) - xa) @ b
    full = oer.oe_step_reference(case["k"], case["x"], case["xa"], case["sa"], case["se"], case["y"], case["fx"])
    k_c, _ = bar.project_reference(case["k"], b)
    red = oer.oe_step_reference([k_c], c[:, None, :], np.zeros((1, n)), sa_c, case["se"], case["y"], case["fx"])
    assert full["status"].tolist() == red["status"].tolist() == [1, 1]
    assert (full["cond"] <= oer.COND_MAX).all() and (red["cond"] <= oer.COND_MAX).all()
    err = _blockwise(bar.expand_reference(b, red["x_new"].reshape(2, n), xa)[0], full["x_new"].reshape(2, n), xa, nblk)
    print("r = n, x_ref + B c+ against the full-state step:", err)
    assert err <= oer.TOL
