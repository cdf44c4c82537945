"""Units do not matter, bit for bit.  With D a diagonal of powers of two on the state and E one on the observation rows,

    K -> E K D^-1,  x, xa -> D x, D xa,  Sa -> D Sa D,  Sa^-1 -> D^-1 Sa^-1 D^-1,  y, F -> E y, E F,  Se -> E Se E

is the same problem in other units: every product, fma, division and square root scales exactly and every sum keeps its
order, so each device output must be the unscaled one times its own power of two (oe_exact_reference.rescale_outputs), bit
for bit -- no reference and no tolerance.  Exponents are drawn in [-40, 40] per block and element and per row: far from
overflow, and the seeded data has no subnormals.  A failure means a kernel holds an absolute threshold or a range-limited
helper, and states in kg/kg beside states in ppmv are not safe in it.

tests/test_oe_exact_reference.py applies the same transformation to the float64 references on the CPU."""
import numpy as np
import pytest

import nform_reference as nfr
import oe_exact_reference as ex
import oe_reference as oer
import whiten_reference as whr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def _assert_same(got, want, keys, label):
    for key in keys:
        pairs = zip(got[key], want[key]) if isinstance(want[key], list) else [(got[key], want[key])]
        for q, (a, b) in enumerate(pairs):
            assert np.isfinite(b).all() if b.dtype == np.float64 else True, (label, key)
            assert _same_bits(a, b), (label, key, q, int((np.asarray(a) != np.asarray(b)).sum()))


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_m_form_step_and_gain(gpu_ctx, se_full):
    import oe_conditioning_device as ocd
    nlev, nblk, m = 65, 2, 98
    case = oer.make_case(nlev, nblk, m, nprof=2, se_full=se_full)
    D, E = ex.unit_exponents(nblk, nlev, m)
    plain = ocd.run_mform(gpu_ctx, case, gain=True)
    scaled = ocd.run_mform(gpu_ctx, ex.rescale_case(case, D, E, se_full), gain=True)
    assert plain["status"].tolist() == [1, 1] and plain["gain_status"].tolist() == [1, 1]
    _assert_same(scaled, ex.rescale_outputs(plain, D, E), ("x_new", "status", "chi2", "dfs", "post_var", "nobs", "gain_status",
                                                         "keep") + ex.GAIN_OUT, ("m-form", se_full))


@pytest.mark.parametrize("gamma", [None, 0.5], ids=["g0", "damped"])
@pytest.mark.parametrize("se_pp", [False, True], ids=["shared", "perprofile"])
def test_n_form_prepare_solve_cost(gpu_ctx, se_pp, gamma):
    import oe_conditioning_device as ocd
    nlev, nblk, m = 43, 2, 60
    case = nfr.make_case(nlev, nblk, m, nprof=2, se_per_profile=se_pp)
    case["sa_inv"] = nfr.sym_inv(case["sa"])
    D, E = ex.unit_exponents(nblk, nlev, m)
    other = ex.rescale_case(case, D, E, False)
    plain = ocd.run_nform(gpu_ctx, case, gamma=gamma, sa_inv=case["sa_inv"])
    scaled = ocd.run_nform(gpu_ctx, other, gamma=gamma, sa_inv=other["sa_inv"])
    assert plain["status"].tolist() == [1, 1] and plain["lin_status"].tolist() == [1, 1] and plain["cost_status"].tolist() == [1, 1]
    keys = ("h", "g", "rwr", "keep", "nobs", "lin_status", "x_new", "status", "cost", "cost_obs", "cost_prior", "cost_status")
    if gamma is None:
        keys += ("chi2", "dfs", "post_var", "post_cov")
    _assert_same(scaled, ex.rescale_outputs(plain, D, E), keys, ("n-form", se_pp, gamma))


@pytest.mark.parametrize("se_full", [False, True], ids=["diag", "full"])
def test_whitening_and_apply(gpu_ctx, se_full):
    import test_whiten as twh
    shape = (65, 2, 65)
    nlev, nblk, m = shape
    case = whr.make_case(shape, se_full=se_full, nprof=2)
    D, E = ex.unit_exponents(nblk, nlev, m)
    other = ex.rescale_case(case, D, E, se_full)
    keys = ("l", "keep", "status", "y_out", "fx_out", "k_out")
    plain = twh.whiten(gpu_ctx, case["k"], case["se_p"], case["y"], case["fx"])
    scaled = twh.whiten(gpu_ctx, other["k"], other["se_p"], other["y"], other["fx"])
    assert plain["status"].tolist() == [1, 1]
    want = ex.rescale_outputs(plain, D, E)
    _assert_same(scaled, want, keys, ("whiten", se_full))
    for mode in (0, 1):                                  # L^-1 and L^-T with the stored factors
        v, b = twh.apply(gpu_ctx, plain["l"], plain["keep"], mode, vecs=(case["y"], case["fx"]), blocks=case["k"])
        if mode == 0:
            vs, bs = twh.apply(gpu_ctx, scaled["l"], scaled["keep"], 0, vecs=(other["y"], other["fx"]), blocks=other["k"])
            exp_v, exp_b = v, ex.rescale_outputs(dict(k_out=b), D, E)["k_out"]
        else:                                            # L^-T v: v in whitened units comes back divided by E
            vs, bs = twh.apply(gpu_ctx, scaled["l"], scaled["keep"], 1, vecs=(case["y"], case["fx"]), blocks=case["k"])
            exp_v, exp_b = [a / E for a in v], [a / E[None, :, None] for a in b]
        for q, (a, w) in enumerate(zip(list(vs) + list(bs), list(exp_v) + list(exp_b))):
            assert np.isfinite(w).all() and _same_bits(a, w), ("apply", se_full, mode, q)
