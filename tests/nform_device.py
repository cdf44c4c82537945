"""The three n-form entries driven on the device for a case of tests/nform_reference.py: what tests/test_oe_nform.py and
tools/nform_errors.py share.  ``Dev`` holds a case in HBM with sentinel-filled outputs and runs prepare, solve and cost back
to back; ``reference`` is the NumPy answer to the same case; ``seeded`` caches both per shape and variant.  Needs torch with a
GPU; a helper, not a test module."""
import numpy as np
import torch

import nform_reference as nfr

IN_KEYS = ("k", "x", "xa", "se", "y", "fx")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _cur():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """A case of nform_reference.make_case on the device with every output of the three calls pre-filled with a sentinel,
    so an entry a kernel leaves unwritten shows."""

    def __init__(self, case):
        self.k = [_dev(b) for b in case["k"]]
        self.nprof, self.m, self.nlev = self.k[0].shape
        self.nblk = len(self.k)
        self.n = self.nblk * self.nlev
        self.x, self.xa, self.se, self.y, self.fx = (_dev(case[key]) for key in ("x", "xa", "se", "y", "fx"))
        self.sa_inv = _dev(nfr.sym_inv(case["sa"]))
        self.xa_pp, self.se_pp = case["xa"].ndim == 3, case["se"].ndim == 2
        self.reset()

    def reset(self):
        f64, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.uint8, device="cuda")
        nprof, m, n = self.nprof, self.m, self.n
        self.out = dict(h=torch.full((nprof, n * (n + 1) // 2), -7.0, **f64), g=torch.full((nprof, n), -7.0, **f64),
                        rwr=torch.full((nprof,), -7.0, **f64), keep=torch.full((nprof, m), 9, **u8),
                        nobs=torch.full((nprof,), -7, dtype=torch.int32, device="cuda"), lin_status=torch.full((nprof,), 9, **u8),
                        x_new=torch.full((nprof, self.nblk, self.nlev), -7.0, **f64), status=torch.full((nprof,), 9, **u8),
                        chi2=torch.full((nprof,), -7.0, **f64), dfs=torch.full((nprof,), -7.0, **f64),
                        post_var=torch.full((nprof, self.nblk, self.nlev), -7.0, **f64),
                        post_cov=torch.full((nprof, n, n), -7.0, **f64),
                        cost=torch.full((nprof,), -7.0, **f64), cost_obs=torch.full((nprof,), -7.0, **f64),
                        cost_prior=torch.full((nprof,), -7.0, **f64), cost_status=torch.full((nprof,), 9, **u8))

    def _p(self, key):
        return self.out[key].data_ptr()

    def prepare_args(self, active=None):
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, d_k=[b.data_ptr() for b in self.k], d_x=self.x.data_ptr(),
                    d_xa=self.xa.data_ptr(), d_se=self.se.data_ptr(), d_y=self.y.data_ptr(), d_fx=self.fx.data_ptr(),
                    d_h=self._p("h"), d_g=self._p("g"), d_rwr=self._p("rwr"), d_keep=self._p("keep"), d_nobs=self._p("nobs"),
                    d_lin_status=self._p("lin_status"), d_active=None if active is None else active.data_ptr(),
                    xa_per_profile=self.xa_pp, se_per_profile=self.se_pp, stream=_cur())

    def solve_args(self, gamma=None, active=None, optional=True):
        opt = dict(d_chi2=self._p("chi2"), d_dfs=self._p("dfs"), d_post_var=self._p("post_var"),
                   d_post_cov=self._p("post_cov")) if optional else {}
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, nblk=self.nblk, d_x=self.x.data_ptr(), d_xa=self.xa.data_ptr(),
                    d_sa_inv=self.sa_inv.data_ptr(), d_h=self._p("h"), d_g=self._p("g"), d_rwr=self._p("rwr"),
                    d_lin_status=self._p("lin_status"), d_x_new=self._p("x_new"), d_status=self._p("status"),
                    d_gamma=None if gamma is None else gamma.data_ptr(), d_active=None if active is None else active.data_ptr(),
                    xa_per_profile=self.xa_pp, stream=_cur(), **opt)

    def cost_args(self, active=None):
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, nblk=self.nblk, d_x=self.x.data_ptr(), d_xa=self.xa.data_ptr(),
                    d_sa_inv=self.sa_inv.data_ptr(), d_se=self.se.data_ptr(), d_y=self.y.data_ptr(), d_fx=self.fx.data_ptr(),
                    d_keep=self._p("keep"), d_cost=self._p("cost"), d_cost_obs=self._p("cost_obs"),
                    d_cost_prior=self._p("cost_prior"), d_status=self._p("cost_status"),
                    d_active=None if active is None else active.data_ptr(), xa_per_profile=self.xa_pp,
                    se_per_profile=self.se_pp, stream=_cur())

    def run(self, ctx, gamma=None, active=None, optional=None):
        """prepare, solve, cost back to back -> dict of NumPy outputs.  ``gamma``: None (a NULL d_gamma, with every optional
        output unless ``optional`` says otherwise) or one value per profile (the optional outputs keep their sentinels)."""
        g = None if gamma is None else _dev(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.nprof,)).copy())
        ctx.oe_nform_prepare_device(**self.prepare_args(active))
        ctx.oe_nform_solve_device(**self.solve_args(g, active, optional=(gamma is None) if optional is None else optional))
        ctx.oe_nform_cost_device(**self.cost_args(active))
        torch.cuda.synchronize()
        return self.host()

    def host(self):
        return {key: v.cpu().numpy() for key, v in self.out.items()}


def reference(case, gamma=None):
    ins = {key: case[key] for key in IN_KEYS}
    lin = nfr.prepare_reference(**ins)
    sol = nfr.solve_reference(sa_inv=nfr.sym_inv(case["sa"]), gamma=gamma, **ins)
    cost = nfr.cost_reference(case["x"], case["xa"], nfr.sym_inv(case["sa"]), case["se"], case["y"], case["fx"], lin["keep"])
    return lin, sol, cost


_cases = {}


def seeded(nlev, nblk, m, se_pp, xa_pp, nprof):
    key = (nlev, nblk, m, se_pp, xa_pp, nprof)
    if key not in _cases:
        case = nfr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=se_pp, xa_per_profile=xa_pp)
        gamma = np.resize(np.array(nfr.GAMMAS), nprof)
        _cases[key] = (case, gamma, reference(case), reference(case, gamma))
    return _cases[key]
