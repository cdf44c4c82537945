"""mwrt_oe_nform_char_device and mwrt_oe_nform_gain_device driven on the device behind prepare, for a case of
tests/nform_reference.py: what tests/test_oe_nform_char.py and tools/nform_char_errors.py share.  ``CharDev`` is
``nform_device.Dev`` with the sentinel-filled outputs of the two entries; ``reference`` is the NumPy answer to the same case;
``seeded`` caches both per shape and variant.  Needs torch with a GPU; a helper, not a test module."""
import numpy as np
import torch

import nform_char_reference as ncr
import nform_reference as nfr
from nform_device import IN_KEYS, Dev, _cur, _dev  # noqa: F401

CHAR_KEYS = ("c_status", "c_post_cov", "avk", "avk_diag", "noise_var", "smooth_var", "dfs_block")
OPTIONAL = ("c_post_cov", "avk", "avk_diag", "noise_var", "smooth_var", "dfs_block")


class CharDev(Dev):
    """A case on the device with the outputs of prepare, solve, char and gain pre-filled with sentinels.  ``rows`` is the
    window of A (None: all n rows)."""

    def __init__(self, case, rows=None):
        self.rows = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
        super().__init__(case)

    def reset(self):
        super().reset()
        f64, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.uint8, device="cuda")
        nprof, m, n = self.nprof, self.m, self.n
        self.out.update(c_status=torch.full((nprof,), 9, **u8), c_post_cov=torch.full((nprof, n, n), -7.0, **f64),
                        avk=torch.full((nprof, self.rows[1] or n, n), -7.0, **f64),
                        avk_diag=torch.full((nprof, self.nblk, self.nlev), -7.0, **f64),
                        noise_var=torch.full((nprof, self.nblk, self.nlev), -7.0, **f64),
                        smooth_var=torch.full((nprof, self.nblk, self.nlev), -7.0, **f64),
                        dfs_block=torch.full((nprof, self.nblk), -7.0, **f64), gain=torch.full((nprof, m, n), -7.0, **f64))

    def char_args(self, active=None, outputs=OPTIONAL):
        name = dict(c_post_cov="d_post_cov", avk="d_avk", avk_diag="d_avk_diag", noise_var="d_noise_var",
                    smooth_var="d_smooth_var", dfs_block="d_dfs_block")
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, nblk=self.nblk, d_sa_inv=self.sa_inv.data_ptr(),
                    d_h=self._p("h"), d_lin_status=self._p("lin_status"), d_status=self._p("c_status"),
                    d_active=None if active is None else active.data_ptr(), row_begin=self.rows[0], row_count=self.rows[1],
                    stream=_cur(), **{name[key]: self._p(key) for key in outputs})

    def gain_args(self, active=None, from_solve=False):
        return dict(nprof=self.nprof, nlev=self.nlev, m=self.m, d_k=[b.data_ptr() for b in self.k], d_se=self.se.data_ptr(),
                    d_keep=self._p("keep"), d_post_cov=self._p("post_cov" if from_solve else "c_post_cov"),
                    d_status=self._p("status" if from_solve else "c_status"), d_gain=self._p("gain"),
                    d_active=None if active is None else active.data_ptr(), se_per_profile=self.se_pp, stream=_cur())

    def characterise(self, ctx, active=None, outputs=OPTIONAL, gain=True):
        """prepare, char and (with S^ among the outputs) gain back to back -> dict of NumPy outputs."""
        ctx.oe_nform_prepare_device(**self.prepare_args(active))
        ctx.oe_nform_char_device(**self.char_args(active, outputs))
        if gain and "c_post_cov" in outputs:
            ctx.oe_nform_gain_device(**self.gain_args(active))
        torch.cuda.synchronize()
        return self.host()


def reference(case, rows=None):
    return ncr.nform_char_reference(sa_inv=nfr.sym_inv(case["sa"]), rows=rows, **{key: case[key] for key in IN_KEYS})


def as_reference(got):
    """The device outputs under the reference's names."""
    return dict(gain=got["gain"], avk=got["avk"], avk_diag=got["avk_diag"], dfs_block=got["dfs_block"],
                noise_var=got["noise_var"], smooth_var=got["smooth_var"], post_cov=got["c_post_cov"])


_cases = {}


def seeded(nlev, nblk, m, se_pp, xa_pp, nprof):
    key = (nlev, nblk, m, se_pp, xa_pp, nprof)
    if key not in _cases:
        case = nfr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=se_pp, xa_per_profile=xa_pp)
        _cases[key] = (case, reference(case))
    return _cases[key]
