"""Runs the columns of tests/rte_cases.py through the two K2 entries on the device and holds the TBs to tests/rte_reference.py.
tests/test_rte_columns.py (GPU) and tools/rte_column_errors.py share it.  CHECKS maps a case name to a function
(ctx, report=None) -> rows in the format of rte_reference.check."""
import functools

import numpy as np

import rte_cases as rc
import rte_reference as rr

MODEL = "R24"


def run(ctx, case):
    """-> (TB [nprof][nang][nf] float64, valid [nprof] uint8 after the call).  The tau entry reads `valid`; its array is
    uploaded with the case's flags and must come back unchanged.  The alpha entry writes it: it starts as 7."""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    t = torch.from_numpy(case.t).to(dev)
    out = torch.full((case.nprof, case.nang, case.nf), -777.0, dtype=torch.float64, device=dev)
    if case.entry == "tau":
        pitch = ctx.layer_tau_pitch(case.nf) + case.pitch_extra
        tau = np.full((case.nprof, case.nlev, pitch), np.nan)          # scratch columns [nf, pitch): never read into a result
        tau[:, :, :case.nf] = case.tau
        d_tau = torch.from_numpy(tau).to(dev)
        val = torch.from_numpy(case.valid.copy()).to(dev)
        torch.cuda.synchronize()
        ctx.tb_from_layer_tau_device(MODEL, case.nprof, case.nlev, d_tau.data_ptr(), pitch, t.data_ptr(), case.frq, case.elev,
                                     val.data_ptr(), out.data_ptr(), stream=st)
    else:
        z, aw, ad = (torch.from_numpy(a).to(dev) for a in (case.z, case.awet, case.adry))
        val = torch.full((case.nprof,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.tb_from_absorption_device(MODEL, case.nprof, case.nlev, z.data_ptr(), t.data_ptr(), case.frq, case.elev, aw.data_ptr(),
                                      ad.data_ptr(), out.data_ptr(), val.data_ptr(), stream=st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), val.cpu().numpy()


@functools.lru_cache(maxsize=None)
def cached_run(ctx, name):
    tb, valid = run(ctx, rc.table()[name])
    tb.setflags(write=False)
    valid.setflags(write=False)
    return tb, valid


def oracle_tb(case):
    """lo.planck_down + lo.bright in double on the case's columns (the tau the device is given; for the alpha entry the
    reference's layer values rounded to double): [nprof][nang][nf], NaN where the contract says NaN"""
    import warnings
    from mwr_fast_forward_operators_and_lbls_amd import spectroscopy as sp
    from oracle import lbl_oracle as lo
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = sp.get_model(MODEL)
    tau = np.asarray(case.tau_ld, dtype=np.float64)
    out = np.full((case.nprof, case.nang, case.nf), np.nan)
    skip = case.nan_expected()
    with np.errstate(all="ignore"):
        for p in range(case.nprof):
            for a in range(case.nang):
                for j in range(case.nf):
                    if skip[p, a, j]:
                        continue
                    boftotl, _, _, _, hvk = lo.planck_down(m, case.frq[j], case.t[p], tau[p, :, j] * case.am[a])
                    out[p, a, j] = lo.bright(hvk, boftotl)
    return out


def check_case(name, tb, valid, report=None, label=None):
    case = rc.table()[name]
    assert np.array_equal(valid, case.valid_expected), (name, valid, case.valid_expected)
    ref = case.reference
    src = "rte_reference.py: derived, %s entry" % case.entry
    return [rr.check(label or name, tb, ref["tb"], ref["bar"], src, report, nan_expected=case.nan_expected())]


def device_check(name, ctx, report=None):
    tb, valid = cached_run(ctx, name)
    return check_case(name, tb, valid, report)


CHECKS = {name: functools.partial(device_check, name) for name in rc.names(held=True)}
