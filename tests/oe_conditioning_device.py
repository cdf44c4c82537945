"""The cases of tests/oe_exact_reference.py driven on the device: what tests/test_oe_conditioning.py, tests/test_oe_scaling.py
and tools/oe_conditioning_errors.py share.  Each ``run_*`` takes a case and returns the device's outputs under the keys of
the exact reference; each ``*_device_errors`` returns, per profile, the errors of every output in the family's units.  The
callers of the entries are those of the families' own tests (test_oe_step.run_device, test_oe_char.run_gain,
test_oe_lm.Dev, nform_device.Dev, test_whiten.whiten / apply).  Needs torch with a GPU; a helper, not a test module."""
import numpy as np

import nform_device as nfd
import oe_exact_reference as ex
import test_oe_char as toc
import test_oe_lm as tlm
import test_oe_step as tos
import test_whiten as twh


def run_mform(ctx, case, gamma=None, gain=False):
    """mwrt_oe_step_device (gamma None; with ``gain`` also mwrt_oe_gain_device) or the mwrt_oe_lm_* pair at ``gamma``."""
    if gamma is not None:
        got = tlm.Dev(case, gamma=gamma).run(ctx)
        return {key: got[key] for key in ("x_new", "status", "chi2", "nobs")}
    got = tos.run_device(ctx, case)
    if gain:
        g = toc.run_gain(ctx, case)
        got.update({key: g[key] for key in ex.GAIN_OUT})
        got["gain_status"], got["keep"] = g["status"], g["keep"]
    return got


def run_nform(ctx, case, gamma=None, sa_inv=None):
    """prepare + solve (+ cost) through nform_device.Dev; ``sa_inv`` replaces the inverse Dev takes of case["sa"]."""
    d = nfd.Dev(case)
    if sa_inv is not None:
        d.sa_inv = nfd._dev(sa_inv)
    return d.run(ctx, gamma=None if gamma is None else np.full(d.nprof, gamma))


def run_whiten(ctx, case):
    """mwrt_obs_whiten_device, then mwrt_obs_whiten_apply_device (mode 0) with the factor it stored on the same y, F and K
    -> (outputs of the first, the same keys from the second)."""
    got = twh.whiten(ctx, case["k"], case["se_p"], case["y"], case["fx"], nlev=case["k"][0].shape[2] if case["k"] else 1)
    vecs, blocks = twh.apply(ctx, got["l"], got["keep"], 0, vecs=(case["y"], case["fx"]), blocks=case["k"])
    return got, dict(l=got["l"], y_out=vecs[0], fx_out=vecs[1], k_out=blocks)


def finite_and_ok(got, keys, status_keys=("status",)):
    return all((got[s] == 1).all() for s in status_keys) and all(np.isfinite(np.asarray(got[k])).all() for k in keys)


def mform_device_errors(ctx, key):
    """-> (per-profile error dicts, got) of one case of ex.mform_cases()."""
    shape, se_full, k, gamma = key
    e = ex.mform_entry(key)
    with_gain = gamma is None and shape == ex.MFORM_GAIN_SHAPE
    got = run_mform(ctx, e["case"], gamma=gamma, gain=with_gain)
    err = ex.mform_errors(got, e["exact"], e["case"], keys=ex.MFORM_OUT if gamma is None else ("x_new",))
    if with_gain:
        for a, b in zip(err, ex.gain_errors(got, e["exact"], e["case"])):
            a.update(b)
    return err, got


def nform_device_errors(ctx, key):
    shape, k, gamma = key
    e = ex.nform_entry(key)
    got = run_nform(ctx, e["case"], gamma=gamma, sa_inv=e["case"]["sa_inv"])
    return ex.nform_errors(got, e["exact"], e["case"], keys=ex.NFORM_OUT if gamma is None else ("x_new",)), got


def whiten_device_errors(ctx, key):
    """The larger of the combined entry's error and the apply entry's, per profile and output."""
    e = ex.whiten_entry(key)
    got, applied = run_whiten(ctx, e["case"])
    err = ex.whiten_errors(got, e["exact"])
    for a, b in zip(err, ex.whiten_errors(applied, e["exact"])):
        for out in a:
            a[out] = max(a[out], b[out])
    return err, got


DEVICE_ERRORS = {"mform": mform_device_errors, "nform": nform_device_errors, "whiten": whiten_device_errors}
