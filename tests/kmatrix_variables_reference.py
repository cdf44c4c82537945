"""TEST INFRASTRUCTURE ONLY -- the device K-matrix in retrieval variables (include/mwrt.h mwrt_jac_variables, DESIGN.md
4.5.3), twice over on the CPU:

* ``chain``: the header's chain-rule formulas in NumPy, applied to a raw K-matrix (the rows of
  ``cloudy_tl_reference.k_matrix_cloudy``), with the sum of the absolute terms of every entry -- the scale the GPU tests'
  tolerance is taken from;
* ``end_to_end``: torch autograd of the TBs as a function of (T, h, q_liq, q_ice) with the variable definitions written
  out -- e from h, density from mixing ratio, heights from the hydrostatic rule -- and nothing of the chain rule.

``tests/test_kmatrix_variables_cpu.py`` holds the two against each other for every mode combination, which is what
licenses ``chain`` as the reference at sizes where one backward pass per TB would be slow.

``variables`` is ``(humidity, cloud, heights)``, the integers of ``mwrt_jac_variables``.  Neither a conftest nor a test
file; nothing here touches the native library or a GPU.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

import cloudy_tl_reference as cr
from oracle import tl_oracle as tl

_t = tl._t
RD_HYDRO, G0 = 287.04, 9.80665          # rttov_gb_wrapper.to_lbl_inputs
R_DRY_AIR = 287.06                      # pyrtlib_processing.R_DRY_AIR
#: every (humidity, cloud, heights)
ALL_VARIABLES = list(itertools.product((0, 1, 2), (0, 1), (0, 1)))
KEYS = ("dtb_dt", "dtb_dh", "dtb_ddz", "dtb_dliq", "dtb_dice")


def es_and_slope(tk):
    """Goff-Gratch es(T) [hPa] over water and d es / dT, NumPy: es = 10^g(y), y = 373.16 / T."""
    tk = np.asarray(tk, dtype=np.float64)
    ln10 = math.log(10.0)
    y = 373.16 / tk
    a, b = 10.0 ** (11.344 * (1.0 - 1.0 / y)), 10.0 ** (-3.49149 * (y - 1.0))
    g = -7.90298 * (y - 1.0) + 5.02808 * np.log10(y) - 1.3816e-07 * (a - 1.0) + 0.0081328 * (b - 1.0) + math.log10(1013.246)
    gy = -7.90298 + 5.02808 / (ln10 * y) - 1.3816e-07 * a * ln10 * 11.344 / y ** 2 - 0.0081328 * b * ln10 * 3.49149
    es = 10.0 ** g
    return es, es * ln10 * gy * (-y / tk)


def hydrostatic_z(z0, p, t, rh):
    """Heights [km] that obey the hydrostatic rule above z0 (NumPy, levels ground -> top)."""
    es, _ = es_and_slope(t)
    e = rh * es
    tv = t * (1.0 + 0.608 * (0.622 * e / (p - 0.378 * e)))
    dz = RD_HYDRO / G0 * 0.5 * (tv[1:] + tv[:-1]) * np.log(p[:-1] / p[1:]) / 1000.0
    return z0 + np.concatenate([[0.0], np.cumsum(dz)])


def chain(K, p, t, rh, denliq, denice, variables):
    """Raw rows K = {"dtb_dt", "dtb_de", "dtb_ddz"[, "dtb_dliq", "dtb_dice"]} [..., nlev] (NumPy or torch) and the level
    arrays [nlev] -> (rows, scale): rows = {"dtb_dt", "dtb_dh", "dtb_ddz", and the cloud rows K holds} in the variables
    asked for; scale = the sum of the absolute values of the terms each entry is the sum of, the same keys."""
    hum, cloud, heights = variables
    R = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in K.items()
         if k.startswith("dtb_") and v is not None}
    p, t, rh = (np.asarray(x, dtype=np.float64) for x in (p, t, rh))
    es, des = es_and_slope(t)
    e = rh * es
    a_t, a_e, zr = R["dtb_dt"].copy(), R["dtb_de"].copy(), R["dtb_ddz"]
    s_t, s_e = np.abs(a_t), np.abs(a_e)
    if heights:
        c = np.zeros_like(p)
        c[1:] = RD_HYDRO / (2.0 * G0) * np.log(p[:-1] / p[1:]) / 1000.0
        lo = zr * c                                           # Z_i c_i
        up = np.zeros_like(lo)
        up[..., :-1] = lo[..., 1:]                            # Z_{i+1} c_{i+1}
        q = 0.622 * e / (p - 0.378 * e)
        k_t, k_e = 1.0 + 0.608 * q, 0.608 * t * 0.622 * p / (p - 0.378 * e) ** 2
        a_t += (lo + up) * k_t
        a_e += (lo + up) * k_e
        s_t += (np.abs(lo) + np.abs(up)) * k_t
        s_e += (np.abs(lo) + np.abs(up)) * k_e
    de_dh = {0: np.ones_like(p), 1: es, 2: p / 1e6}[hum]
    de_dt = rh * des if hum == 1 else np.zeros_like(p)
    out = {"dtb_dt": a_t + a_e * de_dt, "dtb_dh": a_e * de_dh, "dtb_ddz": zr}
    scale = {"dtb_dt": s_t + s_e * np.abs(de_dt), "dtb_dh": s_e * de_dh, "dtb_ddz": np.abs(zr)}
    rho1000 = 1000.0 * 100.0 * p / (R_DRY_AIR * t)
    for key, den in (("dtb_dliq", denliq), ("dtb_dice", denice)):
        if key not in R:
            continue
        r = R[key]
        if cloud:
            den = np.zeros_like(p) if den is None else np.asarray(den, dtype=np.float64)
            out["dtb_dt"] = out["dtb_dt"] - r * den / t
            scale["dtb_dt"] = scale["dtb_dt"] + np.abs(r * den) / t
            r = r * rho1000
        out[key], scale[key] = r, np.abs(r)
    return out, scale


def end_to_end(m, z, p, t, rh, denliq, denice, frq, angles, variables):
    """tb [nang][nf] and the rows d tb / d (T, h, q_liq, q_ice) [nang][nf][nlev] by autograd through the variable
    definitions: "dtb_dt", "dtb_dh", "dtb_dliq", "dtb_dice", and with fixed heights "dtb_ddz".  With hydrostatic heights
    the layer thicknesses are BUILT by the rule from (p, T, e), so z must obey it for the TBs to be those of z."""
    hum, cloud, heights = variables
    with torch.enable_grad():
        p, t0, rh0 = _t(p), _t(t), _t(rh)
        tq = t0.clone().requires_grad_(True)
        es0, _ = tl.vapor(t0, torch.ones_like(t0))
        h = {0: rh0 * es0, 1: rh0, 2: rh0 * es0 * 1e6 / p}[hum].clone().requires_grad_(True)
        es, _ = tl.vapor(tq, torch.ones_like(tq))
        e = {0: h, 1: h * es, 2: h * p / 1e6}[hum]
        rho1000 = 1000.0 * 100.0 * p / (R_DRY_AIR * tq)
        cl = []
        for den in (denliq, denice):
            den = cr._cloud(den, t0)
            x = (den / (1000.0 * 100.0 * p / (R_DRY_AIR * t0)) if cloud else den).clone().requires_grad_(True)
            cl.append(x)
        dl, di = (x * rho1000 if cloud else x for x in cl)
        if heights:
            tv = tq * (1.0 + 0.608 * (0.622 * e / (p - 0.378 * e)))
            dz = RD_HYDRO / G0 * 0.5 * (tv[1:] + tv[:-1]) * torch.log(p[:-1] / p[1:]) / 1000.0
            dsz = torch.cat([torch.zeros_like(dz[:1]), dz])
        else:
            dsz = cr._dsz(_t(z)).detach().requires_grad_(True)
        awet, adry = tl.clearsky_absorption(m, p, tq, e, frq)
        aliq = cr.liquid_water_absorption(m, dl, frq, tq)
        aice = cr.ice_absorption(di, frq)
        tb = cr.tb_from_absorption(m, awet, adry, aliq, aice, dsz, tq, frq, angles)
        xs = [tq, h, cl[0], cl[1]] + ([] if heights else [dsz])
        g = tl._rows(tb, xs)
        out = {"tb": tb.detach(), "dtb_dt": g[0].numpy(), "dtb_dh": g[1].numpy(), "dtb_dliq": g[2].numpy(),
               "dtb_dice": g[3].numpy()}
        if not heights:
            out["dtb_ddz"] = g[4].numpy()
        return out


def scaled_row_errors(got, want, scale):
    """|got - want| / (the row's largest scale), rows over the last axis; a row whose scale is all zero must be exactly
    zero (inf otherwise)."""
    s = np.abs(scale).max(axis=-1, keepdims=True)
    err = np.abs(got - want)
    return np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where(err > 0, np.inf, 0.0))
