"""TEST INFRASTRUCTURE ONLY -- the exact derivative reference of ``oracle/tl_oracle.py`` extended to cloud liquid and ice.

``oracle.tl_oracle`` restates the clear-sky plane-parallel path of ``oracle/lbl_oracle.py`` in torch float64 on the CPU so
that autograd yields exact derivatives.  This module composes its functions (``clearsky_absorption``, ``_LogMean``,
``exponential_integration``, ``planck_down``, ``bright``, ``_rows``, ``absorption_tl``) and adds what
``lbl_oracle.tb_cloud_rte(..., denliq, denice)`` adds: ``liquid_water_absorption`` (both ``liq_mode``s, complex128), the
ice term and the ``zeroflg = False`` layer rule.  ``tests/test_cloudy_tl_reference.py`` pins it to ``lbl_oracle``;
``tests/test_jacobian_cloudy.py`` checks ``mwrt_tb_jacobian_batch_opt_device`` against it entry by entry.

Derivative conventions (include/mwrt.h) -- the derivative of the branch the oracle takes:

* a density <= 0 is "no cloud": the absorption is 0 and so is its derivative;
* the ``zeroflg = False`` layer rule: a layer with a zero end value has the value 0 and the partials (0, 0) (the
  log-mean's own one-sided slope there is infinite); ``|x1 - x0| < 1e-9``: value x1, partials (1, 0); otherwise the
  log-mean with ``tl._LogMean``'s partials.

Neither a conftest nor a test file; nothing here touches the native library or a GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import tl_oracle as tl

F64 = tl.F64
_t = tl._t
#: RTEquation.cloudy_absorption's ice term per GHz and g m-3: (8.18645 / wavelength[cm]) * 0.000959553 dB/km -> Np/km
KICE = 8.18645 * 0.000959553 * (math.log(10.0) * 0.1) * 1e9 / (299792458.0 * 100.0)


def liquid_water_absorption(m, water, freq, temp):
    """lbl_oracle.liquid_water_absorption for every frequency and level at once: water [g m-3], temp [K]: [nlev];
    freq [GHz]: [nf] -> [nf][nlev] Np/km.  water <= 0: 0, with zero gradient (double where: the untaken branch sees 1)."""
    water, temp = _t(water), _t(temp)
    freq = _t(freq).reshape(-1, 1)
    pos = water > 0
    w = torch.where(pos, water, torch.ones_like(water))
    one = torch.ones(freq.shape[0], temp.shape[0], dtype=F64)
    if m.liq_mode == 0:
        theta1 = 1.0 - 300.0 / temp
        eps0 = 77.66 - 103.3 * theta1
        eps1 = 0.0671 * eps0
        eps2 = 3.52
        fp = (316.0 * theta1 + 146.4) * theta1 + 20.2
        fs = 39.8 * fp
        eps = (eps0 - eps1) / torch.complex(one, freq / fp) + (eps1 - eps2) / torch.complex(one, freq / fs) + eps2
    else:
        tc = temp - 273.15
        z = torch.complex(torch.zeros_like(freq), freq)
        theta = 300.0 / temp
        eps0 = -43.7527 * theta ** 0.05 + 299.504 * theta ** 1.47 - 399.364 * theta ** 2.11 + 221.327 * theta ** 2.31
        delta = 80.69715 * torch.exp(-tc / 226.45)
        sd = 1164.023 * torch.exp(-651.4728 / (tc + 133.07))
        kappa = -delta * z / (sd + z)
        delta = 4.008724 * torch.exp(-tc / 103.05)
        hdelta = delta / 2.0
        f1 = 10.46012 + 0.1454962 * tc + 0.063267156 * tc ** 2 + 0.00093786645 * tc ** 3
        z1 = complex(-0.75, 1.0) * f1
        z2 = complex(-4500.0, 2000.0)
        cnorm = torch.log(z2 / z1)
        chip = (hdelta * torch.log((z - z2) / (z - z1))) / cnorm
        chij = (hdelta * torch.log((z - z2.conjugate()) / (z - torch.conj(z1)))) / torch.conj(cnorm)
        dchi = chip + chij - delta
        kappa = kappa + dchi
        eps = eps0 + kappa
    re = (eps - 1.0) / (eps + 2.0)
    out = -0.06286 * re.imag * freq * w
    return torch.where(pos, out, torch.zeros_like(out))


def ice_absorption(deni, freq):
    """lbl_oracle.cloudy_absorption's ice term: deni [nlev], freq [nf] -> [nf][nlev] Np/km; deni <= 0: 0, zero gradient."""
    deni = _t(deni)
    freq = _t(freq).reshape(-1, 1)
    out = (KICE * freq) * deni
    return torch.where(deni > 0, out, torch.zeros_like(out))


def exponential_integration_noz(x, ds):
    """lbl_oracle.exponential_integration(zeroflg = False) for every row at once, in the oracle's branch order:
    |x1 - x0| < 1e-9 -> x1, partials (1, 0); a zero end -> the constant 0, partials (0, 0); else the log-mean."""
    if bool((x < 0.0).any()):
        raise ValueError("Error encountered in exponential_integration")
    x1, x0 = x[..., 1:], x[..., :-1]
    small = torch.abs(x1 - x0) < 1e-09
    zero = (x0 == 0.0) | (x1 == 0.0)
    general = ~small & ~zero
    g1 = torch.where(general, x1, torch.full_like(x1, 2.0))      # double where, as tl.exponential_integration
    g0 = torch.where(general, x0, torch.ones_like(x0))
    xlayer = torch.where(small, x1, torch.where(zero, torch.zeros_like(x1), tl._LogMean.apply(g1, g0)))
    xds = xlayer * ds[..., 1:]
    return torch.cat([torch.zeros_like(xds[..., :1]), xds], dim=-1)


def tb_from_absorption(m, awet, adry, aliq, aice, dsz, tk, frq, angles):
    """The RTE half of tb_cloud_rte under cloud: absorption rows [nf][nlev] -> TBs [nang][nf]; the layer optical depth
    is summed in the oracle's order, pw + pd + pi + pl."""
    ds = dsz.reshape(1, -1) * tl._amass(angles).reshape(-1, 1)
    pw = tl.exponential_integration(awet[:, None, :], ds)
    pd = tl.exponential_integration(adry[:, None, :], ds)
    pl = exponential_integration_noz(aliq[:, None, :], ds)
    pi = exponential_integration_noz(aice[:, None, :], ds)
    taulay = pw + pd + pi + pl
    boftotl, hvk, _ = tl.planck_down(m, _t(frq).reshape(-1, 1, 1), tk, taulay)
    return tl.bright(hvk, boftotl).T


def _dsz(z):
    zz = z - z[0]
    return torch.cat([torch.zeros_like(zz[:1]), zz[1:] - zz[:-1]])


def _cloud(x, like):
    return torch.zeros_like(like) if x is None else _t(x)


def tb_rh(m, z, p, t, rh, denliq, denice, frq, angles):
    """tb_cloud_rte(..., denliq, denice)'s tbtotal [nang][nf] from the (z, p, t, rh) inputs; a cloud array may be None."""
    z, p, t, rh = (_t(x) for x in (z, p, t, rh))
    e, _ = tl.vapor(t, rh)
    awet, adry = tl.clearsky_absorption(m, p, t, e, frq)
    aliq = liquid_water_absorption(m, _cloud(denliq, t), frq, t)
    aice = ice_absorption(_cloud(denice, t), frq)
    return tb_from_absorption(m, awet, adry, aliq, aice, _dsz(z), t, frq, angles)


def k_matrix_cloudy(m, z, p, tk, e, denliq, denice, frq, angles):
    """The device K-matrix of one cloudy profile in the ABI's layout: tb [nang][nf] and dtb_dt (fixed e), dtb_de (fixed T),
    dtb_ddz, dtb_dliq, dtb_dice [nang][nf][nlev].  Two autograd stages joined by the chain rule, as tl.k_matrix: the exact
    clear-sky absorption partials (local per level), then each TB's gradients with respect to the absorption rows, T
    (the Planck terms and the liquid absorption), the layer thicknesses and the two cloud columns."""
    with torch.enable_grad():
        z, p, tk, e = (_t(x) for x in (z, p, tk, e))
        ab = tl.absorption_tl(m, p, tk, e, frq)
        aw = ab["awet"].clone().requires_grad_(True)
        ad = ab["adry"].clone().requires_grad_(True)
        tq = tk.clone().requires_grad_(True)
        dl = _cloud(denliq, tk).clone().requires_grad_(True)
        di = _cloud(denice, tk).clone().requires_grad_(True)
        dsz = _dsz(z).detach().requires_grad_(True)
        aliq = liquid_water_absorption(m, dl, frq, tq)
        aice = ice_absorption(di, frq)
        tb = tb_from_absorption(m, aw, ad, aliq, aice, dsz, tq, frq, angles)
        nang, nf = tb.shape
        nlev = z.shape[0]
        jf = torch.arange(nf)
        g_aw, g_ad, g_t, g_dz, g_dl, g_di = tl._rows(tb, (aw, ad, tq, dsz, dl, di))
        g_aw = g_aw.reshape(nang, nf, nf, nlev)[:, jf, jf, :]
        g_ad = g_ad.reshape(nang, nf, nf, nlev)[:, jf, jf, :]
        dt = g_aw * ab["dawet_dt"] + g_ad * ab["dadry_dt"] + g_t
        de = g_aw * ab["dawet_de"] + g_ad * ab["dadry_de"]
        return {"tb": tb.detach(), "dtb_dt": dt, "dtb_de": de, "dtb_ddz": g_dz, "dtb_dliq": g_dl, "dtb_dice": g_di}


def k_matrix_cloudy_rh(m, z, p, t, rh, denliq, denice, frq, angles):
    """k_matrix_cloudy from the (z, p, t, rh) inputs the device entry takes."""
    e, _ = tl.vapor(_t(t), _t(rh))
    return k_matrix_cloudy(m, z, p, t, e.detach(), denliq, denice, frq, angles)


def direct_gradients(m, z, p, t, rh, denliq, denice, frq, angles, weights=None):
    """Autograd of sum(weights * TB) with respect to z, t, rh, denliq and denice (one backward through the whole graph).
    -> {"z", "t", "rh", "denliq", "denice"} [nlev] each."""
    tt = _t(t)
    xs = [x.clone().requires_grad_(True) for x in (_t(z), tt, _t(rh), _cloud(denliq, tt), _cloud(denice, tt))]
    tb = tb_rh(m, xs[0], _t(p), xs[1], xs[2], xs[3], xs[4], frq, angles)
    w = torch.ones_like(tb) if weights is None else _t(weights)
    g = torch.autograd.grad((w * tb).sum(), xs)
    return dict(zip(("z", "t", "rh", "denliq", "denice"), g))


def cloud_profile(nlev, seed=0, t0=288.0):
    """A plain moist profile for the cloud tests: z [km], p [hPa], t [K], rh, each [nlev] numpy."""
    rng = np.random.default_rng(seed)
    dz = rng.uniform(0.5, 1.5, nlev) * (12.0 / nlev)              # ~12 km whatever the number of levels
    dz[0] = 0.0
    h = np.cumsum(dz)
    z = h + 0.3
    p = 1010.0 * np.exp(-h / 7.7)
    t = t0 - 6.2 * np.minimum(h, 11.0) + rng.normal(0.0, 0.3, nlev)
    rh = np.clip(0.85 * np.exp(-h / 3.5) + rng.uniform(-0.04, 0.04, nlev), 0.01, 1.0)
    return z, p, t, rh
