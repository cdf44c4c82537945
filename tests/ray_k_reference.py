"""TEST INFRASTRUCTURE ONLY -- the exact derivative reference of the K-matrix along refracted spherical ray paths
(include/mwrt.h mwrt_tb_jacobian_batch_ray_device).

``oracle/lbl_oracle.py`` traces its rays in a scalar NumPy loop (``refractivity``, ``ray_tracing``).  This module restates
the two in torch float64, vectorised over the levels and in the oracle's branch order, so that autograd yields the exact
response of every layer's slant path to the state; the absorption, the layer rule, the Planck recursion and ``bright`` are
``oracle.tl_oracle``'s and ``cloudy_tl_reference``'s own functions (imported, not copied).  The rows come out in the ABI's
layout: T at fixed e, e at fixed T, thickness of the layer below each level with z_0 and every other thickness held, and
the two cloud columns; ``kmatrix_variables_reference.chain`` turns them into retrieval variables.

Conventions -- the derivative of the branch the operator takes:

* ``order="oracle"`` forms a layer's angles as the oracle does, from the running sums phi and tau of the levels below;
  ``order="direct"`` forms the differences directly, as the device's path kernel does (they agree to rounding; the test
  of the conditioning floor measures by how much);
* the operator is the device's: a zero-thickness layer outside the zenith branch has the slant path 0 (k_ray_paths writes
  the path factor 0 there; the oracle's own formula gives the horizontal chord), with no tangent;
* within 1 degree of zenith ds = dz exactly, for every layer;
* a trapped ray (``argth <= 0`` at any level) gives NaN for its whole elevation, as the oracle raises for it.

Neither a conftest nor a test file; nothing here touches the native library or a GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import cloudy_tl_reference as cr
from oracle import tl_oracle as tl

F64 = tl.F64
_t = tl._t
EARTH_RADIUS_KM = 6370.949


def refractivity(p, tk, e):
    """lbl_oracle.refractivity's refractive index per level (Thayer 1974), torch."""
    pa = p - e
    tc = tk - 273.16
    tk2 = tk * tk
    tc2 = tc * tc
    rza = 1.0 + pa * (5.79e-07 * (1.0 + 0.52 / tk) - (0.00094611 * tc) / tk2)
    rzw = 1.0 + 1650.0 * (e / (tk * tk2)) * (1.0 - 0.01317 * tc + 0.000175 * tc2 + 1.44e-06 * (tc2 * tc))
    wetn = (64.79 * (e / tk) + 377600.0 * (e / tk2)) * rzw
    dryn = 77.6036 * (pa / tk) * rza
    return 1.0 + (dryn + wetn) * 1e-06


def is_zenith(angle):
    return (89 <= angle <= 91) or (-91 <= angle <= -89)


def ray_path(zr, refindx, angle, z0, order="oracle"):
    """lbl_oracle.ray_tracing(z, refindx, angle, z0) for one elevation, every level at once: zr [nlev] heights above the
    ground level (zr[0] = 0), refindx [nlev], z0 the ground level's height (a constant: never differentiated) ->
    (ds [nlev] with ds[0] = 0, trapped).  A trapped ray returns NaN above the ground."""
    nl = zr.shape[0]
    dz = zr[1:] - zr[:-1]
    zero = torch.zeros(1, dtype=F64)
    if is_zenith(angle):
        return torch.cat([zero, dz]), False
    theta0 = angle * (math.pi / 180)
    re = EARTH_RADIUS_KM
    rs = re + 0.0 + z0
    costh0 = math.cos(theta0)
    sina = math.sin(theta0 * 0.5)
    a0 = 2.0 * (sina ** 2)
    n, nprev, n0 = refindx[1:], refindx[:-1], refindx[0]
    r = re + zr + z0                                         # [nlev]
    unit = (n == nprev) | (n == 1.0) | (nprev == 1.0)
    gn = torch.where(unit, torch.full_like(n, 1.0002), n)    # double where: the log form sees harmless stand-ins
    gp = torch.where(unit, torch.full_like(n, 1.0003), nprev)
    refbar = torch.where(unit, (n + nprev) * 0.5, 1.0 + (gp - gn) / torch.log((gp - 1.0) / (gn - 1.0)))
    z1 = zr[1:]
    argdth = z1 / rs - ((n0 - n) * costh0 / n)
    argth = 0.5 * (a0 + argdth) / r[1:]
    if bool((argth <= 0).any()):
        return torch.cat([zero, torch.full((nl - 1,), math.nan, dtype=F64)]), True
    sint = torch.sqrt(r[1:] * argth)
    theta_b = 2.0 * torch.asin(sint)
    near = (theta_b - 2.0 * theta0) <= 0.0
    dendth = 2.0 * (sint + sina) * torch.cos((theta_b + theta0) * 0.25)
    sind4 = (0.5 * argdth - z1 * argth) / dendth
    sind4 = torch.where(near, sind4, torch.zeros_like(sind4))           # (the branch not taken must stay finite)
    dtheta = torch.where(near, 4.0 * torch.asin(sind4), theta_b - theta0)
    theta = torch.where(near, theta0 + dtheta, theta_b)
    tanth = torch.tan(theta)
    tanthl = torch.cat([torch.full((1,), math.tan(theta0), dtype=F64), tanth[:-1]])
    cthbar = ((1.0 / tanth) + (1.0 / tanthl)) * 0.5
    dtau = cthbar * (nprev - n) / refbar
    if order == "oracle":
        tau = torch.cumsum(dtau, dim=0)
        phi = dtheta + tau
        phil = torch.cat([zero, phi[:-1]])
        taul = torch.cat([zero, tau[:-1]])
        dphi = phi - phil
        dtaua = torch.abs(tau - taul)
    else:
        dthl = torch.cat([zero, dtheta[:-1]])
        dphi = (dtheta - dthl) + dtau
        dtaua = torch.abs(dtau)
    thick = dz != 0.0
    dzs = torch.where(thick, dz, torch.ones_like(dz))
    ds = torch.sqrt(dzs ** 2 + 4.0 * r[1:] * r[:-1] * ((torch.sin(dphi * 0.5)) ** 2))
    bent = dtau != 0.0
    da = torch.where(bent, dtaua, torch.ones_like(dtaua))
    ds = torch.where(bent, ds * (da / (2.0 * torch.sin(da * 0.5))), ds)
    ds = torch.where(thick, ds, torch.zeros_like(ds))
    return torch.cat([zero, ds]), False


def ray_paths(z, refindx, angles, order="oracle"):
    """ds [nang][nlev] and trapped [nang] for absolute heights z [nlev] (z[0] enters as the constant z0)."""
    z0 = float(z[0].detach())
    zr = z - z[0]
    out = [ray_path(zr, refindx, float(a), z0, order) for a in np.asarray(angles, dtype=np.float64)]
    return torch.stack([o[0] for o in out]), np.array([o[1] for o in out])


def tb_from_paths(m, awet, adry, aliq, aice, ds, tk, frq):
    """The RTE half of tb_cloud_rte for slant paths ds [nang][nlev]: absorption rows [nf][nlev] -> TBs [nang][nf]; the
    layer optical depth is summed in the oracle's order, pw + pd + pi + pl.  aliq / aice None: clear sky."""
    pw = tl.exponential_integration(awet[:, None, :], ds)
    pd = tl.exponential_integration(adry[:, None, :], ds)
    taulay = pw + pd
    if aliq is not None:
        pl = cr.exponential_integration_noz(aliq[:, None, :], ds)
        pi = cr.exponential_integration_noz(aice[:, None, :], ds)
        taulay = pw + pd + pi + pl
    boftotl, hvk, _ = tl.planck_down(m, _t(frq).reshape(-1, 1, 1), tk, taulay)
    return tl.bright(hvk, boftotl).T


def tb_rh(m, z, p, t, rh, frq, angles, denliq=None, denice=None, order="oracle"):
    """tb_cloud_rte(..., ray_tracing_on=True)'s tbtotal [nang][nf] from the (z, p, t, rh) inputs; NaN where trapped."""
    z, p, t, rh = (_t(x) for x in (z, p, t, rh))
    e, _ = tl.vapor(t, rh)
    ds, trapped = ray_paths(z, refractivity(p, t, e), angles, order)
    awet, adry = tl.clearsky_absorption(m, p, t, e, frq)
    cloudy = denliq is not None or denice is not None
    aliq = cr.liquid_water_absorption(m, cr._cloud(denliq, t), frq, t) if cloudy else None
    aice = cr.ice_absorption(cr._cloud(denice, t), frq) if cloudy else None
    ok = np.flatnonzero(~trapped)
    tb = torch.full((len(trapped), len(np.atleast_1d(frq))), math.nan, dtype=F64)
    if ok.size:
        tb[ok] = tb_from_paths(m, awet, adry, aliq, aice, ds[ok], t, frq)
    return tb


def k_matrix_ray(m, z, p, tk, e, frq, angles, denliq=None, denice=None, frozen=False, order="oracle"):
    """The ray-traced K-matrix of one profile in the ABI's layout: tb [nang][nf] and dtb_dt (fixed e), dtb_de (fixed T),
    dtb_ddz and, with a cloud array, dtb_dliq / dtb_dice [nang][nf][nlev]; a trapped elevation is NaN throughout.  Also
    "path_dt" / "path_de": the part of the two rows that reaches the TB through the refractive index alone.

    Autograd in two stages joined by the chain rule, as tl.k_matrix: the exact absorption partials (local per level), then
    each TB's gradients with respect to the absorption rows, T (Planck terms, liquid absorption), T and e as the refractive
    index sees them, the layer thicknesses (heights rebuilt from them above the fixed z_0) and the cloud columns.
    ``frozen=True`` holds every path factor ds/dz fixed: the plane-parallel rule with a factor per layer."""
    with torch.enable_grad():
        z, p, tk, e = (_t(x) for x in (z, p, tk, e))
        cloudy = denliq is not None or denice is not None
        ab = tl.absorption_tl(m, p, tk, e, frq)
        aw = ab["awet"].clone().requires_grad_(True)
        ad = ab["adry"].clone().requires_grad_(True)
        tq = tk.clone().requires_grad_(True)
        tn = tk.clone().requires_grad_(True)
        en = e.clone().requires_grad_(True)
        dsz = cr._dsz(z).detach().requires_grad_(True)
        zabs = z[0].detach() + torch.cumsum(torch.cat([torch.zeros(1, dtype=F64), dsz[1:]]), dim=0)     # (entry 0: no layer)
        ds, trapped = ray_paths(zabs, refractivity(p, tn, en), angles, order)
        if frozen:
            thick = dsz != 0.0
            f = torch.where(thick, ds / torch.where(thick, dsz, torch.ones_like(dsz)), torch.zeros_like(ds)).detach()
            zen = torch.tensor([is_zenith(float(a)) for a in np.asarray(angles, dtype=np.float64)])
            ds = torch.where(zen[:, None], dsz.expand_as(ds), f * dsz)
        leaves = [aw, ad, tq, tn, en, dsz]
        aliq = aice = None
        if cloudy:
            dl = cr._cloud(denliq, tk).clone().requires_grad_(True)
            di = cr._cloud(denice, tk).clone().requires_grad_(True)
            aliq = cr.liquid_water_absorption(m, dl, frq, tq)
            aice = cr.ice_absorption(di, frq)
            leaves += [dl, di]
        nang, nf, nlev = len(trapped), len(np.atleast_1d(frq)), z.shape[0]
        ok = np.flatnonzero(~trapped)
        out = {"tb": torch.full((nang, nf), math.nan, dtype=F64)}
        keys = ["dtb_dt", "dtb_de", "dtb_ddz", "path_dt", "path_de"] + (["dtb_dliq", "dtb_dice"] if cloudy else [])
        for k in keys:
            out[k] = torch.full((nang, nf, nlev), math.nan, dtype=F64)
        if ok.size:
            tb = tb_from_paths(m, aw, ad, aliq, aice, ds[ok], tq, frq)
            g = tl._rows(tb, leaves)
            jf = torch.arange(nf)
            g_aw = g[0].reshape(len(ok), nf, nf, nlev)[:, jf, jf, :]
            g_ad = g[1].reshape(len(ok), nf, nf, nlev)[:, jf, jf, :]
            out["tb"][ok] = tb.detach()
            out["dtb_dt"][ok] = g_aw * ab["dawet_dt"] + g_ad * ab["dadry_dt"] + g[2] + g[3]
            out["dtb_de"][ok] = g_aw * ab["dawet_de"] + g_ad * ab["dadry_de"] + g[4]
            out["dtb_ddz"][ok] = g[5]
            out["path_dt"][ok], out["path_de"][ok] = g[3], g[4]
            if cloudy:
                out["dtb_dliq"][ok], out["dtb_dice"][ok] = g[6], g[7]
        return out


def k_matrix_ray_rh(m, z, p, t, rh, frq, angles, denliq=None, denice=None, frozen=False, order="oracle"):
    """k_matrix_ray from the (z, p, t, rh) inputs the device entry takes."""
    e, _ = tl.vapor(_t(t), _t(rh))
    return k_matrix_ray(m, z, p, t, e.detach(), frq, angles, denliq, denice, frozen, order)
