"""Differentiable brightness temperatures for PyTorch: ``brightness_temperature`` takes part in a loss and
``.backward()`` runs through the device K-matrix (include/mwrt.h ``mwrt_tb_jacobian_batch_device``).

    tb, valid = brightness_temperature("R24", z, p, t, rh, frq, elev)      # z, p, t, rh: float64 [nprof][nlev] CUDA
    loss = ((tb - tb_obs) ** 2).sum(); loss.backward()                      # t.grad, rh.grad, z.grad

Without grad the forward is one ``mwrt_tb_batch_device`` call.  When z, t or rh requires grad the forward is ONE
``mwrt_tb_jacobian_batch_device`` call, which also yields the TBs, and the op saves the three Jacobians
(dTB/dT at fixed e, dTB/de, dTB/d layer thickness, each [nprof][nang][nf][nlev] float64): 3 x 8 B x nprof x nang x nf x
nlev, i.e. 3 x 141 MB at 1000 profiles x 7 elevations x 14 channels x 180 levels.  The backward contracts them with
the incoming gradient on the device and applies the chain rule to the op's own variables:

    dTB/dt|rh = dtb_dt + dtb_de * rh * des/dT,   dTB/drh = dtb_de * es(T),   dTB/dz_i = dtb_ddz_i - dtb_ddz_{i+1}

(es: Goff-Gratch over water, as RTEquation.vapor; level i is the top of one layer and the bottom of the next).
With ``denliq`` / ``denice`` (cloud liquid / ice, g m-3) the same holds through ``mwrt_tb_batch_opt_device`` and
``mwrt_tb_jacobian_batch_opt_device``; two more saved Jacobians give ``grad_denliq = sum_{ang, f} g * dtb_dliq`` (ice alike).
No pressure derivative is computed: ``p.requires_grad`` raises NotImplementedError.  A profile flagged invalid
(valid 0: NaN input, 2: negative absorption) gets NaN gradients -- NaN in, NaN out.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native

LN10 = math.log(10.0)


def _native_tb(model, z, p, t, rh, frq, elev, stream):
    """TBs only: one ``mwrt_tb_batch_device`` call.  Returns (tb [nprof][nang][nf], valid [nprof] uint8)."""
    nprof, nlev = _check_device(z, p, t, rh)
    tb = torch.empty((nprof, elev.size, frq.size), dtype=torch.float64, device=z.device)
    valid = torch.empty(nprof, dtype=torch.uint8, device=z.device)
    _native.default_context(z.device.index or 0).tb_batch_device(
        model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, elev, tb.data_ptr(),
        valid.data_ptr(), stream=_stream_of(z, stream))
    return tb, valid


def _native_jacobian(model, z, p, t, rh, frq, elev, stream):
    """The K-matrix: one ``mwrt_tb_jacobian_batch_device`` call.  Returns (tb, valid, dtb_dt, dtb_de, dtb_ddz).

    The single place the op reaches the native library: CPU tests substitute an oracle stand-in here."""
    nprof, nlev = _check_device(z, p, t, rh)
    opts = dict(dtype=torch.float64, device=z.device)
    tb = torch.empty((nprof, elev.size, frq.size), **opts)
    jac = [torch.empty((nprof, elev.size, frq.size, nlev), **opts) for _ in range(3)]
    valid = torch.empty(nprof, dtype=torch.uint8, device=z.device)
    _native.default_context(z.device.index or 0).tb_jacobian_batch_device(
        model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, elev, tb.data_ptr(),
        jac[0].data_ptr(), jac[1].data_ptr(), jac[2].data_ptr(), valid.data_ptr(), stream=_stream_of(z, stream))
    return (tb, valid, *jac)


def _native_tb_cloudy(model, z, p, t, rh, denliq, denice, frq, elev, stream):
    """TBs only under cloud: one ``mwrt_tb_batch_opt_device`` call.  Returns (tb, valid)."""
    nprof, nlev = _check_device(z, p, t, rh, denliq=denliq, denice=denice)
    tb = torch.empty((nprof, elev.size, frq.size), dtype=torch.float64, device=z.device)
    valid = torch.empty(nprof, dtype=torch.uint8, device=z.device)
    _native.default_context(z.device.index or 0).tb_batch_device(
        model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, elev, tb.data_ptr(),
        valid.data_ptr(), stream=_stream_of(z, stream),
        d_denliq=None if denliq is None else denliq.data_ptr(), d_denice=None if denice is None else denice.data_ptr())
    return tb, valid


def _native_jacobian_cloudy(model, z, p, t, rh, denliq, denice, frq, elev, stream):
    """The K-matrix under cloud: one ``mwrt_tb_jacobian_batch_opt_device`` call.  Returns (tb, valid, dtb_dt, dtb_de,
    dtb_ddz, dtb_dliq, dtb_dice); a cloud Jacobian is None where its input is.

    The single place the cloudy op reaches the native library: CPU tests substitute a reference stand-in here."""
    nprof, nlev = _check_device(z, p, t, rh, denliq=denliq, denice=denice)
    opts = dict(dtype=torch.float64, device=z.device)
    tb = torch.empty((nprof, elev.size, frq.size), **opts)
    jac = [torch.empty((nprof, elev.size, frq.size, nlev), **opts) for _ in range(3)]
    jl = None if denliq is None else torch.empty((nprof, elev.size, frq.size, nlev), **opts)
    ji = None if denice is None else torch.empty((nprof, elev.size, frq.size, nlev), **opts)
    valid = torch.empty(nprof, dtype=torch.uint8, device=z.device)
    _native.default_context(z.device.index or 0).tb_jacobian_batch_opt_device(
        model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, elev, tb.data_ptr(),
        jac[0].data_ptr(), jac[1].data_ptr(), jac[2].data_ptr(), valid.data_ptr(),
        d_denliq=None if denliq is None else denliq.data_ptr(), d_denice=None if denice is None else denice.data_ptr(),
        d_dtb_dliq=None if jl is None else jl.data_ptr(), d_dtb_dice=None if ji is None else ji.data_ptr(),
        stream=_stream_of(z, stream))
    return (tb, valid, *jac, jl, ji)


def _check_device(z, p, t, rh, **cloud):
    for name, x in (("z", z), ("p", p), ("t", t), ("rh", rh), *((k, v) for k, v in cloud.items() if v is not None)):
        if not x.is_cuda or x.dtype != torch.float64 or x.dim() != 2 or not x.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous float64 [nprof][nlev] CUDA tensor")
        if x.shape != z.shape or x.device != z.device:
            raise ValueError(f"{name}: shape / device differs from z")
    return z.shape


def _stream_of(x, stream):
    return torch.cuda.current_stream(x.device).cuda_stream if stream is None else stream


def goff_gratch_es(t):
    """Saturation vapour pressure over water [hPa] and its derivative d es / dT [hPa/K] (RTEquation.vapor [EXT])."""
    y = 373.16 / t
    e1 = 10.0 ** (11.344 * (1.0 - 1.0 / y))
    e2 = 10.0 ** (-3.49149 * (y - 1.0))
    lg = (-7.90298 * (y - 1.0) + 5.02808 * torch.log10(y) - 1.3816e-07 * (e1 - 1.0) + 0.0081328 * (e2 - 1.0)
          + math.log10(1013.246))
    es = 10.0 ** lg
    dlg_dy = (-7.90298 + 5.02808 / (y * LN10) - 1.3816e-07 * e1 * LN10 * 11.344 / (y * y)
              + 0.0081328 * e2 * LN10 * (-3.49149))
    des_dt = es * LN10 * dlg_dy * (-373.16 / (t * t))
    return es, des_dt


class _BrightnessTemperature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, t, rh, p, model, frq, elev, stream):
        tb, valid, dtb_dt, dtb_de, dtb_ddz = _native_jacobian(model, z, p, t, rh, frq, elev, stream)
        ctx.save_for_backward(t, rh, valid, dtb_dt, dtb_de, dtb_ddz)
        ctx.mark_non_differentiable(valid)
        return tb, valid

    @staticmethod
    def backward(ctx, grad_tb, _grad_valid):
        t, rh, valid, dtb_dt, dtb_de, dtb_ddz = ctx.saved_tensors
        g = grad_tb.unsqueeze(-1)                                   # [nprof][nang][nf][1]
        keep = g != 0                                               # rows nobody asked about (e.g. NaN elevations) add nothing

        def contract(j):
            return torch.where(keep, j * g, torch.zeros((), dtype=j.dtype, device=j.device)).sum(dim=(1, 2))

        gt, ge, gdz = contract(dtb_dt), contract(dtb_de), contract(dtb_ddz)     # [nprof][nlev]
        es, des_dt = goff_gratch_es(t)
        grad_t = gt + ge * rh * des_dt
        grad_rh = ge * es
        grad_z = gdz - torch.nn.functional.pad(gdz[:, 1:], (0, 1))
        bad = (valid != 1).unsqueeze(-1)
        nan = torch.full((), float("nan"), dtype=grad_t.dtype, device=grad_t.device)
        grad_z, grad_t, grad_rh = (torch.where(bad, nan, x) for x in (grad_z, grad_t, grad_rh))
        return (grad_z if ctx.needs_input_grad[0] else None, grad_t if ctx.needs_input_grad[1] else None,
                grad_rh if ctx.needs_input_grad[2] else None, None, None, None, None, None)


class _BrightnessTemperatureCloudy(torch.autograd.Function):
    """The op under cloud liquid / ice: the clear op's backward plus grad_denliq = sum_{ang, f} g * dtb_dliq (ice alike)."""

    @staticmethod
    def forward(ctx, z, t, rh, denliq, denice, p, model, frq, elev, stream):
        tb, valid, dtb_dt, dtb_de, dtb_ddz, dtb_dliq, dtb_dice = _native_jacobian_cloudy(
            model, z, p, t, rh, denliq, denice, frq, elev, stream)
        ctx.has_liq, ctx.has_ice = dtb_dliq is not None, dtb_dice is not None
        ctx.save_for_backward(t, rh, valid, dtb_dt, dtb_de, dtb_ddz, *(x for x in (dtb_dliq, dtb_dice) if x is not None))
        ctx.mark_non_differentiable(valid)
        return tb, valid

    @staticmethod
    def backward(ctx, grad_tb, _grad_valid):
        t, rh, valid, dtb_dt, dtb_de, dtb_ddz, *cloud = ctx.saved_tensors
        dtb_dliq = cloud.pop(0) if ctx.has_liq else None
        dtb_dice = cloud.pop(0) if ctx.has_ice else None
        g = grad_tb.unsqueeze(-1)
        keep = g != 0

        def contract(j):
            return torch.where(keep, j * g, torch.zeros((), dtype=j.dtype, device=j.device)).sum(dim=(1, 2))

        gt, ge, gdz = contract(dtb_dt), contract(dtb_de), contract(dtb_ddz)
        es, des_dt = goff_gratch_es(t)
        grads = [gdz - torch.nn.functional.pad(gdz[:, 1:], (0, 1)), gt + ge * rh * des_dt, ge * es,
                 contract(dtb_dliq) if dtb_dliq is not None else None,
                 contract(dtb_dice) if dtb_dice is not None else None]
        bad = (valid != 1).unsqueeze(-1)
        nan = torch.full((), float("nan"), dtype=gt.dtype, device=gt.device)
        grads = [torch.where(bad, nan, x) if x is not None and ctx.needs_input_grad[k] else None
                 for k, x in enumerate(grads)]
        return (*grads, None, None, None, None, None)


def brightness_temperature(model, z, p, t, rh, frq, elev, stream=None, denliq=None, denice=None):
    """Plane-parallel downwelling TBs, differentiable with respect to z, t and rh -- and, under cloud, with respect to
    ``denliq`` / ``denice`` (cloud liquid / ice water content, g m-3, float64 [nprof][nlev] CUDA tensors; include/mwrt.h
    ``mwrt_tb_jacobian_batch_opt_device`` states the derivative conventions: an isolated cloudy level has none).

    model: a model name or ModelTables record; z [km], p [hPa], t [K], rh [fraction]: float64 [nprof][nlev] CUDA tensors,
    ground -> top; frq [GHz] and elev [deg] host arrays.  ``stream``: a hipStream_t handle (default: torch's current
    stream).  Returns ``tb [nprof][nang][nf]`` and ``valid [nprof]`` (uint8, include/mwrt.h).  With both cloud arguments
    None this is the clear-sky op; otherwise the forward is one ``mwrt_tb_batch_opt_device`` call without grad and one
    ``mwrt_tb_jacobian_batch_opt_device`` call with."""
    if p.requires_grad:
        raise NotImplementedError("brightness_temperature: no derivative with respect to pressure is computed")
    frq = np.ascontiguousarray(frq, dtype=np.float64).ravel()
    elev = np.ascontiguousarray(elev, dtype=np.float64).ravel()
    if denliq is not None or denice is not None:
        cloud = [x for x in (denliq, denice) if x is not None]
        if torch.is_grad_enabled() and any(x.requires_grad for x in (z, t, rh, *cloud)):
            return _BrightnessTemperatureCloudy.apply(z, t, rh, denliq, denice, p, model, frq, elev, stream)
        return _native_tb_cloudy(model, z.detach(), p, t.detach(), rh.detach(),
                                 None if denliq is None else denliq.detach(),
                                 None if denice is None else denice.detach(), frq, elev, stream)
    if torch.is_grad_enabled() and any(x.requires_grad for x in (z, t, rh)):
        return _BrightnessTemperature.apply(z, t, rh, p, model, frq, elev, stream)
    return _native_tb(model, z.detach(), p, t.detach(), rh.detach(), frq, elev, stream)
