"""Optimal-estimation (1D-Var) retrieval on the device: the K-matrix call and the Gauss-Newton update
(include/mwrt.h ``mwrt_oe_step_device``) back to back on one stream.

    ov = OneDVar("R24", frq, elev, sa, se, variables=JacVariables.of(humidity="rh"), blocks=("t", "h"), xa=xa)
    x_new, diag = ov.step(z, p, x, y)            # one K-matrix call + one update, nothing leaves the device
    res = ov.retrieve(z, p, y)                   # iterate from xa until every profile has converged
    res = ov.retrieve_lm(z, p, y)                # the same with Levenberg-Marquardt damping: no step may raise the cost
    ch = ov.characterise(z, p, res.x, y, avk=True, post_cov=True)   # gain, averaging kernel, posterior, error budget

The state ``x`` is ``[nprof][nblk][nlev]`` (float64, CUDA, levels ground -> top) with the blocks in the order given:
``"t"`` temperature [K], ``"h"`` humidity in the variable ``variables.humidity`` names (e [hPa], rh [fraction] or ppmv),
then optionally ``"liq"`` and ``"ice"`` in ``variables.cloud`` (g m-3 or kg/kg).  ``y`` is ``[nprof][nang][nf]`` (or
``[nprof][m]``); a NaN in it drops that observation.  ``sa`` is ``[n][n]`` with n = nblk * nlev, ``se`` ``[m]`` variances or
``[m][m]``, ``xa`` ``[nblk][nlev]`` shared or ``[nprof][nblk][nlev]``.  With ``variables.heights = "hydrostatic"`` the heights
are rebuilt from the state before every forward run (the rule of mwrt_jac_variables, anchored at ``z[:, 0]``); otherwise
``z`` is used as passed.  With ``instrument=`` (``instrument.Instrument``: antenna beam and channel bandpass)
the forward operator runs on the instrument's quadrature grid and ``mwrt_obs_apply_device`` reduces its TBs and K rows to
channels: ``y``, ``se`` and every diagnostic are then in channel space.

``step`` and ``retrieve`` take the undamped Gauss-Newton update, which is linear around x and may overshoot where the forward
model is not; ``retrieve_lm`` damps it (Levenberg-Marquardt, Rodgers 2000 eq. 5.36) on the split entries
``mwrt_oe_lm_prepare_device`` / ``mwrt_oe_lm_solve_device`` / ``mwrt_oe_cost_device``: one linearisation per accepted state,
one m x m solve per trial.  ``characterise`` returns what the undamped step at a state says about itself (Rodgers 2000, ch. 3;
DESIGN.md 4.6.2) on ``mwrt_oe_gain_device`` / ``mwrt_oe_product_device``.  Log-humidity states are not offered.

All of this is the m-form, an m x m system per profile with m <= 140.  ``OneDVar(..., form="n")`` runs ``step``, ``retrieve``
and ``retrieve_lm`` in the n-form instead (``mwrt_oe_nform_prepare_device`` / ``mwrt_oe_nform_solve_device`` /
``mwrt_oe_nform_cost_device``): an n x n system for a state of at most 128 elements -- the r coefficients of a basis, or a
coarse full state -- and any number of observations.  The constructor's ``se`` is then ``[m]`` variances; ``se=`` of a call as
``[nprof][m]`` goes straight in, as ``[nprof][m][m]`` through the pre-whitening below.  ``step(..., post_cov=True)`` returns the
posterior covariance it has formed anyway; ``characterise`` stays with ``form="m"`` and ``characterise_nform`` returns the
same ``Characterisation`` for ``form="n"`` (``mwrt_oe_nform_char_device`` / ``mwrt_oe_nform_gain_device``).

    ov = OneDVar("R24", frq, elev16, None, se, variables=..., blocks=("t", "h"), xa=xa, basis=eof, form="n")   # m = 224
    res = ov.retrieve(z, p, y)

With ``basis=StateBasis(b, sa_c)`` the retrieval runs in r coefficients of a basis shared by the batch, x = xa + B c
(DESIGN.md 4.9): ``mwrt_basis_project_device`` contracts the K rows with B behind the K-matrix call and the update sees the
single block K B ``[nprof][m][r]``, the state c, its prior ``c_a`` and its covariance ``sa_c``.

    eof = StateBasis.from_covariance(sa, 32)     # the leading eigenvectors of Sa, sa_c = diag(lambda)
    ov = OneDVar("R24", frq, elev, None, se, variables=..., blocks=("t", "h"), xa=xa, basis=eof)
    res = ov.retrieve(z, p, y)                   # res.x the physical state, res.coeff [nprof][r]

With ``se=`` on ``step``, ``retrieve``, ``retrieve_lm`` and ``characterise`` every profile has its own observation-error
covariance, ``[nprof][m]`` variances or ``[nprof][m][m]``: each linearisation is pre-whitened with the
Cholesky factor of the profile's Se_p on the rows it keeps (``mwrt_obs_whiten_device``, behind the instrument's reduction
and the basis projection) and the unchanged update entries run with Se = 1, which gives exactly the step of Se_p.

    se_p = noise[None] + ov.representation_error(z, p, x)            # K S_res K^T of a truncated basis, per profile
    res = ov.retrieve(z, p, y, se=se_p)

Which observations of a scan carry the information -- the greedy order by entropy reduction, the degrees of freedom along
it and the posterior after the picks -- is the business of the module ``selection`` (DESIGN.md 4.12;
``mwrt_oe_select_device``): ``selection.rank_observations(ov, z, p, x)`` takes a ``OneDVar`` of either form.

The tensor contract.  The library is handed bare pointers and reads contiguous doubles behind them on the
GPU, so every tensor argument of this module -- the constructor's ``sa``, ``se``, ``xa``, ``StateBasis``'s ``b``, ``sa_c``,
``c_a``, and ``z``, ``p``, ``x``, ``x0``, ``y``, ``se=`` of every public method -- must be a float64 ``torch.Tensor`` of the
stated shape, on the device of ``xa`` (the three of a ``StateBasis`` on one device of their own: the constructor copies
them to xa's).  Another dtype, a NumPy array or a list, another shape, another device, or a per-profile ``xa`` / ``c_a``
whose nprof is not the call's is a ``ValueError`` naming the argument: nothing is converted, and nothing has reached the
library by then.  Any strides are taken (an ``.expand``, a slice of a larger buffer, permuted storage, an offset): each
argument is made contiguous once, at entry, and a call gives the same bits as on contiguous clones.  With the native
context only CUDA tensors pass (``_context``).  NaN values are not refused: the kernels answer those with a status."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native
from ._native import JacVariables
from .autodiff import goff_gratch_es


def _checked(name, v, *shapes, device=None, want=None):
    """The one check of a tensor argument of this module: ``v`` must be a float64 tensor in one of ``shapes`` (tuples of
    sizes; None or a string stands for any size and is printed as ``*`` or as itself) and, with ``device``, on that device.
    Returns it contiguous: any strides are taken, and made contiguous here, once.  Another dtype is refused, not converted,
    and so is anything that is not a tensor (``want`` replaces the words after "expected" in the message)."""
    if want is None:
        want = "a float64 tensor " + " or ".join(
            "".join(f"[{'*' if d is None else d}]" for d in s) for s in shapes)
    if not torch.is_tensor(v):
        raise ValueError(f"{name}: expected {want}, got {type(v).__name__}")
    fits = lambda s: len(s) == v.dim() and all(not isinstance(d, int) or d == k for d, k in zip(s, v.shape))   # noqa: E731
    if v.dtype != torch.float64 or not any(fits(s) for s in shapes):
        raise ValueError(f"{name}: expected {want}, got {v.dtype} {tuple(v.shape)}")
    if device is not None and v.device != device:
        raise ValueError(f"{name}: expected {want} on {device} (the device of xa), got one on {v.device}")
    return v.contiguous()


def _context(ref):
    """The context whose entries take the pointers of tensors on the device of ``ref``: the one place this module asks
    for one.  The library reads every pointer on the GPU, so with the native context a tensor anywhere else is refused
    here; a stand-in context (CPU tests) takes what it is given."""
    ctx = _native.default_context(ref.device.index or 0)
    if isinstance(ctx, _native.Context) and not ref.is_cuda:
        raise ValueError(f"expected CUDA tensors: the native library reads device pointers, got a tensor on {ref.device}")
    return ctx


def _k_matrix(entry, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
    """The body of the two K-matrix seams: one call of ``entry(context, ...)``, the context method either of them names."""
    nprof, nlev = z.shape
    opts = dict(dtype=torch.float64, device=z.device)
    tb = torch.empty((nprof, elev.size, frq.size), **opts)
    rows = {b: torch.empty((nprof, elev.size, frq.size, nlev), **opts) for b in want}
    valid = torch.empty(nprof, dtype=torch.uint8, device=z.device)
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    entry(
        _context(z), model, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, elev, tb.data_ptr(),
        rows["t"].data_ptr(), rows["h"].data_ptr(), valid.data_ptr(), d_denliq=ptr(denliq), d_denice=ptr(denice),
        d_dtb_dliq=ptr(rows.get("liq")), d_dtb_dice=ptr(rows.get("ice")), variables=variables, stream=stream)
    return tb, valid, rows


def _native_k_matrix(model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
    """One ``mwrt_tb_jacobian_batch_vars_device`` call -> (tb [nprof][nang][nf], valid, {block: K rows [nprof][nang][nf][nlev]}).

    The single place the K-matrix of this module reaches the native library: CPU tests substitute a stand-in here."""
    entry = lambda ctx, *args, **kw: ctx.tb_jacobian_batch_vars_device(*args, **kw)   # noqa: E731
    return _k_matrix(entry, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream)


def _native_k_matrix_ray(model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream):
    """One ``mwrt_tb_jacobian_batch_ray_device`` call: ``_native_k_matrix`` along refracted spherical ray paths, what
    ``OneDVar(..., ray_tracing=True)`` runs instead.  CPU tests substitute a stand-in here."""
    entry = lambda ctx, *args, **kw: ctx.tb_jacobian_batch_ray_device(*args, **kw)   # noqa: E731
    return _k_matrix(entry, model, z, p, t, rh, denliq, denice, frq, elev, variables, want, stream)


def _native_oe_step(k_blocks, x, xa, sa, se, y, fx, want_post_var, stream):
    """One ``mwrt_oe_step_device`` call -> dict(x_new, status, chi2, dfs, nobs, post_var or None).

    The single place the update reaches the native library: CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    m = y.shape[1]
    opts = dict(dtype=torch.float64, device=x.device)
    out = dict(x_new=torch.empty_like(x), status=torch.empty(nprof, dtype=torch.uint8, device=x.device),
               chi2=torch.empty(nprof, **opts), dfs=torch.empty(nprof, **opts),
               nobs=torch.empty(nprof, dtype=torch.int32, device=x.device),
               post_var=torch.empty_like(x) if want_post_var else None)
    _context(x).oe_step_device(
        nprof, nlev, m, [k.data_ptr() for k in k_blocks], x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(),
        y.data_ptr(), fx.data_ptr(), out["x_new"].data_ptr(), out["status"].data_ptr(), d_chi2=out["chi2"].data_ptr(),
        d_dfs=out["dfs"].data_ptr(), d_post_var=None if out["post_var"] is None else out["post_var"].data_ptr(),
        d_nobs=out["nobs"].data_ptr(), xa_per_profile=xa.dim() == 3, se_full=se.dim() == 2, stream=stream)
    return out


def _native_oe_lm_prepare(k_blocks, x, xa, sa, se, y, fx, lin, active, stream):
    """One ``mwrt_oe_lm_prepare_device`` call: fills ``lin`` (dict of g0, r, kdx, keep, lin_status) in place for the profiles
    whose ``active`` flag (uint8) is set.  CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    _context(x).oe_lm_prepare_device(
        nprof, nlev, y.shape[1], [k.data_ptr() for k in k_blocks], x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(),
        y.data_ptr(), fx.data_ptr(), lin["g0"].data_ptr(), lin["r"].data_ptr(), lin["kdx"].data_ptr(), lin["keep"].data_ptr(),
        lin["lin_status"].data_ptr(), d_active=active.data_ptr(), xa_per_profile=xa.dim() == 3, se_full=se.dim() == 2,
        stream=stream)


def _native_oe_lm_solve(k_blocks, x, xa, sa, se, gamma, lin, out, active, stream):
    """One ``mwrt_oe_lm_solve_device`` call: the damped trial of every active profile into ``out`` (dict of x_new, status) in
    place.  CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    _context(x).oe_lm_solve_device(
        nprof, nlev, lin["r"].shape[1], [k.data_ptr() for k in k_blocks], x.data_ptr(), xa.data_ptr(), sa.data_ptr(),
        se.data_ptr(), gamma.data_ptr(), lin["g0"].data_ptr(), lin["r"].data_ptr(), lin["kdx"].data_ptr(),
        lin["keep"].data_ptr(), lin["lin_status"].data_ptr(), out["x_new"].data_ptr(), out["status"].data_ptr(),
        d_active=active.data_ptr(), xa_per_profile=xa.dim() == 3, se_full=se.dim() == 2, stream=stream)


def _native_oe_cost(x, xa, se, y, fx, keep, sa_inv, cost, active, stream):
    """One ``mwrt_oe_cost_device`` call: J at ``x`` on the rows ``keep`` names into ``cost`` in place, active profiles only.
    CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    _context(x).oe_cost_device(
        nprof, nlev, y.shape[1], nblk, x.data_ptr(), xa.data_ptr(), se.data_ptr(), y.data_ptr(), fx.data_ptr(),
        keep.data_ptr(), sa_inv.data_ptr(), cost.data_ptr(), d_active=active.data_ptr(), xa_per_profile=xa.dim() == 3,
        se_full=se.dim() == 2, stream=stream)


def _native_oe_nform_prepare(k_blocks, x, xa, se, y, fx, lin, active, stream):
    """One ``mwrt_oe_nform_prepare_device`` call: fills ``lin`` (dict of h, g, rwr, keep, nobs, lin_status) in place, for the
    profiles whose ``active`` flag (uint8) is set or, with ``active=None``, for all.  ``se`` holds variances, ``[m]`` or
    ``[nprof][m]``.  CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    _context(x).oe_nform_prepare_device(
        nprof, nlev, y.shape[1], [k.data_ptr() for k in k_blocks], x.data_ptr(), xa.data_ptr(), se.data_ptr(), y.data_ptr(),
        fx.data_ptr(), lin["h"].data_ptr(), lin["g"].data_ptr(), lin["rwr"].data_ptr(), lin["keep"].data_ptr(),
        lin["nobs"].data_ptr(), lin["lin_status"].data_ptr(), d_active=None if active is None else active.data_ptr(),
        xa_per_profile=xa.dim() == 3, se_per_profile=se.dim() == 2, stream=stream)


def _native_oe_nform_solve(x, xa, sa_inv, lin, gamma, out, active, stream):
    """One ``mwrt_oe_nform_solve_device`` call on the linearisation ``lin`` into ``out`` in place: x_new and status, and --
    with ``gamma=None`` only -- whichever of chi2, dfs, post_var and post_cov it holds a tensor for.  CPU tests substitute
    the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    _context(x).oe_nform_solve_device(
        nprof, nlev, lin["keep"].shape[1], nblk, x.data_ptr(), xa.data_ptr(), sa_inv.data_ptr(), lin["h"].data_ptr(),
        lin["g"].data_ptr(), lin["rwr"].data_ptr(), lin["lin_status"].data_ptr(), out["x_new"].data_ptr(),
        out["status"].data_ptr(), d_gamma=ptr(gamma), d_chi2=ptr(out.get("chi2")), d_dfs=ptr(out.get("dfs")),
        d_post_var=ptr(out.get("post_var")), d_post_cov=ptr(out.get("post_cov")), d_active=ptr(active),
        xa_per_profile=xa.dim() == 3, stream=stream)


def _native_oe_nform_cost(x, xa, sa_inv, se, y, fx, keep, cost, active, stream):
    """One ``mwrt_oe_nform_cost_device`` call: J at ``x`` on the rows ``keep`` names into ``cost`` in place, active profiles
    only.  CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    _context(x).oe_nform_cost_device(
        nprof, nlev, y.shape[1], nblk, x.data_ptr(), xa.data_ptr(), sa_inv.data_ptr(), se.data_ptr(), y.data_ptr(),
        fx.data_ptr(), keep.data_ptr(), cost.data_ptr(), d_active=None if active is None else active.data_ptr(),
        xa_per_profile=xa.dim() == 3, se_per_profile=se.dim() == 2, stream=stream)


def _native_oe_nform_char(sa_inv, lin, nblk, out, rows, stream):
    """One ``mwrt_oe_nform_char_device`` call on the linearisation ``lin`` into ``out`` in place: status, and whichever of
    post_cov ``[nprof][n][n]``, avk ``[nprof][rows][n]`` (``rows = (begin, count)``, (0, 0): all), avk_diag, noise_var,
    smooth_var ``[nprof][nblk][nlev]`` and dfs_block ``[nprof][nblk]`` it holds a tensor for.  CPU tests substitute the
    NumPy reference here."""
    nprof, n = lin["g"].shape
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    _context(sa_inv).oe_nform_char_device(
        nprof, n // nblk, lin["keep"].shape[1], nblk, sa_inv.data_ptr(), lin["h"].data_ptr(), lin["lin_status"].data_ptr(),
        out["status"].data_ptr(), d_post_cov=ptr(out.get("post_cov")), d_avk=ptr(out.get("avk")),
        d_avk_diag=ptr(out.get("avk_diag")), d_dfs_block=ptr(out.get("dfs_block")), d_noise_var=ptr(out.get("noise_var")),
        d_smooth_var=ptr(out.get("smooth_var")), row_begin=rows[0], row_count=rows[1], stream=stream)


def _native_oe_nform_gain(k_blocks, se, keep, post_cov, status, stream):
    """One ``mwrt_oe_nform_gain_device`` call -> gain ``[nprof][m][n]`` from the K blocks ``[nprof]...[nlev]``, the
    variances ``se`` (``[m]`` or ``[nprof][m]``), prepare's ``keep`` and the ``post_cov`` and ``status`` the characterisation
    wrote.  CPU tests substitute the NumPy reference here."""
    nprof, m = keep.shape
    n = post_cov.shape[-1]
    gain = torch.empty((nprof, m, n), dtype=torch.float64, device=keep.device)
    _context(keep).oe_nform_gain_device(
        nprof, n // len(k_blocks), m, [k.data_ptr() for k in k_blocks], se.data_ptr(), keep.data_ptr(), post_cov.data_ptr(),
        status.data_ptr(), gain.data_ptr(), se_per_profile=se.dim() == 2, stream=stream)
    return gain


def _native_oe_gain(k_blocks, x, xa, sa, se, y, fx, stream):
    """One ``mwrt_oe_gain_device`` call with every output -> dict(gain, ksa, keep, avk_diag, dfs_block, noise_var,
    smooth_var, status, nobs).

    The single place the gain reaches the native library: CPU tests substitute the NumPy reference here."""
    nprof, nblk, nlev = x.shape
    m, n = y.shape[1], nblk * nlev
    f64 = dict(dtype=torch.float64, device=x.device)
    out = dict(gain=torch.empty((nprof, m, n), **f64), ksa=torch.empty((nprof, m, n), **f64),
               keep=torch.empty((nprof, m), dtype=torch.uint8, device=x.device), avk_diag=torch.empty_like(x),
               dfs_block=torch.empty((nprof, nblk), **f64), noise_var=torch.empty_like(x), smooth_var=torch.empty_like(x),
               status=torch.empty(nprof, dtype=torch.uint8, device=x.device),
               nobs=torch.empty(nprof, dtype=torch.int32, device=x.device))
    _context(x).oe_gain_device(
        nprof, nlev, m, [k.data_ptr() for k in k_blocks], x.data_ptr(), xa.data_ptr(), sa.data_ptr(), se.data_ptr(),
        y.data_ptr(), fx.data_ptr(), out["status"].data_ptr(), d_gain=out["gain"].data_ptr(), d_ksa=out["ksa"].data_ptr(),
        d_keep=out["keep"].data_ptr(), d_avk_diag=out["avk_diag"].data_ptr(), d_dfs_block=out["dfs_block"].data_ptr(),
        d_noise_var=out["noise_var"].data_ptr(), d_smooth_var=out["smooth_var"].data_ptr(), d_nobs=out["nobs"].data_ptr(),
        xa_per_profile=xa.dim() == 3, se_full=se.dim() == 2, stream=stream)
    return out


def _native_oe_product(product, gain, keep, k_blocks, ksa, sa, rows, stream):
    """One ``mwrt_oe_product_device`` call -> [nprof][count][n]: ``product`` "avk" (gain K) or "post_cov" (Sa - gain W),
    rows ``rows = (begin, count)`` ((0, 0): all).

    The single place the products reach the native library: CPU tests substitute the NumPy reference here."""
    nprof, m, n = gain.shape
    nlev = n // len(k_blocks)
    out = torch.empty((nprof, rows[1] or n, n), dtype=torch.float64, device=gain.device)
    _context(gain).oe_product_device(
        nprof, nlev, m, _native.OE_PRODUCT_AVK if product == "avk" else _native.OE_PRODUCT_POST_COV, gain.data_ptr(),
        keep.data_ptr(), out.data_ptr(), [k.data_ptr() for k in k_blocks], d_ksa=ksa.data_ptr(), d_sa=sa.data_ptr(),
        row_begin=rows[0], row_count=rows[1], stream=stream)
    return out


def _native_obs_apply(instrument, tb, k_blocks, stream):
    """One ``mwrt_obs_apply_device`` call -> (tb_ch [nprof][nang][nch] or None, list of K blocks [nprof][nang][nch][nlev] or
    None) from ``tb [nprof][nang_q][nf_q]`` and / or the K blocks ``[nprof][nang_q][nf_q][nlev]`` on the instrument's
    quadrature grid.

    The single place the instrument's reduction reaches the native library: CPU tests substitute the NumPy reference here."""
    k_blocks = None if k_blocks is None else list(k_blocks)
    ref = tb if tb is not None else k_blocks[0]
    named = [("tb", tb)] + [(f"k_blocks[{i}]", k) for i, k in enumerate(k_blocks or [])]
    for name, v in named:                                     # ``Instrument.apply`` hands over the caller's tensors
        if v is not None and not torch.is_tensor(v):
            raise ValueError(f"{name}: expected a float64 tensor, got {type(v).__name__}")
    if len({v.device for _, v in named if v is not None}) > 1:
        raise ValueError("tb and k_blocks: expected tensors on one device, got "
                         + ", ".join(f"{name} on {v.device}" for name, v in named if v is not None))
    nprof = ref.shape[0] if ref.dim() else 0
    nang, nch = instrument.elev.size, instrument.frq.size
    grid = f"[{instrument.elev_q.size}][{instrument.frq_q.size}]"
    opts = dict(dtype=torch.float64, device=ref.device)
    if tb is not None and (tb.dtype != torch.float64 or tb.dim() < 2 or tb[0].numel() != instrument.m_in):
        raise ValueError(f"tb: expected float64 [nprof]{grid} (or [nprof][{instrument.m_in}]), got {tb.dtype} {tuple(tb.shape)}")
    nlev = k_blocks[0].shape[-1] if k_blocks and k_blocks[0].dim() else 1
    for i, k in enumerate(k_blocks or []):
        if k.dtype != torch.float64 or k.dim() < 3 or k.shape[0] != nprof or k.shape[-1] != nlev or \
                k[0].numel() != instrument.m_in * nlev:
            raise ValueError(f"k_blocks[{i}]: expected float64 [{nprof}]{grid}[{nlev}], got {k.dtype} {tuple(k.shape)}")
    k_blocks = None if k_blocks is None else [k.contiguous() for k in k_blocks]
    tb_in = None if tb is None else tb.contiguous()
    tb_out = None if tb is None else torch.empty((nprof, nang, nch), **opts)
    k_out = None if k_blocks is None else [torch.empty((nprof, nang, nch, nlev), **opts) for _ in k_blocks]
    ctx, handle = instrument.native_handle(ref.device.index or 0, ctx=_context(ref))
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    ctx.obs_apply_device(handle, nprof, nlev, d_tb_in=ptr(tb_in), d_tb_out=ptr(tb_out),
                         d_k_in=[k.data_ptr() for k in k_blocks or []], d_k_out=[k.data_ptr() for k in k_out or []],
                         stream=stream)
    return tb_out, k_out


def _native_basis_project(basis, k_blocks, stream):
    """One ``mwrt_basis_project_device`` call -> K B ``[nprof][m][r]`` from the K blocks ``[nprof]...[nlev]`` in the state's
    order (the K-matrix call's, or the instrument's channel rows).

    The single place the projection reaches the native library: CPU tests substitute the NumPy reference here."""
    k_blocks = [k.contiguous() for k in k_blocks]
    nprof, nlev = k_blocks[0].shape[0], k_blocks[0].shape[-1]
    for i, k in enumerate(k_blocks):
        if k.dtype != torch.float64 or k.shape != k_blocks[0].shape:
            raise ValueError(f"k_blocks[{i}]: expected float64 {tuple(k_blocks[0].shape)}, got {k.dtype} {tuple(k.shape)}")
    if len(k_blocks) * nlev != basis.n:
        raise ValueError(f"basis: expected b [{len(k_blocks) * nlev}][r] for {len(k_blocks)} blocks of {nlev} levels, got "
                         f"{tuple(basis.b.shape)}")
    m = k_blocks[0][0].numel() // nlev
    out = torch.empty((nprof, m, basis.r), dtype=torch.float64, device=k_blocks[0].device)
    ctx, handle = basis.native_handle(len(k_blocks), k_blocks[0].device.index or 0, ctx=_context(k_blocks[0]))
    ctx.basis_project_device(handle, nprof, m, [k.data_ptr() for k in k_blocks], out.data_ptr(), stream=stream)
    return out


def _native_basis_expand(basis, c, x_ref, stream):
    """One ``mwrt_basis_expand_device`` call -> x_ref + B c ``[nprof][nblk][nlev]`` from ``c [nprof][r]`` and ``x_ref
    [nblk][nlev]`` (shared) or ``[nprof][nblk][nlev]``.

    The single place the expansion reaches the native library: CPU tests substitute the NumPy reference here."""
    nprof = c.shape[0]
    nblk, nlev = x_ref.shape[-2:]
    if c.dtype != torch.float64 or tuple(c.shape) != (nprof, basis.r) or x_ref.dtype != torch.float64 or \
            nblk * nlev != basis.n or x_ref.dim() not in (2, 3) or (x_ref.dim() == 3 and x_ref.shape[0] != nprof):
        raise ValueError(f"expected float64 c [{nprof}][{basis.r}] and x_ref [nblk][nlev] or [{nprof}][nblk][nlev] with nblk nlev = "
                         f"{basis.n}, got {c.dtype} {tuple(c.shape)} and {x_ref.dtype} {tuple(x_ref.shape)}")
    c, x_ref = c.contiguous(), x_ref.contiguous()
    out = torch.empty((nprof, nblk, nlev), dtype=torch.float64, device=c.device)
    ctx, handle = basis.native_handle(nblk, c.device.index or 0, ctx=_context(c))
    ctx.basis_expand_device(handle, nprof, c.data_ptr(), x_ref.data_ptr(), out.data_ptr(), x_ref_per_profile=x_ref.dim() == 3,
                            stream=stream)
    return out


def _native_obs_whiten(k_blocks, se, y, fx, stream):
    """One ``mwrt_obs_whiten_device`` call -> dict(k: list of L^-1 K blocks in the shapes given, y, fx: L^-1 y and L^-1 F
    ``[nprof][m]``, l ``[nprof][m (m + 1) / 2]``, keep ``[nprof][m]`` and status ``[nprof]`` uint8) from the K blocks
    ``[nprof]...[nlev]`` the update would see, ``se [nprof][m]`` or ``[nprof][m][m]`` and ``y``, ``fx [nprof][m]``.

    The single place the pre-whitening reaches the native library: CPU tests substitute the NumPy reference here."""
    k_blocks = [k.contiguous() for k in k_blocks]
    nprof, m = y.shape
    nlev = k_blocks[0].shape[-1] if k_blocks else 1
    for i, k in enumerate(k_blocks):
        if k.dtype != torch.float64 or k.shape[0] != nprof or k.shape[-1] != nlev or k[0].numel() != m * nlev:
            raise ValueError(f"k_blocks[{i}]: expected float64 [{nprof}][{m}][{nlev}], got {k.dtype} {tuple(k.shape)}")
    if se.dtype != torch.float64 or tuple(se.shape) not in ((nprof, m), (nprof, m, m)):
        raise ValueError(f"se: expected float64 [{nprof}][{m}] or [{nprof}][{m}][{m}], got {se.dtype} {tuple(se.shape)}")
    se, y, fx = se.contiguous(), y.contiguous(), fx.contiguous()
    f64, u8 = dict(dtype=torch.float64, device=y.device), dict(dtype=torch.uint8, device=y.device)
    out = dict(k=[torch.empty_like(k) for k in k_blocks], y=torch.empty_like(y), fx=torch.empty_like(fx),
               l=torch.empty((nprof, m * (m + 1) // 2), **f64), keep=torch.empty((nprof, m), **u8),
               status=torch.empty(nprof, **u8))
    _context(y).obs_whiten_device(
        nprof, nlev, m, se.data_ptr(), y.data_ptr(), fx.data_ptr(), [k.data_ptr() for k in k_blocks], out["l"].data_ptr(),
        out["keep"].data_ptr(), out["status"].data_ptr(), d_y_out=out["y"].data_ptr(), d_fx_out=out["fx"].data_ptr(),
        d_k_out=[k.data_ptr() for k in out["k"]], se_full=se.dim() == 3, stream=stream)
    return out


def _native_obs_whiten_apply(l, keep, mode, vec, block, stream):
    """One ``mwrt_obs_whiten_apply_device`` call with a stored factor: ``mode`` 0 is L^-1, 1 is L^-T, on ``vec [nprof][m]``
    and / or ``block [nprof][m][ncol]`` (either may be None) -> (vec_out or None, block_out or None).

    The single place the stored factor reaches the native library: CPU tests substitute the NumPy reference here."""
    nprof, m = keep.shape
    vec = None if vec is None else vec.contiguous()
    block = None if block is None else block.contiguous()
    v_out = None if vec is None else torch.empty_like(vec)
    b_out = None if block is None else torch.empty_like(block)
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    _context(keep).obs_whiten_apply_device(
        nprof, 1 if block is None else block.shape[-1], m, l.data_ptr(), keep.data_ptr(), mode=mode, d_y=ptr(vec),
        d_y_out=ptr(v_out), d_k_in=[] if block is None else [block.data_ptr()],
        d_k_out=[] if block is None else [b_out.data_ptr()], stream=stream)
    return v_out, b_out


class StateBasis:
    """A reduced basis for the state of ``OneDVar``: x = xa + B c with ``b [n][r]`` (n = nblk * nlev, state index = block *
    nlev + level; float64), the prior covariance of the coefficients ``sa_c [r][r]`` and their prior mean ``c_a`` (``[r]``
    shared or ``[nprof][r]``; default 0, so that the prior state is ``OneDVar``'s ``xa``).  The columns may be anything
    fixed for the batch: leading EOFs of a prior ensemble (``from_covariance``), coarse layers, or a single column that
    scales a liquid-water profile shape.  The device copy of B is made once per device and context, on first use."""

    def __init__(self, b, sa_c, c_a=None):
        b = _checked("b", b, ("n", "r"), want="float64 [n][r], a tensor")
        self.n, self.r = int(b.shape[0]), int(b.shape[1])
        r = self.r
        sa_c = _checked("sa_c", sa_c, (r, r), want=f"[{r}][{r}], a float64 tensor")
        c_a = torch.zeros(r, dtype=torch.float64, device=b.device) if c_a is None else c_a
        c_a = _checked("c_a", c_a, (r,), ("nprof", r), want=f"[{r}] or [nprof][{r}], a float64 tensor")
        if not b.device == sa_c.device == c_a.device:
            raise ValueError(f"b, sa_c and c_a: expected on one device, got b on {b.device}, sa_c on {sa_c.device} and c_a "
                             f"on {c_a.device}")
        self.b, self.sa_c, self.c_a = b, sa_c, c_a
        self.sa_res = None         # [n][n] what the basis leaves out of the prior covariance (``from_covariance`` sets it)
        self._handles = {}

    @classmethod
    def from_covariance(cls, sa, r, c_a=None):
        """The leading ``r`` eigenvectors of ``sa [n][n]`` as columns (largest eigenvalue first), ``sa_c = diag(lambda)``.
        The sign of each column is fixed so that its largest-magnitude component is positive; B^T B = I.  The truncated
        part ``sa - B diag(lambda) B^T``, symmetrised, is kept as ``sa_res [n][n]`` (formed in torch on the host): what
        ``OneDVar.representation_error`` turns into the observation-error term of the truncation."""
        sa = torch.as_tensor(sa)
        n = sa.shape[0]
        if sa.dim() != 2 or sa.shape[1] != n or not 1 <= int(r) <= n:
            raise ValueError(f"expected sa [n][n] and 1 <= r <= n, got {tuple(sa.shape)} and r = {r}")
        s64 = sa.detach().to("cpu", torch.float64)
        lam, vec = torch.linalg.eigh(0.5 * (s64 + s64.T))
        lam, vec = lam.flip(0)[:r], vec.flip(1)[:, :r]
        top = vec.abs().argmax(dim=0)
        vec = vec * torch.where(vec[top, torch.arange(int(r))] < 0, -1.0, 1.0).to(torch.float64)[None, :]
        basis = cls(vec.contiguous().to(sa.device), torch.diag(lam).to(sa.device), c_a)
        res = 0.5 * (s64 + s64.T) - (vec * lam[None, :]) @ vec.T
        basis.sa_res = (0.5 * (res + res.T)).contiguous().to(sa.device)
        return basis

    def native_handle(self, nblk, device_index=0, ctx=None):
        """(context, basis handle) for ``nblk`` blocks on a device: created on first use, released with the object.  ``ctx``
        is the context to create it on (default: ``_native.default_context(device_index)``)."""
        key = (int(nblk), device_index)
        hit = self._handles.get(key)
        if hit is None or hit[0]._handle is None or (ctx is not None and hit[0] is not ctx):   # first use, or the context
            if hit is not None:                                                              # was closed or replaced since
                hit[0].basis_destroy(hit[1])
            if self.n % int(nblk) != 0:
                raise ValueError(f"basis: b [{self.n}][{self.r}] does not split into {nblk} blocks")
            ctx = _native.default_context(device_index) if ctx is None else ctx
            hit = self._handles[key] = (ctx, ctx.basis_create(nblk, self.n // int(nblk), self.b.detach().cpu().numpy()))
        return hit

    def close(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for ctx, h in handles.values():
            ctx.basis_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Characterisation:
    """What ``OneDVar.characterise`` returns: the undamped step at a state, described (Rodgers 2000, ch. 3; include/mwrt.h
    mwrt_oe_gain_device).  Every field is a tensor on the state's device; n = nblk * nlev, state index = block * nlev + level.
    With a basis the step is the one in the coefficients: n = r and nblk = 1 in every field, ``coeff`` is the state."""
    gain: Optional[torch.Tensor]   # [nprof][m][n] row i: the contribution function d x^ / d y_i; 0 in a dropped row (None:
    #                                ``characterise_nform(gain=False)``)
    avk_diag: torch.Tensor     # [nprof][nblk][nlev] diagonal of the averaging kernel
    dfs_block: torch.Tensor    # [nprof][nblk] degrees of freedom for signal per state block; their sum is the step's dfs
    noise_var: torch.Tensor    # [nprof][nblk][nlev] measurement-noise part of the posterior variance
    smooth_var: torch.Tensor   # [nprof][nblk][nlev] smoothing part; noise_var + smooth_var = diag of the posterior
    status: torch.Tensor       # [nprof] uint8, mwrt_oe_step_device's status
    nobs: torch.Tensor         # [nprof] int32 observations used
    keep: torch.Tensor         # [nprof][m] uint8, 1: the observation was used
    avk: Optional[torch.Tensor] = None        # [nprof][rows][n] averaging kernel d x^ / d x (``avk=True``)
    post_cov: Optional[torch.Tensor] = None   # [nprof][rows][n] posterior covariance (``post_cov=True``)
    coeff: Optional[torch.Tensor] = None      # [nprof][r] the coefficients the step was characterised at (with a basis)


@dataclass
class Retrieval:
    """What ``OneDVar.retrieve`` and ``retrieve_lm`` return; every field is a tensor on the state's device."""
    x: torch.Tensor            # [nprof][nblk][nlev] the retrieved state
    chi2: torch.Tensor         # [nprof] d^T G^-1 d of each profile's last step
    dfs: torch.Tensor          # [nprof] degrees of freedom for signal
    post_var: torch.Tensor     # [nprof][nblk][nlev] diagonal of the posterior covariance
    status: torch.Tensor       # [nprof] uint8, mwrt_oe_step_device's status of the last step
    nobs: torch.Tensor         # [nprof] int32 observations used
    iterations: torch.Tensor   # [nprof] int32 steps taken before the profile was frozen
    converged: torch.Tensor    # [nprof] bool
    cost: Optional[torch.Tensor] = None    # [nprof] J at x (``retrieve_lm`` only)
    gamma: Optional[torch.Tensor] = None   # [nprof] the damping factor the profile ended with (``retrieve_lm`` only)
    coeff: Optional[torch.Tensor] = None   # [nprof][r] the retrieved coefficients (with a basis; x = clamp(xa + B coeff))


class _MForm:
    """What the m-form of the update does its own way (an m x m system per profile: ``mwrt_oe_step_device`` and the
    ``mwrt_oe_lm_*`` split): how ``se=`` of a call is prepared, the buffers of a linearisation, prepare / cost / solve on
    them, and the undamped update with its diagnostics.  ``OneDVar`` holds one of ``_MForm`` and ``_NForm`` as ``_form``;
    everything around these five -- the step, the damped loop, the iteration -- is written once."""

    def __init__(self, ov):
        self.ov = ov

    def se(self, se_p, k_blocks, y, fx, stream):
        """``(k_blocks, y, fx, se, w)`` as the entries are given them: a per-profile Se is always pre-whitened."""
        return self.ov._whiten(se_p, k_blocks, y, fx, stream)

    @staticmethod
    def lin(nprof, n, m, dev):
        """The buffers of one linearisation (``mwrt_oe_lm_prepare_device`` writes them)."""
        f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
        return dict(g0=torch.zeros((nprof, m * (m + 1) // 2), **f64), r=torch.zeros((nprof, m), **f64),
                    kdx=torch.zeros((nprof, m), **f64), keep=torch.zeros((nprof, m), **u8), lin_status=torch.zeros(nprof, **u8))

    def prepare(self, k_blocks, x, se, y, fx, lin, active, stream):
        _native_oe_lm_prepare(k_blocks, x, self.ov._prior_mean, self.ov._prior_cov, se, y, fx, lin, active, stream)

    def cost(self, x, se, y, fx, keep, cost, active, stream):
        _native_oe_cost(x, self.ov._prior_mean, se, y, fx, keep, self.ov.sa_inv, cost, active, stream)

    def solve(self, k_blocks, x, se, gamma, lin, out, active, stream):
        _native_oe_lm_solve(k_blocks, x, self.ov._prior_mean, self.ov._prior_cov, se, gamma, lin, out, active, stream)

    def update(self, k_blocks, u, se, y, fx, stream, post_var, post_cov=False, lin=None):
        """The undamped step at the update's state ``u`` on what ``se`` returned -> dict(x_new, status, chi2, dfs, nobs,
        post_var or None): one ``_native_oe_step`` call; with a basis ``post_var`` is ``_post_var_levels``.  ``post_cov``
        and ``lin`` are the n-form's."""
        ov = self.ov
        out = _native_oe_step(k_blocks, u, ov._prior_mean, ov._prior_cov, se, y, fx, post_var and ov.basis is None, stream)
        if post_var and ov.basis is not None:
            out["post_var"] = ov._post_var_levels(k_blocks, u, y, fx, stream, se)
        return out


class _NForm(_MForm):
    """The same five for the n-form (an n x n system per profile, any m; ``mwrt_oe_nform_*_device``)."""

    def se(self, se_p, k_blocks, y, fx, stream):
        """The constructor's variances ``[m]``; per-profile variances ``[nprof][m]`` as they are (the entries'
        se_per_profile; nothing is whitened, w is None); a per-profile full covariance ``[nprof][m][m]`` through the
        pre-whitening, then variances of 1."""
        if se_p is not None and se_p.dim() == 2:
            return k_blocks, y, fx, se_p, None
        return self.ov._whiten(se_p, k_blocks, y, fx, stream)

    @staticmethod
    def lin(nprof, n, m, dev):
        """The buffers of one n-form linearisation (``mwrt_oe_nform_prepare_device`` writes them)."""
        f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
        return dict(h=torch.zeros((nprof, n * (n + 1) // 2), **f64), g=torch.zeros((nprof, n), **f64), rwr=torch.zeros(nprof, **f64),
                    keep=torch.zeros((nprof, m), **u8), nobs=torch.zeros(nprof, dtype=torch.int32, device=dev),
                    lin_status=torch.zeros(nprof, **u8))

    def prepare(self, k_blocks, x, se, y, fx, lin, active, stream):
        _native_oe_nform_prepare(k_blocks, x, self.ov._prior_mean, se, y, fx, lin, active, stream)

    def cost(self, x, se, y, fx, keep, cost, active, stream):
        _native_oe_nform_cost(x, self.ov._prior_mean, self.ov.sa_inv, se, y, fx, keep, cost, active, stream)

    def solve(self, k_blocks, x, se, gamma, lin, out, active, stream):
        _native_oe_nform_solve(x, self.ov._prior_mean, self.ov.sa_inv, lin, gamma, out, active, stream)

    def update(self, k_blocks, u, se, y, fx, stream, post_var, post_cov=False, lin=None):
        """The undamped n-form step at ``u``: one prepare (into ``lin``, all profiles) and one solve -> dict(x_new, status,
        chi2, dfs, nobs, post_var or None[, post_cov [nprof][n][n]]).  With a basis ``post_var`` is the level-space
        diag(B S^_c B^T) from the solve's C^-1 in one contraction."""
        ov = self.ov
        nprof, n = u.shape[0], u.shape[1] * u.shape[2]
        lin = self.lin(nprof, n, y.shape[1], u.device) if lin is None else lin
        self.prepare(k_blocks, u, se, y, fx, lin, None, stream)
        f64 = dict(dtype=torch.float64, device=u.device)
        out = dict(x_new=torch.empty_like(u), status=torch.empty(nprof, dtype=torch.uint8, device=u.device),
                   chi2=torch.empty(nprof, **f64), dfs=torch.empty(nprof, **f64))
        if post_var and ov.basis is None:
            out["post_var"] = torch.empty_like(u)
        if post_cov or (post_var and ov.basis is not None):
            out["post_cov"] = torch.empty((nprof, n, n), **f64)
        self.solve(k_blocks, u, se, None, lin, out, None, stream)
        out["nobs"] = lin["nobs"]
        if post_var and ov.basis is not None:
            var = torch.einsum("kj,pji,ki->pk", ov._b, out["post_cov"], ov._b)
            out["post_var"] = var.reshape((nprof,) + tuple(ov.xa.shape[-2:]))
        out.setdefault("post_var", None)
        if not post_cov:
            out.pop("post_cov", None)
        return out


class OneDVar:
    def __init__(self, model, frq, elev, sa, se, variables: Optional[JacVariables] = None, blocks=("t", "h"), xa=None,
                 instrument=None, ray_tracing=False, basis: Optional[StateBasis] = None, form="m"):
        blocks = tuple(blocks)
        if form not in ("m", "n"):
            raise ValueError(f"form must be 'm' (an m x m system per profile) or 'n' (an n x n one), got {form!r}")
        self.form = form
        # refracted spherical ray paths: the forward operator and its exact K rows come from mwrt_tb_jacobian_batch_ray_device
        self.ray_tracing = bool(ray_tracing)
        if blocks[:2] != ("t", "h") or blocks[2:] not in ((), ("liq",), ("ice",), ("liq", "ice")):
            raise ValueError(f"blocks must be ('t', 'h') followed by 'liq' and / or 'ice' in that order, got {blocks}")
        self.model, self.blocks = model, blocks
        self.frq = np.ascontiguousarray(frq, dtype=np.float64).ravel()
        self.elev = np.ascontiguousarray(elev, dtype=np.float64).ravel()
        self.variables = variables if variables is not None else JacVariables.of()
        if xa is None:
            raise ValueError("xa (the prior state) is required")
        if sa is None and basis is None:
            raise ValueError("sa (the prior covariance) is required without a basis")
        self.m = self.frq.size * self.elev.size
        # with an instrument (instrument.Instrument) the forward operator runs on its quadrature grid and every TB and K row is
        # reduced to channels before the update sees it: se, y and all diagnostics are in channel space, m = instrument.m_out
        self.instrument = instrument
        if instrument is not None:
            if not (np.array_equal(self.frq, instrument.frq) and np.array_equal(self.elev, instrument.elev)):
                raise ValueError("frq and elev must equal the instrument's channel centres and elevations "
                                 f"(instrument.frq = {instrument.frq.tolist()}, instrument.elev = {instrument.elev.tolist()})")
            self.m = instrument.m_out
        nblk = len(blocks)
        # the tensor contract (module docstring): xa names the device, everything else is checked against it
        self.xa = _checked("xa", xa, (nblk, "nlev"), ("nprof", nblk, "nlev"))
        self.device = self.xa.device
        n = nblk * self.xa.shape[-1]
        self.sa = None if sa is None else _checked("sa", sa, (n, n), device=self.device)
        self.se = _checked("se", se, (self.m,), (self.m, self.m), device=self.device)
        # what the update works in: the state itself, or with a basis the coefficients c ([nprof][1][r] inside this class)
        # with the prior c_a and sa_c.  The coefficients are never clamped: humidity and cloud >= 0 is applied to the
        # physical state clamp(xa + B c) the forward model sees, not to c.
        self.basis = basis
        if basis is None:
            self._prior_mean, self._prior_cov = self.xa, self.sa
            self._sigma = torch.sqrt(torch.diagonal(self.sa)).reshape(nblk, -1)
        else:
            if basis.n != n:
                raise ValueError(f"basis: expected b [{n}][r] for xa {tuple(self.xa.shape)}, got {tuple(basis.b.shape)}")
            if basis.c_a.dim() == 2 and self.xa.dim() == 3 and basis.c_a.shape[0] != self.xa.shape[0]:
                raise ValueError(f"basis.c_a: expected [{basis.r}] or [{self.xa.shape[0]}][{basis.r}], got {tuple(basis.c_a.shape)}")
            dev = self.xa.device
            self._b = basis.b.to(dev)
            self._prior_mean = basis.c_a.to(dev).reshape((-1, 1, basis.r) if basis.c_a.dim() == 2 else (1, basis.r)).contiguous()
            self._prior_cov = basis.sa_c.to(dev).contiguous()
            self._sigma = torch.sqrt(torch.diagonal(self._prior_cov)).reshape(1, -1)
        self._sa_inv = None
        self._form = _NForm(self) if form == "n" else _MForm(self)
        if form == "n":
            # the n-form entries (include/mwrt.h mwrt_oe_nform_*_device): an n x n system per profile, any m, variances only
            size = n if basis is None else basis.r
            if size > _native.OE_NFORM_MAX_N:
                what = f"{nblk} blocks of {self.xa.shape[-1]} levels" if basis is None else f"a basis of r = {basis.r}"
                raise ValueError(f"form='n' takes a state of at most {_native.OE_NFORM_MAX_N} elements, got {size} ({what}): "
                                 "use a reduced basis (basis=StateBasis(...)), a coarser grid, or form='m'")
            if self.se.dim() != 1:
                raise ValueError(f"form='n' takes se [{self.m}] variances in the constructor, got {tuple(self.se.shape)}: pass "
                                 f"the variances here and a per-profile full covariance [nprof][{self.m}][{self.m}] as se= of "
                                 "the call (it is pre-whitened), or use form='m'")

    @property
    def sa_inv(self):
        """Sa^-1 for the cost's prior term: float64, symmetrised, formed on first use (``retrieve_lm`` alone needs it)."""
        if self._sa_inv is None:
            inv = torch.linalg.inv(self._prior_cov.to(torch.float64))
            self._sa_inv = (0.5 * (inv + inv.T)).contiguous()
        return self._sa_inv

    # -- the tensor contract (module docstring) -----------------------------------------------------------------------
    def _inputs(self, z, p, x=None, y=None, x0=None, se=None, physical=False):
        """The tensor arguments of a public method, each checked once (``_checked``: a float64 tensor of the stated shape on
        the device of xa) and contiguous from here on -> ``(z, p, x, y, x0, se)``, None where None was given.  ``x`` and
        ``x0`` are the update's state: ``[nprof][nblk][nlev]``, or with a basis (and not ``physical``) the coefficients
        ``[nprof][r]`` (``[nprof][1][r]`` is taken too).  ``y`` comes back as ``[nprof][m]``.  nprof is that of ``x``, else
        of ``y``; a per-profile xa or c_a of another nprof is refused."""
        nblk, nlev = self.xa.shape[-2:]
        dev, nprof = self.device, "nprof"
        coeff = self.basis is not None and not physical
        state = lambda n: ((n, self.basis.r), (n, 1, self.basis.r)) if coeff else ((n, nblk, nlev),)   # noqa: E731
        if x is not None:
            x = _checked("x", x, *state(nprof), device=dev)
            nprof = x.shape[0]
        if y is not None:
            y = _checked("y", y, (nprof, self.elev.size, self.frq.size), (nprof, self.m), device=dev)
            nprof = y.shape[0]
            y = y.reshape(nprof, self.m)
        if x0 is not None:
            x0 = _checked("x0", x0, *state(nprof), device=dev)
        z = _checked("z", z, (nprof, nlev), device=dev)
        p = _checked("p", p, (nprof, nlev), device=dev)
        self._batch(nprof)
        return z, p, x, y, x0, self._per_profile_se(se, nprof)

    def _batch(self, nprof):
        """A per-profile prior belongs to one batch size: xa ``[nprof][nblk][nlev]`` and c_a ``[nprof][r]`` must have this one."""
        if self.xa.dim() == 3 and self.xa.shape[0] != nprof:
            raise ValueError(f"xa: expected [nblk][nlev] or [{nprof}][nblk][nlev] for this batch, got {tuple(self.xa.shape)}")
        if self.basis is not None and self._prior_mean.dim() == 3 and self._prior_mean.shape[0] != nprof:
            raise ValueError(f"basis.c_a: expected [{self.basis.r}] or [{nprof}][{self.basis.r}] for this batch, got "
                             f"{tuple(self.basis.c_a.shape)}")

    # -- the state in the operator's inputs -----------------------------------------------------------------------------
    def physical(self, z, p, x):
        """(z, t, rh, denliq, denice) the forward operator takes for the state ``x`` (cloud arrays None when not a block)."""
        z, p, x = self._inputs(z, p, x=x, physical=True)[:3]
        return self._physical(z, p, x)

    def _physical(self, z, p, x):
        v = self.variables
        t = x[:, 0].contiguous()
        h = x[:, 1]
        es = goff_gratch_es(t)[0]
        e = h if v.humidity == 0 else h * es if v.humidity == 1 else h * p / 1e6
        rh = (e / es).contiguous()
        cloud = {}
        for b in ("liq", "ice"):
            if b in self.blocks:
                q = x[:, self.blocks.index(b)]
                cloud[b] = (q * 1000.0 * (100.0 * p / (287.06 * t)) if v.cloud == 1 else q).contiguous()
        if v.heights == 1:
            tv = t * (1.0 + 0.608 * (0.622 * e / (p - 0.378 * e)))
            dz = (287.04 / 9.80665) * 0.5 * (tv[:, 1:] + tv[:, :-1]) * torch.log(p[:, :-1] / p[:, 1:]) / 1000.0
            z = torch.cat([z[:, :1], z[:, :1] + torch.cumsum(dz, dim=1)], dim=1).contiguous()
        return z, t, rh, cloud.get("liq"), cloud.get("ice")

    def clamp(self, x):
        """Humidity and cloud are kept >= 0 (the linear update knows no such bound)."""
        return self._clamp(_checked("x", x, ("nprof", len(self.blocks), self.xa.shape[-1]), device=self.device))

    def _clamp(self, x):
        x = x.clone()
        for i, b in enumerate(self.blocks):
            if b != "t":
                x[:, i].clamp_(min=0.0)
        return x

    # -- the reduced basis -------------------------------------------------------------------------------------------
    def expand(self, c):
        """xa + B c ``[nprof][nblk][nlev]`` for the coefficients ``c [nprof][r]`` (``mwrt_basis_expand_device``), unclamped."""
        if self.basis is None:
            raise ValueError("expand needs a basis")
        c = _checked("c", c, ("nprof", self.basis.r), ("nprof", 1, self.basis.r), device=self.device)
        self._batch(c.shape[0])
        return self._expand(c)

    def _expand(self, c):
        return _native_basis_expand(self.basis, c.reshape(c.shape[0], self.basis.r), self.xa, self._stream(c))

    def _state(self, u):
        """The physical state the forward model sees for the update's state ``u``: u itself, or clamp(xa + B c)."""
        return u if self.basis is None else self._clamp(self._expand(u))

    def _bound(self, u):
        """The update's state after a move: clamped as ``clamp`` says, except coefficients, which have no bound."""
        return self._clamp(u) if self.basis is None else u

    def _start(self, x0, nprof):
        """The first state of an iteration ([nprof][nblk][nlev], or [nprof][1][r] with a basis): ``x0`` or the prior."""
        prior = self._prior_mean
        if x0 is not None:
            return x0.clone() if self.basis is None else x0.reshape(nprof, 1, self.basis.r).clone()
        return (prior.expand(nprof, -1, -1) if prior.dim() == 2 else prior).clone()

    # -- a per-profile Se ---------------------------------------------------------------------------------------------
    def _per_profile_se(self, se, nprof):
        """``se=`` of a call, checked: None (the constructor's shared se) or float64 [nprof][m] / [nprof][m][m]."""
        if se is None:
            return None
        return _checked("se", se, (nprof, self.m), (nprof, self.m, self.m), device=self.device)

    def _whiten(self, se_p, k_blocks, y, fx, stream):
        """What the update entries are given: ``(k_blocks, y, fx, se, None)`` as they are without a per-profile Se; with one
        ``(L^-1 K, L^-1 y, L^-1 F, ones(m), w)`` from one ``_native_obs_whiten`` call, w holding l, keep and status."""
        if se_p is None:
            return k_blocks, y, fx, self.se, None
        w = _native_obs_whiten(k_blocks, se_p, y, fx, stream)
        return w["k"], w["y"], w["fx"], torch.ones(self.m, dtype=torch.float64, device=y.device), w

    @staticmethod
    def _fail_whitened(w, out):
        """A profile whose Se_p is not positive definite (whiten status 2) reaches the update with every row dropped, which
        the update calls status 3 and answers with the prior: make it status 2 with NaN in every floating-point field."""
        if w is None:
            return out
        bad = w["status"] == 2
        for key, v in out.items():
            if v is None or key in ("fx", "valid", "keep"):
                continue
            mask = bad.reshape((-1,) + (1,) * (v.dim() - 1))
            if key == "status":
                out[key] = torch.where(bad, torch.full_like(v, 2), v)
            elif v.is_floating_point():
                out[key] = v.masked_fill(mask, float("nan"))
            else:
                out[key] = v.masked_fill(mask, 0)
        return out

    def representation_error(self, z, p, x):
        """K S_res K^T ``[nprof][m][m]`` at the physical state ``x [nprof][nblk][nlev]``: the observation-error covariance
        of what the basis leaves out of the prior (``basis.sa_res``, e.g. of ``StateBasis.from_covariance``), from the
        unprojected K rows at ``x`` -- the instrument's channel rows when there is one.  One K-matrix call and two batched
        products in torch; add it to the noise covariance and pass the sum as ``se=``."""
        if self.basis is None or self.basis.sa_res is None:
            raise ValueError("representation_error needs a basis with sa_res (StateBasis.from_covariance sets it)")
        z, p, x = self._inputs(z, p, x=x, physical=True)[:3]
        _, _, k_blocks = self._observe(z, p, x, project=False)
        nprof = x.shape[0]
        k = torch.cat([b.reshape(nprof, self.m, -1) for b in k_blocks], dim=2)
        return k @ self.basis.sa_res.to(k.device) @ k.transpose(1, 2)

    def _post_var_levels(self, k_blocks, u, y, fx, stream, se):
        """diag(B S^_c B^T) ``[nprof][nblk][nlev]``: the posterior variance of the physical state from the posterior covariance
        of the coefficients (``mwrt_oe_gain_device`` + ``mwrt_oe_product_device``, [r][r] per profile) and one contraction."""
        g = _native_oe_gain(k_blocks, u, self._prior_mean, self._prior_cov, se, y, fx, stream)
        s_c = _native_oe_product("post_cov", g["gain"], g["keep"], k_blocks, g["ksa"], self._prior_cov, (0, 0), stream)
        s_c = s_c.masked_fill(((g["status"] == 0) | (g["status"] == 2))[:, None, None], float("nan"))
        var = torch.einsum("kj,pji,ki->pk", self._b, s_c, self._b)
        return var.reshape((u.shape[0],) + tuple(self.xa.shape[-2:]))

    # -- one Gauss-Newton step ---------------------------------------------------------------------------------------
    def _observe(self, z, p, x, want_rows=True, project=True):
        """One K-matrix call at ``x`` -> (tb [nprof][nang][nf], valid, K blocks in the state's order or None), in what the
        update sees: the operator's own outputs, or with an instrument the channel quantities -- the call then runs on the
        instrument's quadrature grid and ``_native_obs_apply`` reduces the TBs and, when wanted, every block's rows.  With a
        basis the rows are then contracted with it (``_native_basis_project``, behind the channel reduction, which shrinks
        the rows first): the one block K B.  ``x`` is the physical state.  The one place of this class that runs the forward
        operator."""
        zz, t, rh, dl, di = self._physical(z, p, x)
        inst = self.instrument
        frq, elev = (self.frq, self.elev) if inst is None else (inst.frq_q, inst.elev_q)
        stream = self._stream(x)
        k_matrix = _native_k_matrix_ray if self.ray_tracing else _native_k_matrix
        tb, valid, rows = k_matrix(self.model, zz.contiguous(), p.contiguous(), t, rh, dl, di, frq, elev, self.variables,
                                   self.blocks, stream)
        k_blocks = [rows[b] for b in self.blocks] if want_rows else None
        if inst is not None:
            tb, k_blocks = _native_obs_apply(inst, tb, k_blocks, stream)
        if self.basis is not None and k_blocks is not None and project:
            k_blocks = [_native_basis_project(self.basis, k_blocks, stream)]
        return tb, valid, k_blocks

    def forward(self, z, p, x):
        """The forward model at the state ``x``: ``(tb [nprof][nang][nf], valid [nprof])`` on torch's current stream (the
        K-matrix call's TBs; its rows are discarded).  With an instrument: the channel TBs.  ``x`` is the physical state
        also with a basis (``expand`` gives it for coefficients)."""
        z, p, x = self._inputs(z, p, x=x, physical=True)[:3]
        tb, valid, _ = self._observe(z, p, x, want_rows=False)
        return tb, valid

    @staticmethod
    def _stream(x):
        return torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else None

    def step(self, z, p, x, y, post_var=True, se=None, post_cov=False):
        """One K-matrix call at ``x`` plus one update, both queued on torch's current stream -- the stream the change of
        variables and the allocations of this method run on too (use ``torch.cuda.stream(...)`` around the call for another).
        Returns ``(x_new, diagnostics)``: diagnostics holds ``status``, ``chi2``, ``dfs``, ``nobs``, ``post_var`` (None with
        ``post_var=False``), ``fx`` (the forward model at x, [nprof][m]) and ``valid`` (the K-matrix call's flags).
        ``x_new`` is the raw update: ``retrieve`` clamps it.

        With a basis ``x`` holds the coefficients ``c [nprof][r]`` and so does ``x_new``: the K-matrix call runs at
        clamp(xa + B c) -- c itself is never clamped -- and ``chi2``, ``dfs`` are those of the step in c.  ``post_var`` is
        the level-space diag(B S^_c B^T) ``[nprof][nblk][nlev]``, which costs a gain and a product call more.

        ``se=`` gives every profile its own observation-error covariance, ``[nprof][m]`` or ``[nprof][m][m]`` on the state's
        device, in place of the constructor's: K, y and F are whitened with its factor (behind the instrument and the basis)
        and the update runs with Se = 1.  ``fx`` stays the physical F(x); ``whiten_status`` is added (uint8: 1 ok, 2 Se_p not
        positive definite -- then ``status`` is 2 and x_new and the diagnostics are NaN --, 3 no row kept).

        With ``form="n"`` the update is ``mwrt_oe_nform_prepare_device`` + ``mwrt_oe_nform_solve_device``:
        any m, the same diagnostics; with a basis ``post_var`` comes from the solve's C^-1 in one contraction, with no gain
        or product call.  ``se=`` as ``[nprof][m]`` goes straight in (nothing is whitened, no ``whiten_status``), as
        ``[nprof][m][m]`` through the pre-whitening (m <= 140).  ``post_cov=True`` (form="n" only) adds ``post_cov``
        ``[nprof][n][n]``, the posterior covariance C^-1 in the update's state space (coefficients with a basis)."""
        if post_cov and self.form != "n":
            raise ValueError("step(post_cov=True) needs form='n'; with form='m' characterise(post_cov=True) forms it")
        z, p, x, y, _, se = self._inputs(z, p, x=x, y=y, se=se)
        return self._step(z, p, x, y, post_var, se, post_cov)

    def _step(self, z, p, x, y, post_var=True, se=None, post_cov=False):
        """``step`` on arguments ``_inputs`` has checked, what ``retrieve`` iterates: K-matrix call -> instrument -> basis ->
        the call's se -> the form's update."""
        stream = self._stream(x)
        nprof = x.shape[0]
        se_p = self._per_profile_se(se, nprof)
        u = x.contiguous() if self.basis is None else x.reshape(nprof, 1, self.basis.r).contiguous()
        tb, valid, k_blocks = self._observe(z, p, self._state(u))
        fx = tb.reshape(nprof, self.m)
        k_w, y_w, fx_w, se_w, w = self._form.se(se_p, k_blocks, y.reshape(nprof, self.m).contiguous(), fx, stream)
        out = self._fail_whitened(w, self._form.update(k_w, u, se_w, y_w, fx_w, stream, post_var, post_cov))
        out["fx"], out["valid"] = fx, valid
        if w is not None:
            out["whiten_status"] = w["status"]
        return out.pop("x_new").reshape(x.shape), out

    def retrieve(self, z, p, y, x0=None, max_iter=10, tol=0.05, se=None) -> Retrieval:
        """Iterates ``step`` from ``x0`` (default: the prior).  After every step humidity and cloud are clamped to >= 0.  A
        profile is frozen -- its state and diagnostics no longer change -- once max |x_new - x| / sqrt(diag Sa) < ``tol``
        over its whole state, or when its step fails (status 0 or 2: the state before that step is kept).  Only the scalar
        "is any profile still moving" leaves the device, once per iteration.  Every step asks for ``post_var`` (a profile may
        freeze at any step), which about doubles the update's device time.

        With a basis the iteration runs in the coefficients (``x0``: ``[nprof][r]``, default ``c_a``), which are not clamped;
        convergence is max |c_new - c| / sqrt(diag sa_c) < ``tol``.  The steps then skip ``post_var``: the level-space
        diagonal is formed once, at the final states (one K-matrix call, a gain and a product call), so it is the posterior
        variance at ``Retrieval.x``, not at the state before the last step as ``chi2`` and ``dfs`` are.  With ``form="n"`` there
        is no gain or product call: the diagonal comes from one more full ``step`` at the final states (a K-matrix call, the
        projection, prepare and a solve that returns C^-1), whose x_new is discarded.

        ``se=``: a per-profile observation-error covariance as in ``step``; every step whitens its own linearisation.  A
        profile whose Se_p is not positive definite is frozen as failed at its first step: status 2, NaN diagnostics."""
        z, p, _, y, x0, se_p = self._inputs(z, p, y=y, x0=x0, se=se)
        nprof = y.shape[0]
        x = self._start(x0, nprof)
        dev = x.device
        keys = ("chi2", "dfs", "post_var", "status", "nobs") if self.basis is None else ("chi2", "dfs", "status", "nobs")
        active = torch.ones(nprof, dtype=torch.bool, device=dev)
        converged = torch.zeros(nprof, dtype=torch.bool, device=dev)
        iters = torch.zeros(nprof, dtype=torch.int32, device=dev)
        keep = None
        for _ in range(int(max_iter)):
            x_new, d = self._step(z, p, x, y, post_var=self.basis is None, se=se_p)
            ok = (d["status"] == 1) | (d["status"] == 3)
            x_new = self._bound(torch.where(ok[:, None, None], x_new, x))
            move = ((x_new - x).abs() / self._sigma).amax(dim=(1, 2))
            upd = active
            iters = iters + upd.to(torch.int32)
            x = torch.where(upd[:, None, None], x_new, x)
            diag = {k: d[k] for k in keys}
            if keep is None:
                keep = diag
            else:
                keep = {k: torch.where(upd.reshape((-1,) + (1,) * (v.dim() - 1)), v, keep[k]) for k, v in diag.items()}
            done = upd & ((move < tol) | ~ok)
            converged = converged | (upd & ok & (move < tol))
            active = active & ~done
            if not bool(active.any()):
                break
        if self.basis is None:
            post_var = keep["post_var"]
        elif self.form == "n":                                           # the level-space diagonal at the final states, too
            post_var = self._step(z, p, x, y, post_var=True, se=se_p)[1]["post_var"]
        else:
            k_blocks, fx = self._linearise(z, p, x)
            k_w, y_w, fx_w, se_w, w = self._whiten(se_p, k_blocks, y.reshape(nprof, self.m).contiguous(), fx, self._stream(x))
            post_var = self._post_var_levels(k_w, x.contiguous(), y_w, fx_w, self._stream(x), se_w)
            post_var = self._fail_whitened(w, dict(post_var=post_var))["post_var"]
        return Retrieval(x=self._state(x), chi2=keep["chi2"], dfs=keep["dfs"], post_var=post_var, status=keep["status"],
                         nobs=keep["nobs"], iterations=iters, converged=converged,
                         **({} if self.basis is None else {"coeff": x.reshape(nprof, -1)}))

    # -- what the step says about itself --------------------------------------------------------------------------------
    @staticmethod
    def _rows(rows, n):
        """``rows=(begin, count)`` of a characterisation as the window the entries take; None is all n rows, (0, 0)."""
        if rows is None:
            return 0, 0
        win = (int(rows[0]), int(rows[1]))
        if win[0] < 0 or win[1] < 1 or win[0] + win[1] > n:
            raise ValueError(f"rows: expected (begin, count) with count >= 1 inside 0 .. {n - 1}, got {rows}")
        return win

    def _linearised(self, z, p, x, y, rows, se):
        """What both characterisations begin with: the checked arguments, the update's state u (``[nprof][1][r]`` with a
        basis), the rows window, one linearisation at u and the call's se on it -> ``(u, win, k_blocks, y, fx, se, w,
        stream)``, the middle five as the form's ``se`` returns them."""
        z, p, x, y, _, se = self._inputs(z, p, x=x, y=y, se=se)
        nprof = x.shape[0]
        u = (x if self.basis is None else x.reshape(nprof, 1, self.basis.r)).contiguous()
        win = self._rows(rows, u.shape[1] * u.shape[2])
        stream = self._stream(u)
        k_blocks, fx = self._linearise(z, p, u)
        seen = self._form.se(self._per_profile_se(se, nprof), k_blocks, y.reshape(nprof, self.m).contiguous(), fx, stream)
        return (u, win, *seen, stream)

    def characterise(self, z, p, x, y, avk=False, post_cov=False, rows=None, se=None) -> Characterisation:
        """The gain matrix, the averaging-kernel diagonal, the degrees of freedom per block and the split of the posterior
        variance into noise and smoothing error of the undamped step at ``x`` (e.g. ``Retrieval.x``): one K-matrix call at
        ``x``, then ``mwrt_oe_gain_device``, then -- with ``avk`` / ``post_cov`` -- one ``mwrt_oe_product_device`` call each for
        the full averaging kernel and posterior covariance, all on torch's current stream with nothing leaving the device.
        ``rows=(begin, count)`` limits both products to those rows of the n x n result (a full one is nprof n^2 doubles).
        Profiles whose status is 0 or 2 hold NaN in every floating-point field, the products included.

        With a basis ``x`` holds the coefficients ``[nprof][r]`` (``Retrieval.coeff``) and everything returned is in
        coefficient space: n = r, one block.

        ``se=``: a per-profile observation-error covariance as in ``step``.  The gain entry and the products run on the
        whitened linearisation; the gain is then un-whitened (``mwrt_obs_whiten_apply_device``, L^-T), so that ``gain`` is
        d x^ / d y of the physical observations as without ``se=``.  Every other field is the same in both frames.

        Not offered with ``form="n"``: the gain matrix is an m-form product."""
        if self.form == "n":
            raise ValueError("characterise is not offered with form='n': use characterise_nform there (or form='m') for the "
                             "gain matrix, the averaging kernel and the error budget, or step(..., post_cov=True) for the "
                             "posterior covariance")
        u, win, k_blocks, y_w, fx, se_w, w, stream = self._linearised(z, p, x, y, rows, se)
        g = self._fail_whitened(w, _native_oe_gain(k_blocks, u, self._prior_mean, self._prior_cov, se_w, y_w, fx, stream))
        failed = ((g["status"] == 0) | (g["status"] == 2))[:, None, None]
        prod = {}
        for name, want in (("avk", avk), ("post_cov", post_cov)):
            if want:
                out = _native_oe_product(name, g["gain"], g["keep"], k_blocks, g["ksa"], self._prior_cov, win, stream)
                prod[name] = out.masked_fill_(failed, float("nan"))
        if w is not None:                                   # after the products, which pair the whitened gain with L^-1 K
            g["gain"] = _native_obs_whiten_apply(w["l"], w["keep"], 1, None, g["gain"], stream)[1]
        return Characterisation(gain=g["gain"], avk_diag=g["avk_diag"], dfs_block=g["dfs_block"], noise_var=g["noise_var"],
                                smooth_var=g["smooth_var"], status=g["status"], nobs=g["nobs"], keep=g["keep"], **prod,
                                **({} if self.basis is None else {"coeff": u.reshape(u.shape[0], -1)}))

    def characterise_nform(self, z, p, x, y, gain=True, avk=False, post_cov=False, rows=None, se=None) -> Characterisation:
        """``characterise`` for ``form="n"``: the same fields for the undamped n-form step at ``x``, for any
        number of observations.  One K-matrix call at ``x``, ``mwrt_oe_nform_prepare_device``, then
        ``mwrt_oe_nform_char_device`` -- the averaging-kernel diagonal, the degrees of freedom per block, the noise and
        smoothing variances and, with ``avk`` / ``post_cov``, the averaging kernel and the posterior covariance -- and, with
        ``gain``, ``mwrt_oe_nform_gain_device``; all on torch's current stream with nothing leaving the device.
        ``gain=False`` skips the one pass over K (the field is None).  ``rows=(begin, count)`` limits ``avk`` and
        ``post_cov`` to those rows of the n x n result; ``post_cov`` is sliced from the full S^ when the gain needs it too.
        Profiles whose status is 0 or 2 hold NaN in every floating-point field.

        With a basis ``x`` holds the coefficients ``[nprof][r]`` and everything returned is in coefficient space: n = r, one
        block, ``coeff`` is set.  ``se=`` as in ``step``: variances ``[nprof][m]`` go straight in; a full ``[nprof][m][m]``
        goes through the pre-whitening (m <= 140) and the gain is un-whitened afterwards, as in ``characterise``."""
        if self.form != "n":
            raise ValueError("characterise_nform needs form='n'; with form='m' characterise gives the same fields")
        u, win, k_blocks, y_w, fx, se_w, w, stream = self._linearised(z, p, x, y, rows, se)
        nprof, nblk, n = u.shape[0], u.shape[1], u.shape[1] * u.shape[2]
        lin = self._form.lin(nprof, n, self.m, u.device)
        self._form.prepare(k_blocks, u, se_w, y_w, fx, lin, None, stream)
        f64 = dict(dtype=torch.float64, device=u.device)
        out = dict(status=torch.empty(nprof, dtype=torch.uint8, device=u.device), avk_diag=torch.empty_like(u),
                   dfs_block=torch.empty((nprof, nblk), **f64), noise_var=torch.empty_like(u), smooth_var=torch.empty_like(u))
        if avk:
            out["avk"] = torch.empty((nprof, win[1] or n, n), **f64)
        if gain or post_cov:
            out["post_cov"] = torch.empty((nprof, n, n), **f64)
        _native_oe_nform_char(self.sa_inv, lin, nblk, out, win, stream)
        out["gain"] = _native_oe_nform_gain(k_blocks, se_w, lin["keep"], out["post_cov"], out["status"], stream) if gain else None
        if post_cov:
            out["post_cov"] = out["post_cov"][:, win[0]:win[0] + (win[1] or n)].contiguous()
        else:
            out.pop("post_cov", None)
        out["nobs"], out["keep"] = lin["nobs"], lin["keep"]
        out = self._fail_whitened(w, out)
        if w is not None and gain:                          # after everything else: the gain back to d x^ / d y
            out["gain"] = _native_obs_whiten_apply(w["l"], w["keep"], 1, None, out["gain"], stream)[1]
        return Characterisation(**out, **({} if self.basis is None else {"coeff": u.reshape(nprof, n)}))

    # -- the damped iteration ------------------------------------------------------------------------------------------
    def _linearise(self, z, p, x):
        """One K-matrix call at ``x`` -> (K blocks in the state's order, F(x) [nprof][m]); fresh tensors every call.  With a
        basis ``x`` holds the coefficients [nprof][1][r] and the one block is K B at clamp(xa + B c)."""
        tb, _, k_blocks = self._observe(z, p, self._state(x))
        return k_blocks, tb.reshape(x.shape[0], self.m)

    def retrieve_lm(self, z, p, y, x0=None, max_iter=20, tol=0.05, gamma0=1.0, up=10.0, down=10.0, gamma_max=1e8,
                    se=None) -> Retrieval:
        """Levenberg-Marquardt iteration from ``x0`` (default: the prior), per profile and wholly on the device and torch's
        current stream.  With J = r^T Se^-1 r + (x - xa)^T Sa^-1 (x - xa), every iteration
          1  linearises the profiles whose state changed: one K-matrix call, ``prepare`` and the cost J at x;
          2  takes the damped trial of every active profile with its own gamma (``solve``), clamps humidity and cloud to >= 0,
             runs the forward model at the trial (into tensors of its own: K(x) stays) and takes J there on the
             linearisation's rows;
          3  accepts where J_trial <= J (x <- trial, gamma <- gamma / ``down``), otherwise keeps x and its linearisation and
             sets gamma <- gamma * ``up``.
        A profile is frozen as converged when an accepted move is below ``tol`` sqrt(diag Sa) everywhere, and as failed when
        gamma exceeds ``gamma_max`` or its linearisation's status is not 1.  One scalar leaves the device per iteration (is
        any profile active; does any state want a new K).  Afterwards one undamped ``mwrt_oe_step_device`` call at the
        final states fills chi2, dfs, post_var, nobs and status -- Rodgers' diagnostics are those of gamma = 0 -- and its
        x_new is discarded.  ``iterations`` counts the trials a profile took.

        With a basis x is the coefficient vector c throughout (``x0``: ``[nprof][r]``, default ``c_a``), J's prior term is
        (c - c_a)^T sa_c^-1 (c - c_a), trials are not clamped and the forward model runs at clamp(xa + B c); ``post_var`` is
        the level-space diag(B S^_c B^T) at the final states.

        ``se=``: a per-profile observation-error covariance as in ``step``.  Every linearisation is whitened (the whole
        batch: a profile whose state did not move gets the same factor bit for bit), F(x_trial) is whitened with the factor
        and the rows of the linearisation it is compared on (``mwrt_obs_whiten_apply_device``, L^-1), and J is that of Se_p.
        A profile whose Se_p is not positive definite is frozen as failed: status 2, NaN diagnostics.

        With ``form="n"`` the same loop runs on ``mwrt_oe_nform_prepare_device`` / ``mwrt_oe_nform_solve_device`` /
        ``mwrt_oe_nform_cost_device`` (any m; one n x n solve per trial), and the final diagnostics come from one undamped
        solve at the final states."""
        z, p, _, y, x0, se = self._inputs(z, p, y=y, x0=x0, se=se)
        form = self._form
        nprof, m = y.shape[0], self.m
        se_p = self._per_profile_se(se, nprof)
        se_w, w, y_w = self.se, None, None
        x = self._start(x0, nprof).contiguous()
        dev, stream = x.device, self._stream(x)
        yv = y.reshape(nprof, m).contiguous()
        f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
        lin = form.lin(nprof, x.shape[1] * x.shape[2], m, dev)
        trial = dict(x_new=torch.zeros_like(x), status=torch.zeros(nprof, **u8))
        cost = torch.full((nprof,), float("inf"), **f64)
        cost_try = torch.full((nprof,), float("inf"), **f64)
        gamma = torch.full((nprof,), float(gamma0), **f64)
        active = torch.ones(nprof, dtype=torch.bool, device=dev)
        stale = torch.ones(nprof, dtype=torch.bool, device=dev)          # the state changed since its linearisation
        converged = torch.zeros(nprof, dtype=torch.bool, device=dev)
        iters = torch.zeros(nprof, dtype=torch.int32, device=dev)
        k_blocks = fx = None
        relin = True
        for _ in range(int(max_iter)):
            if relin:
                k_blocks, fx = self._linearise(z, p, x)
                k_blocks, y_w, fx, se_w, w = form.se(se_p, k_blocks, yv, fx, stream)
                mask = (active & stale).to(torch.uint8)
                form.prepare(k_blocks, x, se_w, y_w, fx, lin, mask, stream)
                form.cost(x, se_w, y_w, fx, lin["keep"], cost, mask, stream)
                stale = torch.zeros_like(stale)
                active = active & (lin["lin_status"] == 1)
            mask = active.to(torch.uint8)
            form.solve(k_blocks, x, se_w, gamma, lin, trial, mask, stream)
            ok = active & (trial["status"] == 1)
            x_try = self._bound(torch.where(ok[:, None, None], trial["x_new"], x)).contiguous()
            fx_try = self._observe(z, p, self._state(x_try), want_rows=False)[0].reshape(nprof, m)
            if w is not None:
                fx_try = _native_obs_whiten_apply(w["l"], w["keep"], 0, fx_try, None, stream)[0]
            form.cost(x_try, se_w, y_w, fx_try, lin["keep"], cost_try, mask, stream)
            accept = ok & (cost_try <= cost)
            move = ((x_try - x).abs() / self._sigma).amax(dim=(1, 2))
            iters = iters + active.to(torch.int32)
            x = torch.where(accept[:, None, None], x_try, x).contiguous()
            cost = torch.where(accept, cost_try, cost)
            gamma = torch.where(accept, gamma / down, torch.where(active, gamma * up, gamma))
            done = accept & (move < tol)
            converged = converged | done
            stale = stale | accept
            active = active & ~done & ~(gamma > gamma_max)
            flag = int((active.any().to(torch.int32) + 2 * stale.any().to(torch.int32)).item())
            relin = bool(flag & 2)
            if not flag & 1:
                break
        if relin:
            k_blocks, fx = self._linearise(z, p, x)
            k_blocks, y_w, fx, se_w, w = form.se(se_p, k_blocks, yv, fx, stream)
        d = self._fail_whitened(w, form.update(k_blocks, x, se_w, y_w, fx, stream, True, lin=lin))
        return Retrieval(x=self._state(x), chi2=d["chi2"], dfs=d["dfs"], post_var=d["post_var"], status=d["status"],
                         nobs=d["nobs"], iterations=iters, converged=converged, cost=cost, gamma=gamma,
                         **({} if self.basis is None else {"coeff": x.reshape(nprof, -1)}))
