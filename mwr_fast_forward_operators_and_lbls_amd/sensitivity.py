"""Spectroscopic-parameter sensitivity: d TB / d b for entries b of a model's tables, and the forward-model part
K_b S_b K_b^T of an observation-error covariance (Rodgers 2000, section 3.2.2).

The Jacobian is the native library's (``mwrt_tb_param_jacobian_batch_device``: exact tangents, HIP); everything here is
naming, scaling and a batched product.

A parameter is named after the ``ModelTables`` entry it differentiates: ``"h2o_cf"`` (a scalar), ``"h2o_w0[0]"`` (line 0 of
a per-line field), ``"o2_w300[*]"`` (a common factor on that field of every line: the derivative with respect to the factor
at 1, i.e. already relative), ``"o2_y0"`` (a bare per-line name: every line of the model, one parameter each)."""
from __future__ import annotations

import re
from typing import List, NamedTuple, Sequence

import numpy as np

from . import _native
from .spectroscopy import get_model


class Param(NamedTuple):
    """One parameter: ``name`` (a key of ``_native.PARAM_FIELDS``), ``field`` (its MWRT_PAR_* id), ``line`` (0 for a scalar,
    -1 = MWRT_PAR_ALL_LINES) and ``value``, the table entry (1.0 for a common factor)."""
    name: str
    field: int
    line: int
    value: float

    @property
    def label(self) -> str:
        if self.field < _native.PAR_FIRST_H2O_LINE_FIELD:
            return self.name
        return f"{self.name}[{'*' if self.line < 0 else self.line}]"


_SPEC = re.compile(r"^\s*([a-z0-9_]+)\s*(?:\[\s*(\*|\d+)\s*\])?\s*$")


def _tables(model):
    return get_model(model) if isinstance(model, str) else model


def parse_params(model, specs: Sequence[str]) -> List[Param]:
    """``["h2o_w0[0]", "o2_w300[*]", "h2o_cf", "o2_y0"]`` -> ``Param`` records for ``model`` (a name or a ``ModelTables``).

    ``[*]`` is MWRT_PAR_ALL_LINES; a bare per-line name expands to every line of the model.  ValueError: an unknown name, an
    index on a scalar, a line outside the model's table, an empty list, or more than MWRT_MAX_PARAMS parameters."""
    m = _tables(model)
    out: List[Param] = []
    for spec in specs:
        hit = _SPEC.match(spec) if isinstance(spec, str) else None
        if hit is None or hit.group(1) not in _native.PARAM_FIELDS:
            raise ValueError(f"unknown spectroscopic parameter {spec!r}: one of {', '.join(_native.PARAM_FIELDS)}, "
                             "a per-line name with [k] or [*]")
        name, idx = hit.group(1), hit.group(2)
        field = _native.PARAM_FIELDS[name]
        if field < _native.PAR_FIRST_H2O_LINE_FIELD:
            if idx is not None:
                raise ValueError(f"{spec!r}: {name} is a scalar, it takes no line index")
            out.append(Param(name, field, 0, float(getattr(m, name))))
            continue
        species, key = name.split("_", 1)
        column = np.asarray((m.h2o if species == "h2o" else m.o2)[key], dtype=np.float64)
        if idx == "*":
            out.append(Param(name, field, _native.PAR_ALL_LINES, 1.0))
        elif idx is None:
            out += [Param(name, field, k, float(column[k])) for k in range(column.size)]
        else:
            k = int(idx)
            if k >= column.size:
                raise ValueError(f"{spec!r}: line {k} outside the {column.size} lines of {m.name}")
            out.append(Param(name, field, k, float(column[k])))
    if not out:
        raise ValueError("no parameter given")
    if len(out) > _native.MAX_PARAMS:
        raise ValueError(f"{len(out)} parameters, more than MWRT_MAX_PARAMS = {_native.MAX_PARAMS} of one call")
    return out


def _records(model, params) -> List[Param]:
    params = list(params)
    return params if params and all(isinstance(q, Param) for q in params) else parse_params(model, params)


def _native_param_jacobian(tables, z, p, t, rh, frq, elev, recs):
    """One ``mwrt_tb_param_jacobian_batch_device`` call on torch's current stream -> (tb, kb, valid) device tensors.

    The single place this module reaches the native library: CPU tests substitute a stand-in here."""
    import torch
    if not z.is_cuda:
        raise ValueError("param_jacobian: the profiles must be CUDA tensors (the operator has no CPU path)")
    nprof, nlev = z.shape
    opts = dict(dtype=torch.float64, device=z.device)
    tb = torch.empty((nprof, elev.size, frq.size), **opts)
    kb = torch.empty((nprof, elev.size, frq.size, len(recs)), **opts)
    valid = torch.empty((nprof,), dtype=torch.uint8, device=z.device)
    ctx = _native.default_context(z.device.index or 0)
    ctx.tb_param_jacobian_device(tables, nprof, nlev, z.data_ptr(), p.data_ptr(), t.data_ptr(), rh.data_ptr(), frq, elev,
                                 [(q.field, q.line) for q in recs], kb.data_ptr(), valid.data_ptr(), d_tb=tb.data_ptr(),
                                 stream=torch.cuda.current_stream(z.device).cuda_stream)
    return tb, kb, valid


def param_jacobian(model, z, p, t, rh, frq, elev, params, relative=False):
    """``(tb [nprof][nang][nf], kb [nprof][nang][nf][npar], valid [nprof])`` on the device of the float64 CUDA tensors
    ``z, p, t, rh [nprof][nlev]``, launched on torch's current stream.  ``params``: ``Param`` records or the strings
    ``parse_params`` takes.  ``kb`` is K per unit of the table entry; ``relative=True`` scales column p by b_p, K per unit
    relative change (``[*]`` columns are relative already and are left as they are)."""
    import torch
    recs = _records(model, params)
    for name, x in (("z", z), ("p", p), ("t", t), ("rh", rh)):
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.dim() == 2 and x.shape == z.shape
                and x.device == z.device):
            raise ValueError(f"{name}: expected a float64 tensor [nprof][nlev] on the device of z")
    z, p, t, rh = (x.contiguous() for x in (z, p, t, rh))
    frq, elev = np.ascontiguousarray(frq, dtype=np.float64).ravel(), np.ascontiguousarray(elev, dtype=np.float64).ravel()
    tb, kb, valid = _native_param_jacobian(_tables(model), z, p, t, rh, frq, elev, recs)
    if relative:
        kb = scale_relative(kb, recs)
    return tb, kb, valid


def scale_relative(kb, params):
    """Column p of ``kb [...][npar]`` times the table entry b_p (1 for a ``[*]`` column): K per unit relative change."""
    import torch
    return kb * torch.tensor([q.value for q in params], dtype=kb.dtype, device=kb.device)


def model_error_covariance(kb, sb, reduce=None):
    """K_b S_b K_b^T: the forward-model part of the observation-error covariance, ``[nprof][m][m]`` per profile with
    m = nang * nf (``kb`` is ``[nprof][nang][nf][npar]`` or ``[nprof][m][npar]``), or its mean over the batch with
    ``reduce="mean"`` -- ``[m][m]``, what ``OneDVar(se=se_noise + ...)`` takes.  ``sb``: ``[npar]`` variances or a
    ``[npar][npar]`` covariance, in the units of ``kb``'s columns (relative variances for a ``relative=True`` Jacobian).
    The result is symmetrised (the two roundings of an off-diagonal pair are averaged)."""
    import torch
    if reduce not in (None, "mean"):
        raise ValueError('reduce: None or "mean"')
    k = kb.reshape(kb.shape[0], -1, kb.shape[-1])
    sb = torch.as_tensor(sb, dtype=k.dtype, device=k.device)
    npar = k.shape[-1]
    if sb.shape == (npar,):
        ks = k * sb
    elif sb.shape == (npar, npar):
        ks = k @ sb
    else:
        raise ValueError(f"sb: expected [{npar}] variances or [{npar}][{npar}], got {tuple(sb.shape)}")
    cov = torch.bmm(ks, k.transpose(1, 2))
    cov = 0.5 * (cov + cov.transpose(1, 2))
    return cov.mean(dim=0) if reduce == "mean" else cov
