"""Observation selection by information content on the device (include/mwrt.h ``mwrt_oe_select_device``, DESIGN.md 4.12;
Rodgers 2000, section 2.5; the sequential channel selection of Rabier et al. 2002): which observations of a scan carry the
information, in which order, and how the degrees of freedom grow along it.

    sel = rank_observations(ov, z, p, x)          # one K-matrix call at x, then one selection call; any OneDVar
    sel.order[:, :49]                             # the 49 most informative observations of every profile, best first
    sel.cum_dfs[:, [13, 48, 97]]                  # degrees of freedom for signal after 14, 49 and 98 picks
    sel.first(98)                                 # [m]: in how many profiles an observation is among the first 98

Per profile the greedy sequence takes, round by round, the unchosen candidate with the largest q_i = k_i^T S k_i / se_i --
the largest entropy reduction log2(1 + q_i) / 2 in the current posterior S -- and assimilates it (S <- S - v v^T / d with
v = S k_j, d = se_j + k_j^T v) before the next round; ties go to the lowest index.  ``select_observations`` is the entry on
tensors: K blocks, variances and a start covariance S0 (Sa, the ``sa_c`` of a basis, or ``post_cov`` of an earlier
selection).  ``rank_observations`` runs it for a ``retrieval.OneDVar`` of either form, with or without ``instrument=``,
``basis=`` and ``ray_tracing=``, at a state ``x``.  Everything is on torch's current stream and nothing leaves the device.

A full observation-error covariance is not taken: whitening mixes the rows, so there would be no single observation left
to rank.  The state is at most 128 elements (S lives in LDS): a larger one needs a reduced basis.  Groups of observations
(a whole elevation, a whole channel) are not ranked as groups.

The tensor contract is that of ``retrieval`` (its module docstring): every tensor argument is a float64 ``torch.Tensor`` of
the stated shape on one device (the masks ``keep`` and ``candidate``: uint8 or bool), made contiguous once at entry; anything
else is a ``ValueError`` naming the argument, and nothing has reached the library by then."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _native
from .retrieval import _checked, _context


def _native_oe_select(k_blocks, se, s0, nsel, keep, candidate, sa_inv, out, stream):
    """One ``mwrt_oe_select_device`` call on the K blocks ``[nprof][m][nlev]`` into ``out`` in place: order, q_pick, rank, q,
    count, status, and whichever of dfs_gain, post_cov and post_var it holds a tensor for.  CPU tests substitute the
    reference here."""
    nprof, m, nlev = k_blocks[0].shape
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    _context(k_blocks[0]).oe_select_device(
        nprof, nlev, m, [k.data_ptr() for k in k_blocks], s0.data_ptr(), se.data_ptr(), int(nsel), out["order"].data_ptr(),
        out["q_pick"].data_ptr(), out["rank"].data_ptr(), out["q"].data_ptr(), out["count"].data_ptr(),
        out["status"].data_ptr(), d_sa_inv=ptr(sa_inv), d_keep=ptr(keep), d_candidate=ptr(candidate),
        d_dfs_gain=ptr(out.get("dfs_gain")), d_post_cov=ptr(out.get("post_cov")), d_post_var=ptr(out.get("post_var")),
        se_per_profile=se.dim() == 2, s0_per_profile=s0.dim() == 3, stream=stream)


@dataclass
class Selection:
    """What a selection returns, all on the device.  ``order [nprof][nsel]`` int32: the observation picked in each round, -1
    where fewer than nsel were picked; ``q`` its SNR^2 at that moment (0 there); ``info_bits`` = log2(1 + q) / 2 and
    ``cum_info`` its running sum; ``dfs_gain`` the degrees of freedom for signal each pick adds and ``cum_dfs`` their running
    sum (None without ``sa_inv``); ``rank [nprof][m]`` int32 the round an observation was picked in, -1 if not;
    ``q_left [nprof][m]`` what each unchosen candidate would still add (its q for a chosen one, exact 0 for a row that was no
    candidate); ``count [nprof]`` the picks made; ``status [nprof]`` uint8 (1 ok; 0 S0 or Sa^-1 not finite; 2 a candidate's
    variance <= 0 or a d not > 0; 3 no candidate): with 0 and 2 every floating-point field is NaN.  ``post_cov
    [nprof][n][n]`` and ``post_var [nprof][nblk][nlev]``: the posterior after the picks (None unless asked for).  ``nf`` is
    the number of frequencies of the scan behind ``elev_index`` / ``freq_index`` (None for a selection on bare tensors)."""
    order: torch.Tensor
    q: torch.Tensor
    info_bits: torch.Tensor
    cum_info: torch.Tensor
    dfs_gain: Optional[torch.Tensor]
    cum_dfs: Optional[torch.Tensor]
    rank: torch.Tensor
    q_left: torch.Tensor
    count: torch.Tensor
    status: torch.Tensor
    post_cov: Optional[torch.Tensor] = None
    post_var: Optional[torch.Tensor] = None
    nf: Optional[int] = None

    def _split(self, index):
        if self.nf is None:
            raise ValueError("elev_index and freq_index need the scan's layout: rank_observations sets it, or pass nf=")
        picked = self.order >= 0
        return torch.where(picked, index(self.order.clamp(min=0), self.nf), self.order)

    @property
    def elev_index(self):
        """``order // nf``: the elevation of every pick, -1 kept."""
        return self._split(lambda o, nf: torch.div(o, nf, rounding_mode="floor"))

    @property
    def freq_index(self):
        """``order % nf``: the frequency (channel) of every pick, -1 kept."""
        return self._split(lambda o, nf: o % nf)

    def first(self, k):
        """``[m]`` int64: in how many profiles of the batch each observation is among the first ``k`` picks."""
        m = self.rank.shape[1]
        head = self.order[:, :int(k)].reshape(-1).to(torch.int64)
        return torch.bincount(head[head >= 0], minlength=m)


def _mask(name, v, shape, device):
    if v is None:
        return None
    if not torch.is_tensor(v) or v.dtype not in (torch.uint8, torch.bool) or tuple(v.shape) != shape:
        got = type(v).__name__ if not torch.is_tensor(v) else f"{v.dtype} {tuple(v.shape)}"
        raise ValueError(f"{name}: expected a uint8 or bool tensor {''.join(f'[{d}]' for d in shape)}, got {got}")
    if v.device != device:
        raise ValueError(f"{name}: expected a tensor on {device} (the device of the K blocks), got one on {v.device}")
    return v.to(torch.uint8).contiguous()


def select_observations(k_blocks, se, s0, nsel, keep=None, candidate=None, sa_inv=None, post_cov=False, post_var=False,
                        nf=None) -> Selection:
    """The greedy selection on tensors, on torch's current stream.  ``k_blocks``: 1 .. 4 tensors ``[nprof][m][nlev]`` (the
    columns of K, n = nblk nlev <= 128); ``se`` variances ``[m]`` or ``[nprof][m]``; ``s0`` the start covariance ``[n][n]`` or
    ``[nprof][n][n]``, symmetric; ``nsel`` in 1 .. m.  ``keep [nprof][m]`` and ``candidate [m]`` (uint8 or bool) switch rows
    off; a row with a NaN in K or se is no candidate either.  With ``sa_inv [n][n]`` the degrees of freedom each pick adds
    are returned too.  ``post_cov`` / ``post_var``: return the posterior after the picks."""
    k_blocks = list(k_blocks) if isinstance(k_blocks, (list, tuple)) else [k_blocks]
    if not 1 <= len(k_blocks) <= 4:
        raise ValueError(f"k_blocks: expected 1 .. 4 tensors [nprof][m][nlev], got {len(k_blocks)}")
    first = _checked("k_blocks[0]", k_blocks[0], ("nprof", "m", "nlev"))
    nprof, m, nlev = first.shape
    dev = first.device
    k_blocks = [first] + [_checked(f"k_blocks[{b}]", k, (nprof, m, nlev), device=dev) for b, k in enumerate(k_blocks) if b]
    n = len(k_blocks) * nlev
    if n > _native.OE_NFORM_MAX_N:
        raise ValueError(f"the selection takes a state of at most {_native.OE_NFORM_MAX_N} elements, got {n} ({len(k_blocks)} "
                         f"blocks of {nlev}): use a reduced basis (basis=StateBasis(...)) or a coarser grid")
    se = _checked("se", se, (m,), (nprof, m), device=dev)
    s0 = _checked("s0", s0, (n, n), (nprof, n, n), device=dev)
    sa_inv = None if sa_inv is None else _checked("sa_inv", sa_inv, (n, n), device=dev)
    keep = _mask("keep", keep, (nprof, m), dev)
    candidate = _mask("candidate", candidate, (m,), dev)
    if isinstance(nsel, bool) or not isinstance(nsel, int) or not 1 <= nsel <= m:
        raise ValueError(f"nsel: expected an int in 1 .. {m} (the observations of a profile), got {nsel!r}")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    out = dict(order=torch.empty((nprof, nsel), **i32), q_pick=torch.empty((nprof, nsel), **f64),
               rank=torch.empty((nprof, m), **i32), q=torch.empty((nprof, m), **f64), count=torch.empty(nprof, **i32),
               status=torch.empty(nprof, dtype=torch.uint8, device=dev))
    if sa_inv is not None:
        out["dfs_gain"] = torch.empty((nprof, nsel), **f64)
    if post_cov:
        out["post_cov"] = torch.empty((nprof, n, n), **f64)
    if post_var:
        out["post_var"] = torch.empty((nprof, len(k_blocks), nlev), **f64)
    stream = torch.cuda.current_stream(dev).cuda_stream if first.is_cuda else None
    if nprof:
        _native_oe_select(k_blocks, se, s0, nsel, keep, candidate, sa_inv, out, stream)
    bits = 0.5 * torch.log2(1.0 + out["q_pick"])
    gain = out.get("dfs_gain")
    return Selection(order=out["order"], q=out["q_pick"], info_bits=bits, cum_info=torch.cumsum(bits, dim=1), dfs_gain=gain,
                     cum_dfs=None if gain is None else torch.cumsum(gain, dim=1), rank=out["rank"], q_left=out["q"],
                     count=out["count"], status=out["status"], post_cov=out.get("post_cov"), post_var=out.get("post_var"),
                     nf=nf)


def rank_observations(ov, z, p, x, nsel=None, candidate=None, se=None, post_cov=False, post_var=True) -> Selection:
    """The observations of the scan of ``ov`` (a ``retrieval.OneDVar`` of either form) ranked by information content at the
    state ``x``: one K-matrix call at ``x`` (``ov._observe``: with the instrument's reduction and the basis projection when
    there are any), then one selection from S0 = the prior covariance the update works in (``sa``, or ``sa_c`` of the
    basis) with Sa^-1 = ``ov.sa_inv``.  ``x`` is what ``characterise`` takes: the state ``[nprof][nblk][nlev]``, or with a
    basis the coefficients ``[nprof][r]``.  The variances are the constructor's ``se [m]``, or ``se=`` as ``[nprof][m]``.
    ``nsel=None`` ranks all m.  ``candidate [m]`` (uint8 or bool) limits the choice, e.g. to the elevations a scan can
    reach.  ``post_var`` is in the space the update works in (coefficients with a basis)."""
    z, p, x, _, _, se_p = ov._inputs(z, p, x=x, se=se)
    nprof, m = x.shape[0], ov.m
    variances = ov.se if se_p is None else se_p
    if variances.dim() != (1 if se_p is None else 2):
        where = "the constructor's se" if se_p is None else "se="
        raise ValueError(f"{where}: a full observation-error covariance {tuple(variances.shape)} cannot be ranked row by row: "
                         f"whitening mixes the rows, so there would be no single observation left to rank; pass variances "
                         f"[{m}] (or se= as [nprof][{m}])")
    u = (x if ov.basis is None else x.reshape(nprof, 1, ov.basis.r)).contiguous()
    n = u.shape[1] * u.shape[2]
    if n > _native.OE_NFORM_MAX_N:
        raise ValueError(f"the selection takes a state of at most {_native.OE_NFORM_MAX_N} elements, got {n} "
                         f"({u.shape[1]} blocks of {u.shape[2]} levels): use a reduced basis (basis=StateBasis(...)) or a "
                         "coarser grid")
    _, _, k_blocks = ov._observe(z, p, ov._state(u))
    k_blocks = [k.reshape(nprof, m, k.shape[-1]) for k in k_blocks]
    return select_observations(k_blocks, variances, ov._prior_cov, m if nsel is None else nsel, candidate=candidate,
                               sa_inv=ov.sa_inv, post_cov=post_cov, post_var=post_var, nf=int(ov.frq.size))
