"""The instrument between the monochromatic pencil-beam forward operator and what a radiometer reports:
every channel integrates over its bandpass and its antenna beam.  On a quadrature grid both are one fixed sparse linear map

    y[a, c]    = sum_k sum_j  wb[c][k] wf[c][j]  TB(elev[a] + db[c][k], frq[c] + df[c][j])
    K[a, c][l] = the same sum over the K-matrix rows, for every state block

which ``mwrt_obs_apply_device`` applies on the device to the outputs of one K-matrix call on the grid.

    inst = Instrument(frq, elev, beam=3.5, band=0.23)              # Gaussian beam of 3.5 deg FWHM, 230-MHz boxcar bands
    tb, valid, rows = ...K-matrix call on inst.frq_q, inst.elev_q...
    tb_ch, k_ch = inst.apply(tb, [rows["t"], rows["h"]])           # [nprof][nang][nch], [nprof][nang][nch][nlev] each
    ov = OneDVar(model, frq, elev, sa, se, ..., instrument=inst)   # the retrieval in channel space

The averaging is in brightness temperature, not radiance; a beam node at or below the horizon is refused (ground pickup is
not modelled)."""
from __future__ import annotations

import math

import numpy as np

from . import _native

_FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))       # 2.3548...


def _normalised(w):
    w = np.asarray(w, dtype=np.float64)
    return w / math.fsum(w)


def gaussian_beam(fwhm_deg, n=3):
    """Gauss-Hermite rule for a Gaussian antenna pattern of full width at half maximum ``fwhm_deg``: ``(offsets [deg],
    weights)`` with the weights summing to 1.  Exact for polynomials in the offset up to degree 2n - 1 (mean 0 and, from
    n = 2 on, variance (fwhm / 2.3548)^2).  ``n = 1`` or a zero width is the pencil beam."""
    n, fwhm = int(n), float(fwhm_deg)
    if n < 1 or not (fwhm >= 0.0 and math.isfinite(fwhm)):
        raise ValueError(f"gaussian_beam: need n >= 1 and a finite fwhm >= 0, got n = {n}, fwhm = {fwhm_deg}")
    if n == 1 or fwhm == 0.0:
        return np.zeros(1), np.ones(1)
    x, w = np.polynomial.hermite.hermgauss(n)                 # int exp(-x^2) f(x) dx
    return math.sqrt(2.0) * (fwhm / _FWHM_PER_SIGMA) * x, _normalised(w)


def boxcar_band(bandwidth_ghz, n=3):
    """Gauss-Legendre rule for a rectangular bandpass ``bandwidth_ghz`` wide: ``(offsets [GHz], weights)`` with the weights
    summing to 1, exact for polynomials in the offset up to degree 2n - 1.  ``n = 1`` or a zero width is monochromatic."""
    n, bw = int(n), float(bandwidth_ghz)
    if n < 1 or not (bw >= 0.0 and math.isfinite(bw)):
        raise ValueError(f"boxcar_band: need n >= 1 and a finite bandwidth >= 0, got n = {n}, bandwidth = {bandwidth_ghz}")
    if n == 1 or bw == 0.0:
        return np.zeros(1), np.ones(1)
    x, w = np.polynomial.legendre.leggauss(n)                 # int_-1^1 f(x) dx
    return 0.5 * bw * x, _normalised(w)


def _is_pair(spec):
    """An explicit (offsets, weights) pair: two array-likes (not scalars) of one length."""
    if not isinstance(spec, (tuple, list)) or len(spec) != 2:
        return False
    try:
        return np.ndim(spec[0]) == 1 and np.ndim(spec[1]) == 1 and len(spec[0]) == len(spec[1])
    except ValueError:                                        # ragged: a sequence of per-channel entries
        return False


def _per_channel(spec, nch, n, rule, what):
    """``spec`` (None, a width, an (offsets, weights) pair, or a sequence of nch of these) -> per channel
    ``(offsets, weights normalised to sum 1, width or None)``."""
    def one(s, c):
        if s is None:
            return np.zeros(1), np.ones(1), None
        if _is_pair(s):
            off, w = np.asarray(s[0], dtype=np.float64), np.asarray(s[1], dtype=np.float64)
            if off.size < 1 or not (np.isfinite(off).all() and np.isfinite(w).all()) or not math.fsum(w) > 0.0:
                raise ValueError(f"{what} of channel {c}: offsets and weights must be finite, the weights with a positive sum")
            return off, _normalised(w), None
        if not isinstance(s, (tuple, list)) and np.ndim(s) == 0:
            off, w = rule(s, n)
            return off, w, float(s)
        raise ValueError(f"{what} of channel {c}: expected None, a width or an (offsets, weights) pair, got {s!r}")
    if spec is None or _is_pair(spec) or (not isinstance(spec, (tuple, list)) and np.ndim(spec) == 0):
        return [one(spec, c) for c in range(nch)]
    if len(spec) != nch:
        raise ValueError(f"{what}: expected one entry per channel ({nch}), got {len(spec)}")
    return [one(s, c) for c, s in enumerate(spec)]


class Instrument:
    """Antenna beam and channel bandpass of a radiometer as one sparse map from a quadrature grid to its channels.

    ``frq [nch]`` (GHz) and ``elev [nang]`` (deg) are the channel centres and the pointing elevations.  ``beam`` is the
    antenna pattern: None (pencil), a Gaussian full width at half maximum in degrees (``gaussian_beam`` with ``n_beam``
    nodes), or an explicit ``(offsets_deg, weights)`` pair; ``band`` the bandpass: None (monochromatic), a boxcar width in
    GHz (``boxcar_band`` with ``n_band`` nodes), or an explicit ``(offsets_ghz, weights)`` pair, e.g. a measured filter
    curve or the two sidebands of a double-sideband receiver.  Either may also be a sequence with one such entry per
    channel.  Explicit weights are normalised to sum 1.

    The forward operator runs on the tensor grid ``elev_q [nang_q]`` x ``frq_q [nf_q]``: all elevation nodes of all
    channels and all frequency nodes, sorted and deduplicated.  With per-channel beams of different widths the grid is the
    UNION of their elevation nodes, and every frequency is computed at every one of them, so distinct widths cost
    forward-model work in proportion (up to ``MWRT_MAX_ANGLES`` = 64 elevation nodes; more is a ValueError).

    The map is CSR -- ``row_ptr [m_out + 1]``, ``col [nnz]``, ``w [nnz]`` -- from inputs j = aq * nf_q + fq (the layout of a
    ``tb [nang_q][nf_q]``) to outputs o = a * nch + c (angle-major, like ``tb [nang][nch]``); ``m_in = nang_q * nf_q``,
    ``m_out = nang * nch``.  Elevation nodes above 90 deg are passed on as they are (the operator takes elevations in
    (0, 180)); a node at or outside 0 or 180 deg is a ValueError.  A NaN elevation is kept as one node of the grid: the
    operator blanks its rows and the map carries the NaN to that elevation's channels alone.  The same holds along
    refracted ray paths (``OneDVar(..., ray_tracing=True)``): a beam node below the lowest untrapped elevation gives NaN
    rows (and ``valid = 3``), the CSR reduction confines them to the channels that reference that node, and the step drops
    those channels."""

    def __init__(self, frq, elev, beam=None, band=None, n_beam=3, n_band=3):
        self.frq = np.ascontiguousarray(frq, dtype=np.float64).ravel()
        self.elev = np.ascontiguousarray(elev, dtype=np.float64).ravel()
        nch, nang = self.frq.size, self.elev.size
        if nch < 1 or nang < 1:
            raise ValueError("Instrument: at least one channel and one elevation")
        beams = _per_channel(beam, nch, n_beam, gaussian_beam, "beam")
        bands = _per_channel(band, nch, n_band, boxcar_band, "band")
        for a in range(nang):
            for c, (off, _, fwhm) in enumerate(beams):
                nodes = self.elev[a] + off
                bad = (nodes <= 0.0) | (nodes >= 180.0)       # a NaN elevation passes: the operator blanks its rows
                if bad.any():
                    raise ValueError(
                        f"beam node at {nodes[bad][0]:.4g} deg for elevation {self.elev[a]:g} deg, channel {c} "
                        f"({self.frq[c]:g} GHz), is outside (0, 180) deg: ground pickup is not modelled; "
                        + self._largest_fit(self.elev[a], fwhm, off.size))
        for c, (off, _, _) in enumerate(bands):
            if not (self.frq[c] + off > 0.0).all():
                raise ValueError(f"band node of channel {c} ({self.frq[c]:g} GHz) at or below 0 GHz")
        self.elev_q = np.unique(np.concatenate([self.elev[a] + off for a in range(nang) for off, _, _ in beams]))
        self.frq_q = np.unique(np.concatenate([self.frq[c] + off for c, (off, _, _) in enumerate(bands)]))
        if self.elev_q.size > _native.MAX_ANGLES:
            raise ValueError(f"{self.elev_q.size} distinct elevation nodes, more than MWRT_MAX_ANGLES = {_native.MAX_ANGLES} "
                             "of one forward-operator call: fewer beam nodes, fewer distinct beam widths or fewer elevations")
        nf_q = self.frq_q.size
        self.m_in, self.m_out = self.elev_q.size * nf_q, nang * nch
        row_ptr, col, w = [0], [], []
        for a in range(nang):
            for c in range(nch):
                aq = np.searchsorted(self.elev_q, self.elev[a] + beams[c][0])
                fq = np.searchsorted(self.frq_q, self.frq[c] + bands[c][0])
                ww = np.outer(beams[c][1], bands[c][1]).ravel()
                col.append((aq[:, None] * nf_q + fq[None, :]).ravel())
                w.append(ww / math.fsum(ww))
                row_ptr.append(row_ptr[-1] + ww.size)
        self.row_ptr = np.asarray(row_ptr, dtype=np.int32)
        self.col = np.concatenate(col).astype(np.int32)
        self.w = np.concatenate(w)
        self._handles = {}                                    # device index -> (context, native operator)

    @staticmethod
    def _largest_fit(elev, fwhm, n):
        if fwhm is None:
            return "no explicit node may lie there"
        for k in range(n - 1, 0, -1):
            nodes = elev + gaussian_beam(fwhm, k)[0]
            if ((nodes > 0.0) & (nodes < 180.0)).all():
                return f"the largest n that fits is {k}"
        return "no n fits"

    def dense(self):
        """The map as a dense ``[m_out][m_in]`` matrix (tests and small cases); repeated columns of a row add up."""
        d = np.zeros((self.m_out, self.m_in))
        for o in range(self.m_out):
            sl = slice(self.row_ptr[o], self.row_ptr[o + 1])
            np.add.at(d[o], self.col[sl], self.w[sl])
        return d

    # -- on the device --------------------------------------------------------------------------------------------------
    def native_handle(self, device_index=0, ctx=None):
        """(context, operator handle) on a device: created on first use, released with the object.  ``ctx`` is the context
        to create it on (default: ``_native.default_context(device_index)``)."""
        hit = self._handles.get(device_index)
        if hit is None or hit[0]._handle is None or (ctx is not None and hit[0] is not ctx):   # first use, or the context
            if hit is not None:                                                              # was closed or replaced since
                hit[0].obs_destroy(hit[1])
            ctx = _native.default_context(device_index) if ctx is None else ctx
            hit = self._handles[device_index] = (ctx, ctx.obs_create(self.m_in, self.m_out, self.row_ptr, self.col, self.w))
        return hit

    def apply(self, tb, k_blocks=None):
        """Channel quantities from those on the quadrature grid, on torch's current stream: ``tb [nprof][nang_q][nf_q]`` (or
        None) and ``k_blocks``, a sequence of up to four ``[nprof][nang_q][nf_q][nlev]`` K-matrix blocks (or None), float64
        CUDA tensors as the K-matrix call on ``frq_q`` / ``elev_q`` wrote them.  Returns ``(tb_ch [nprof][nang][nch], k_ch)``
        with ``k_ch`` the list of ``[nprof][nang][nch][nlev]`` blocks; what was not given comes back as None."""
        import torch
        from . import retrieval
        ref = tb if tb is not None else k_blocks[0]
        stream = torch.cuda.current_stream(ref.device).cuda_stream if torch.is_tensor(ref) and ref.is_cuda else None
        return retrieval._native_obs_apply(self, tb, k_blocks, stream)

    def param_jacobian(self, model, z, p, t, rh, params, relative=False):
        """The spectroscopic-parameter Jacobian of the CHANNELS (``sensitivity.param_jacobian`` on the quadrature grid,
        reduced by this map with the parameter axis in the place of the levels): ``(tb_ch [nprof][nang][nch],
        kb_ch [nprof][nang][nch][npar], valid [nprof])``."""
        from . import sensitivity
        tb, kb, valid = sensitivity.param_jacobian(model, z, p, t, rh, self.frq_q, self.elev_q, params, relative=relative)
        tb_ch, k_ch = self.apply(tb, [kb])
        return tb_ch, k_ch[0], valid

    def close(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for ctx, h in handles.values():
            ctx.obs_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
