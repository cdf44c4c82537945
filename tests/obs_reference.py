"""NumPy reference of the instrument operator (include/mwrt.h mwrt_obs_apply_device): the CSR map applied in
the stored order of each row, the per-element scale its error bar is stated in, and the quadrature rules restated from
numpy.polynomial alone -- nothing here imports the package under test."""
import math

import numpy as np

U = 2.0 ** -53


def apply_reference(row_ptr, col, w, x):
    """out[p][o][...] = sum over e in [row_ptr[o], row_ptr[o + 1]) of w[e] * x[p][col[e]][...], accumulated from 0.0 in the
    stored order (plain multiply-add: the device's FMA differs by less than the bar).  ``x`` is [nprof][m_in] or
    [nprof][m_in][nlev].  Returns (out, scale) with scale = sum |w[e] x[...]|, the S of the error bar."""
    x = np.asarray(x, dtype=np.float64)
    m_out = len(row_ptr) - 1
    out = np.zeros((x.shape[0], m_out) + x.shape[2:])
    scale = np.zeros_like(out)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in range(m_out):
            for e in range(row_ptr[o], row_ptr[o + 1]):
                term = w[e] * x[:, col[e]]
                out[:, o] = out[:, o] + term
                scale[:, o] = scale[:, o] + np.abs(term)
    return out, scale


def error_bar(row_ptr, scale):
    """|got - ref| <= 4 (nnz_row + 1) 2^-53 S per element: gamma_n of a recursive FMA sum of nnz terms, doubled for the
    reference's own rounding.  Zero where S is zero."""
    nnz = np.diff(np.asarray(row_ptr)).astype(np.float64)
    shape = (1, -1) + (1,) * (scale.ndim - 2)
    return 4.0 * (nnz.reshape(shape) + 1.0) * U * scale


def gaussian_beam_reference(fwhm_deg, n):
    """Gauss-Hermite nodes and weights of a Gaussian of the given full width at half maximum: offsets, weights (sum 1)."""
    x, w = np.polynomial.hermite.hermgauss(n)
    sigma = fwhm_deg / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    return math.sqrt(2.0) * sigma * x, w / math.sqrt(math.pi)


def boxcar_band_reference(bandwidth_ghz, n):
    """Gauss-Legendre nodes and weights of a rectangular band: offsets, weights (sum 1)."""
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * bandwidth_ghz * x, 0.5 * w


def dense_reference(frq, elev, beams, bands, elev_q, frq_q):
    """The [nang * nch][nang_q * nf_q] matrix of per-channel (offsets, weights) beams and bands on a given grid, rows
    angle-major, built entry by entry."""
    nch, nf_q = len(frq), len(frq_q)
    d = np.zeros((len(elev) * nch, len(elev_q) * nf_q))
    for a, el in enumerate(elev):
        for c, f in enumerate(frq):
            for db, wb in zip(*beams[c]):
                for df, wf in zip(*bands[c]):
                    aq = int(np.argmin(np.abs(np.asarray(elev_q) - (el + db))))
                    fq = int(np.argmin(np.abs(np.asarray(frq_q) - (f + df))))
                    d[a * nch + c, aq * nf_q + fq] += wb * wf
    return d
