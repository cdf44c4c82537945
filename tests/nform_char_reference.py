"""NumPy float64 reference of the n-form's characterisation (include/mwrt.h mwrt_oe_nform_char_device and
mwrt_oe_nform_gain_device) on the seeded cases and shapes of tests/nform_reference.py.

It follows the header literally: the linearisation is ``nform_reference.prepare_reference`` (dropped rows DELETED),
C = H + Sa^-1 is factorised with ``np.linalg.cholesky`` and every output comes from solves with that factor; the deleted
rows of the gain are put back as rows of zeros.  ``char_linearisation`` and ``gain_rows`` are the two entries as they are
called, on a stored linearisation -- what the CPU tests of retrieval.py put in their place.

Beside the outputs it returns the bound matrix |S^| |H| (the sums of absolute values behind every element of A) and cond_2
of the Jacobi-scaled C.  The error units are those of ``oe_char_reference.char_errors`` with |S^| |H| in the place of
|gain|^T |K|: gain of max |ref| per (profile, block); A and avk_diag of the bound over the sub-block; dfs_block of
max(1, sum of the block's bound diagonal); noise_var, smooth_var and post_cov of sqrt(max diag Sa of block j * of block k).
The bar is ``nform_reference.TOL`` (Cholesky and its solves at cond <= COND_MAX; derived there)."""
import numpy as np

import nform_reference as nfr
from oe_char_reference import char_errors  # noqa: F401  (the units are shared: the reference dict has its keys)

# shapes beside nform_reference.SHAPES that the gain's tile plan asks for (tests/test_nform_char_kernel_resources.py holds
# the union against the plan as built): a last row tile full and short by one, three blocks with two row tiles by one row
EDGE_SHAPES = [(8, 1, 128), (9, 2, 127), (5, 3, 129), (40, 1, 256)]
SHAPES = nfr.SHAPES + EDGE_SHAPES


def _window(rows, n):
    return (0, n) if rows is None or tuple(rows) == (0, 0) else (int(rows[0]), int(rows[1]))


def char_linearisation(h, lin_status, sa_inv, nblk, rows=None):
    """mwrt_oe_nform_char_device on a stored linearisation (``h`` packed [nprof][n (n + 1) / 2] or full [nprof][n][n]) ->
    dict of status, post_cov_full [nprof][n][n], post_cov and avk [nprof][count][n] (the row window), avk_diag, noise_var,
    smooth_var [nprof][nblk][nlev], dfs_block [nprof][nblk], cond [nprof], bound_avk [nprof][count][n], bound_diag
    [nprof][n]."""
    sa_inv = np.asarray(sa_inv, dtype=np.float64)
    n = sa_inv.shape[0]
    nprof, nlev = len(lin_status), n // nblk
    r0, rc = _window(rows, n)
    nan = lambda *shape: np.full(shape, np.nan)   # noqa: E731
    out = dict(status=np.zeros(nprof, dtype=np.uint8), post_cov_full=nan(nprof, n, n), avk=nan(nprof, rc, n),
               avk_diag=nan(nprof, n), noise_var=nan(nprof, n), smooth_var=nan(nprof, n), dfs_block=nan(nprof, nblk),
               cond=nan(nprof), bound_avk=nan(nprof, rc, n), bound_diag=nan(nprof, n))
    il = np.tril_indices(n)
    for i in range(nprof):
        ls = lin_status[i]
        if ls == 0:
            continue
        if ls not in (1, 3):
            out["status"][i] = 2
            continue
        H = np.zeros((n, n))
        if ls == 1:
            if np.ndim(h[i]) == 1:
                H[il] = h[i]
                H = H + np.tril(H, -1).T
            else:
                H = np.array(h[i], dtype=np.float64)
        C = H + sa_inv
        try:
            if not np.isfinite(C).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(0.5 * (C + C.T))
        except np.linalg.LinAlgError:
            out["status"][i] = 2 if ls == 1 else 3
            if ls == 3:
                for key in ("avk", "avk_diag", "noise_var", "dfs_block", "bound_avk", "bound_diag"):
                    out[key][i] = 0.0
            continue
        Li = np.linalg.solve(L, np.eye(n))
        post = Li.T @ Li
        out["post_cov_full"][i] = post
        if ls == 3:
            out["status"][i] = 3
            for key in ("avk", "avk_diag", "noise_var", "dfs_block", "bound_avk", "bound_diag"):
                out[key][i] = 0.0
            out["smooth_var"][i] = np.diag(post)
            continue
        A = np.linalg.solve(L.T, np.linalg.solve(L, H))                  # C^-1 H
        bound = np.abs(post) @ np.abs(H)
        noise = np.einsum("jk,kj->j", A, post)
        scale = 1.0 / np.sqrt(np.diag(C))
        out["status"][i] = 1
        out["avk"][i], out["bound_avk"][i] = A[r0:r0 + rc], bound[r0:r0 + rc]
        out["avk_diag"][i], out["bound_diag"][i] = np.diag(A), np.diag(bound)
        out["noise_var"][i], out["smooth_var"][i] = noise, np.diag(post) - noise
        out["dfs_block"][i] = np.diag(A).reshape(nblk, nlev).sum(axis=1)
        out["cond"][i] = np.linalg.cond(C * scale[:, None] * scale[None, :])
    out["post_cov"] = out["post_cov_full"][:, r0:r0 + rc]
    for key in ("avk_diag", "noise_var", "smooth_var"):
        out[key] = out[key].reshape(nprof, nblk, nlev)
    return out


def gain_rows(k, se, keep, post_cov, status):
    """mwrt_oe_nform_gain_device: row i of profile p is S^ k_i / se_i on the rows ``keep`` names, 0 in the others; NaN
    throughout at status 0 or 2, 0 throughout at status 3.  -> [nprof][m][n]"""
    k_blocks = [np.asarray(b, dtype=np.float64) for b in k]
    nprof, m = keep.shape
    kf = np.concatenate([b.reshape(nprof, m, -1) for b in k_blocks], axis=2)
    n = kf.shape[2]
    se = np.broadcast_to(np.asarray(se, dtype=np.float64).reshape(-1, m), (nprof, m))
    gain = np.full((nprof, m, n), np.nan)
    for i in range(nprof):
        if status[i] == 3:
            gain[i] = 0.0
        if status[i] != 1:
            continue
        rows = np.asarray(keep[i]).astype(bool)
        gain[i] = 0.0
        gain[i, rows] = (kf[i, rows] / se[i, rows, None]) @ post_cov[i]
    return gain


def nform_char_reference(k, x, xa, sa_inv, se, y, fx, rows=None):
    """Both entries for a batch; the arguments are those of ``nform_reference.solve_reference``.  -> the dict of
    ``char_linearisation`` and gain [nprof][m][n] (from solves with the factor of C), keep, nobs, lin_status."""
    lin = nfr.prepare_reference(k, x, xa, se, y, fx)
    nblk = len(k)
    out = char_linearisation(lin["h"], lin["lin_status"], sa_inv, nblk, rows)
    nprof, m = lin["keep"].shape
    n = np.asarray(sa_inv).shape[0]
    sev = np.broadcast_to(np.asarray(se, dtype=np.float64).reshape(-1, m), (nprof, m))
    gain = np.full((nprof, m, n), np.nan)
    for i in range(nprof):
        if out["status"][i] == 3:
            gain[i] = 0.0
        if out["status"][i] != 1:
            continue
        kept = lin["keep"][i].astype(bool)
        K = np.concatenate([np.asarray(b[i], dtype=np.float64) for b in k], axis=1)[kept]
        C = lin["h"][i] + np.asarray(sa_inv)
        L = np.linalg.cholesky(0.5 * (C + C.T))
        rhs = (K / sev[i, kept, None]).T                                  # [n][m_used]: the columns k_i / se_i
        gain[i] = 0.0
        gain[i, kept] = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).T
    out.update(gain=gain, keep=lin["keep"], nobs=lin["nobs"], lin_status=lin["lin_status"])
    return out
