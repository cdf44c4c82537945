"""NumPy float64 reference of the characterisation entries (include/mwrt.h mwrt_oe_gain_device and
mwrt_oe_product_device), on the seeded cases of oe_reference.make_case / SHAPES.

``oe_char_reference`` follows the header's definition literally: dropped observation rows are DELETED, G = K Sa K^T + Se is
factorised with ``np.linalg.cholesky``, the gain comes from solves with that factor, and the deleted rows are put back as
rows of zeros.  Beside the outputs it returns cond_2(G) and the bound matrices |gain|^T |K| and |gain|^T |W| (the sums of
absolute values behind every element of A and S^) that the GPU tests scale their bars by."""
import numpy as np

from oe_reference import COND_MAX, SHAPES, TOL, make_case  # noqa: F401  (the recipe and the bar are shared)

EPS = np.finfo(np.float64).eps


def _window(rows, n):
    return (0, n) if rows is None else (int(rows[0]), int(rows[1]))


def oe_char_reference(k, x, xa, sa, se, y, fx, products=True, rows=None):
    """Both entries for a batch; the arguments are those of ``oe_step_reference``.  -> dict of
    gain, ksa [nprof][m][n]; keep [nprof][m] uint8; avk_diag, noise_var, smooth_var [nprof][nblk][nlev]; dfs_block
    [nprof][nblk]; status uint8, nobs int32, cond [nprof]; bound_diag [nprof][n] = diag(|gain|^T |K|); and with ``products``
    avk, post_cov, bound_avk = |gain|^T |K|, bound_cov = |gain|^T |W|, each [nprof][count][n] for the row window
    ``rows = (begin, count)`` (default: all n rows).  Status 0 and 2: every floating-point output NaN (the products too)."""
    k_blocks = [np.asarray(b, dtype=np.float64) for b in k]
    nblk = len(k_blocks)
    nprof, m, nlev = k_blocks[0].shape
    n = nblk * nlev
    r0, rc = _window(rows, n)
    x = np.asarray(x, dtype=np.float64).reshape(nprof, n)
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    sa, se = np.asarray(sa, dtype=np.float64), np.asarray(se, dtype=np.float64)
    y, fx = np.asarray(y, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    se_full = se.ndim == 2
    se_row_ok = np.isfinite(se).all(axis=1) if se_full else np.isfinite(se)
    nan = lambda *shape: np.full(shape, np.nan)   # noqa: E731
    out = dict(gain=nan(nprof, m, n), ksa=nan(nprof, m, n), keep=np.zeros((nprof, m), dtype=np.uint8),
               avk_diag=nan(nprof, n), noise_var=nan(nprof, n), smooth_var=nan(nprof, n), dfs_block=nan(nprof, nblk),
               status=np.zeros(nprof, dtype=np.uint8), nobs=np.zeros(nprof, dtype=np.int32), cond=nan(nprof),
               bound_diag=nan(nprof, n))
    if products:
        out.update(avk=nan(nprof, rc, n), post_cov=nan(nprof, rc, n), bound_avk=nan(nprof, rc, n), bound_cov=nan(nprof, rc, n))
    for i in range(nprof):
        if not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all()):
            continue                                                        # status 0
        K = np.concatenate([b[i] for b in k_blocks], axis=1)               # [m][n]
        kept = np.isfinite(y[i]) & np.isfinite(fx[i]) & np.isfinite(K).all(axis=1) & se_row_ok
        mu = int(kept.sum())
        if mu == 0:
            out["status"][i] = 3
            for key in ("gain", "ksa", "avk_diag", "noise_var", "dfs_block", "bound_diag"):
                out[key][i] = 0.0
            out["smooth_var"][i] = np.diag(sa)
            if products:
                out["avk"][i] = out["bound_avk"][i] = out["bound_cov"][i] = 0.0
                out["post_cov"][i] = sa[r0:r0 + rc]
            continue
        Kk = K[kept]
        S = se[np.ix_(kept, kept)] if se_full else np.diag(se[kept])
        W = Kk @ sa                                                         # [mu][n]
        G = W @ Kk.T + S
        G = 0.5 * (G + G.T)
        out["nobs"][i] = mu
        try:
            if not np.isfinite(G).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            out["status"][i] = 2
            continue
        Z = np.linalg.solve(L, W)                                           # L^-1 K Sa
        g = np.linalg.solve(L.T, Z)                                         # G^-1 K Sa = gain^T on the rows kept
        out["status"][i] = 1
        out["keep"][i] = kept
        out["gain"][i] = 0.0
        out["gain"][i, kept] = g
        out["ksa"][i] = 0.0
        out["ksa"][i, kept] = W
        out["avk_diag"][i] = (g * Kk).sum(axis=0)
        out["bound_diag"][i] = (np.abs(g) * np.abs(Kk)).sum(axis=0)
        out["noise_var"][i] = ((S @ g) * g).sum(axis=0)
        out["smooth_var"][i] = np.diag(sa) - (Z * Z).sum(axis=0) - out["noise_var"][i]
        out["dfs_block"][i] = out["avk_diag"][i].reshape(nblk, nlev).sum(axis=1)
        out["cond"][i] = np.linalg.cond(G)
        if products:
            gw = g[:, r0:r0 + rc].T                                         # [count][mu]
            out["avk"][i] = gw @ Kk
            out["post_cov"][i] = sa[r0:r0 + rc] - gw @ W
            out["bound_avk"][i] = np.abs(gw) @ np.abs(Kk)
            out["bound_cov"][i] = np.abs(gw) @ np.abs(W)
    for key in ("avk_diag", "noise_var", "smooth_var"):
        out[key] = out[key].reshape(nprof, nblk, nlev)
    return out


def product_reference(gain, keep, right, sa=None, rows=None):
    """The product entry alone: sum over the rows kept of gain[i][j] right[i][k] (``right`` = K [nprof][m][n] or W), or
    Sa minus it, for the row window; and the bound matrix of absolute values.  A row with keep 0 is never touched."""
    nprof, m, n = gain.shape
    r0, rc = _window(rows, n)
    res, bound = np.empty((nprof, rc, n)), np.empty((nprof, rc, n))
    for i in range(nprof):
        kept = keep[i] != 0
        gw = gain[i][kept][:, r0:r0 + rc].T
        c = gw @ right[i][kept]
        bound[i] = np.abs(gw) @ np.abs(right[i][kept])
        res[i] = c if sa is None else sa[r0:r0 + rc] - c
    return res, bound


def char_errors(got, ref, case, rows=None):
    """Largest error of every output in units of its bar's scale (no mask, no floor), over the profiles of status 1:
    gain and ksa of max |ref| per (profile, block); avk and avk_diag of the max of |gain_ref|^T |K| over the sub-block;
    dfs_block of max(1, sum of the block's diagonal of |gain_ref|^T |K|); noise_var, smooth_var and post_cov of
    sqrt(max diag Sa of block bj * of block bk).  Outputs absent from ``got`` (or None) are skipped."""
    nprof, m, n = ref["gain"].shape
    nblk = ref["dfs_block"].shape[1]
    nlev = n // nblk
    r0, rc = _window(rows, n)
    dsa = np.diag(case["sa"]).reshape(nblk, nlev).max(axis=1)
    blk = lambda b: slice(b * nlev, (b + 1) * nlev)   # noqa: E731
    err = {}

    def note(key, value):
        err[key] = max(err.get(key, 0.0), float(value))

    have = lambda key: got.get(key) is not None   # noqa: E731
    for i in range(nprof):
        if ref["status"][i] != 1:
            continue
        bd = ref["bound_diag"][i].reshape(nblk, nlev)
        for b in range(nblk):
            for key in ("gain", "ksa"):
                if have(key):
                    r = ref[key][i][:, blk(b)]
                    note(key, np.abs(got[key][i][:, blk(b)] - r).max() / np.abs(r).max())
            if have("avk_diag"):
                # the sub-block (b, b); without the full bound matrix its diagonal alone, which is no larger
                scale = ref["bound_avk"][i][blk(b), blk(b)].max() if "bound_avk" in ref and rc == n else bd[b].max()
                note("avk_diag", np.abs(got["avk_diag"][i, b] - ref["avk_diag"][i, b]).max() / scale)
            if have("dfs_block"):
                note("dfs_block", abs(got["dfs_block"][i, b] - ref["dfs_block"][i, b]) / max(1.0, bd[b].sum()))
            for key in ("noise_var", "smooth_var"):
                if have(key):
                    note(key, np.abs(got[key][i, b] - ref[key][i, b]).max() / dsa[b])
        for key, bound in (("avk", "bound_avk"), ("post_cov", None)):
            if not have(key):
                continue
            for bj in range(nblk):
                lo, hi = max(bj * nlev, r0) - r0, min((bj + 1) * nlev, r0 + rc) - r0
                if hi <= lo:
                    continue
                for bk in range(nblk):
                    d = np.abs(got[key][i][lo:hi, blk(bk)] - ref[key][i][lo:hi, blk(bk)]).max()
                    scale = ref[bound][i][lo:hi, blk(bk)].max() if bound else np.sqrt(dsa[bj] * dsa[bk])
                    note(key, d / scale)
    return err
