"""NumPy float64 reference of one optimal-estimation step (include/mwrt.h mwrt_oe_step_device) and the seeded
case recipe the CPU and GPU tests share.

``oe_step_reference`` follows the header's definition literally: dropped observation rows are DELETED, G = K Sa K^T + Se is
factorised with ``np.linalg.cholesky`` and every output comes from solves with that factor."""
import numpy as np

SIGMA = (2.0, 0.3, 0.05, 0.05)                 # prior standard deviation per state block
AMPL = (0.05, 3.0, 40.0, 40.0)                 # K-row amplitude per block (times min(1, 16 / nlev))
TOL = 1e-8                                     # c m eps cond(G) with c = 64, m <= 140, cond <= 1e4
COND_MAX = 1e4
SEED = 2009                                    # a draw whose every case meets COND_MAX (test_oe_reference.py checks)

# (nlev, nblk, m): wave seams of the level axis, panel remainders, m not a multiple of any tile, m = 1, the m limit
SHAPES = [(2, 1, 1), (2, 2, 3), (3, 3, 14), (33, 1, 17), (63, 2, 14), (64, 2, 15), (65, 2, 98), (180, 2, 98),
          (180, 3, 140), (1024, 2, 140)]


def oe_step_reference(k, x, xa, sa, se, y, fx):
    """One step for a batch.  k: sequence of [nprof][m][nlev]; x [nprof][nblk][nlev]; xa [nblk][nlev] or
    [nprof][nblk][nlev]; sa [n][n]; se [m] or [m][m]; y, fx [nprof][m].
    -> dict of x_new [nprof][nblk][nlev], status, chi2, dfs, post_var, nobs, and cond (cond_2 of G, NaN unless status 1)."""
    k_blocks = [np.asarray(b, dtype=np.float64) for b in k]
    nblk = len(k_blocks)
    nprof, m, nlev = k_blocks[0].shape
    n = nblk * nlev
    x = np.asarray(x, dtype=np.float64).reshape(nprof, n)
    xa = np.asarray(xa, dtype=np.float64)
    xa = np.broadcast_to(xa.reshape(-1, n), (nprof, n))
    sa, se = np.asarray(sa, dtype=np.float64), np.asarray(se, dtype=np.float64)
    y, fx = np.asarray(y, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    se_full = se.ndim == 2
    se_row_ok = np.isfinite(se).all(axis=1) if se_full else np.isfinite(se)
    out = dict(x_new=np.full((nprof, n), np.nan), status=np.zeros(nprof, dtype=np.uint8), chi2=np.full(nprof, np.nan),
               dfs=np.full(nprof, np.nan), post_var=np.full((nprof, n), np.nan), nobs=np.zeros(nprof, dtype=np.int32),
               cond=np.full(nprof, np.nan))
    for i in range(nprof):
        if not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all()):
            continue                                                        # status 0
        K = np.concatenate([b[i] for b in k_blocks], axis=1)               # [m][n]
        rows = np.isfinite(y[i]) & np.isfinite(fx[i]) & np.isfinite(K).all(axis=1) & se_row_ok
        mu = int(rows.sum())
        if mu == 0:
            out["status"][i], out["x_new"][i], out["chi2"][i], out["dfs"][i] = 3, xa[i], 0.0, 0.0
            out["post_var"][i] = np.diag(sa)
            continue
        K = K[rows]
        S = se[np.ix_(rows, rows)] if se_full else np.diag(se[rows])
        d = y[i, rows] - fx[i, rows] + K @ (x[i] - xa[i])
        W = K @ sa                                                          # [mu][n]
        G = W @ K.T + S
        G = 0.5 * (G + G.T)
        out["nobs"][i] = mu
        try:
            if not np.isfinite(G).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            out["status"][i] = 2
            continue
        zv = np.linalg.solve(L, d)
        u = np.linalg.solve(L.T, zv)
        Z = np.linalg.solve(L, W)                                           # L^-1 K Sa
        out["status"][i] = 1
        out["x_new"][i] = xa[i] + W.T @ u
        out["chi2"][i] = zv @ zv
        out["dfs"][i] = mu - np.trace(np.linalg.solve(L.T, np.linalg.solve(L, S)))
        out["post_var"][i] = np.diag(sa) - (Z * Z).sum(axis=0)
        out["cond"][i] = np.linalg.cond(G)
    out["x_new"] = out["x_new"].reshape(nprof, nblk, nlev)
    out["post_var"] = out["post_var"].reshape(nprof, nblk, nlev)
    return out


def n_form_reference(k, x, xa, sa, se, y, fx):
    """The same step in the n-form, x+ = xa + (K^T Se^-1 K + Sa^-1)^-1 K^T Se^-1 d, with its posterior covariance and
    averaging kernel -- for the cross-form check (finite inputs only).  -> x_new [nprof][n], post [nprof][n][n], dfs."""
    k_blocks = k
    nblk = len(k_blocks)
    nprof, m, nlev = k_blocks[0].shape
    n = nblk * nlev
    x = np.asarray(x, dtype=np.float64).reshape(nprof, n)
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    S = se if np.ndim(se) == 2 else np.diag(se)
    Si, Sai = np.linalg.inv(S), np.linalg.inv(sa)
    xs, posts, dfs = [], [], []
    for i in range(nprof):
        K = np.concatenate([b[i] for b in k_blocks], axis=1)
        d = y[i] - fx[i] + K @ (x[i] - xa[i])
        post = np.linalg.inv(K.T @ Si @ K + Sai)
        xs.append(xa[i] + post @ (K.T @ (Si @ d)))
        posts.append(post)
        dfs.append(np.trace(post @ K.T @ Si @ K))
    return np.array(xs), np.array(posts), np.array(dfs)


def make_case(nlev, nblk, m, nprof=4, se_full=False, xa_per_profile=False, seed=SEED):
    """The seeded recipe: smooth weighting-function rows, exponentially correlated prior, white or correlated noise.
    Profile i is drawn from its own stream, so it is the same profile whatever nprof is."""
    lev = np.arange(nlev, dtype=np.float64)
    scale = min(1.0, 16.0 / nlev)
    sig = np.array(SIGMA[:nblk])[:, None]
    k_blocks = [np.empty((nprof, m, nlev)) for _ in range(nblk)]
    x, xap = np.empty((nprof, nblk, nlev)), np.empty((nprof, nblk, nlev))
    y, fx = np.empty((nprof, m)), np.empty((nprof, m))
    xa_shared = np.random.default_rng([seed, nlev, nblk, m, 10 ** 6]).standard_normal((nblk, nlev)) * sig
    for i in range(nprof):
        rng = np.random.default_rng([seed, nlev, nblk, m, i])
        for b in range(nblk):
            a = AMPL[b] * scale
            c = rng.uniform(0.0, nlev - 1, size=(m, 1))
            w = rng.uniform(1.0, max(nlev / 3.0, 1.5), size=(m, 1))
            u = rng.uniform(0.2, 1.0, size=(m, 1))
            k_blocks[b][i] = u * a * np.exp(-((lev - c) / w) ** 2) + 1e-3 * a * rng.standard_normal((m, nlev))
        xap[i] = rng.standard_normal((nblk, nlev)) * sig
        x[i] = (xap[i] if xa_per_profile else xa_shared) + 0.1 * rng.standard_normal((nblk, nlev))
        fx[i] = 250.0 + 20.0 * rng.standard_normal(m)
        y[i] = fx[i] + rng.standard_normal(m)
    n = nblk * nlev
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / max(nlev / 6.0, 1.0))
    sa = np.zeros((n, n))
    for b in range(nblk):
        sa[b * nlev:(b + 1) * nlev, b * nlev:(b + 1) * nlev] = SIGMA[b] ** 2 * corr
    if nblk > 1:
        cross = 0.3 * SIGMA[0] * SIGMA[1] * corr
        sa[:nlev, nlev:2 * nlev] = cross
        sa[nlev:2 * nlev, :nlev] = cross.T
    if se_full:
        i = np.arange(m, dtype=np.float64)
        se = 0.7 * 0.25 * np.eye(m) + 0.3 * 0.25 * np.exp(-np.abs(i[:, None] - i[None, :]) / 3.0)
    else:
        se = np.full(m, 0.25)
    return dict(k=k_blocks, x=x, xa=xap if xa_per_profile else xa_shared, sa=sa, se=se, y=y, fx=fx)


def block_errors(got, ref, case):
    """Largest error of every output in units of its bar's scale (no mask, no floor): x_new of
    max |x_ref - xa| per block, post_var of max diag Sa per block, chi2 and dfs of max(1, |ref|)."""
    nprof, nblk, nlev = ref["x_new"].shape
    xa = np.broadcast_to(case["xa"], ref["x_new"].shape)
    dsa = np.diag(case["sa"]).reshape(nblk, nlev)
    err = dict(x_new=0.0, post_var=0.0, chi2=0.0, dfs=0.0)
    for i in range(nprof):
        if ref["status"][i] != 1:
            continue
        for b in range(nblk):
            sx = np.abs(ref["x_new"][i, b] - xa[i, b]).max()
            err["x_new"] = max(err["x_new"], float(np.abs(got["x_new"][i, b] - ref["x_new"][i, b]).max() / sx))
            if got.get("post_var") is not None:
                err["post_var"] = max(err["post_var"], float(np.abs(got["post_var"][i, b] - ref["post_var"][i, b]).max() / dsa[b].max()))
        for k in ("chi2", "dfs"):
            if got.get(k) is not None:
                err[k] = max(err[k], float(abs(got[k][i] - ref[k][i]) / max(1.0, abs(ref[k][i]))))
    return err
