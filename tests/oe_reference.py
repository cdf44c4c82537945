"""NumPy float64 reference of one optimal-estimation step (include/mwrt.h mwrt_oe_step_device) and the seeded
case recipe the CPU and GPU tests share.

``oe_step_reference`` follows the header's definition literally: dropped observation rows are DELETED, G = K Sa K^T + Se is
factorised with ``np.linalg.cholesky`` and every output comes from solves with that factor."""
import functools

import numpy as np

SIGMA = (2.0, 0.3, 0.05, 0.05)                 # prior standard deviation per state block
AMPL = (0.05, 3.0, 40.0, 40.0)                 # K-row amplitude per block (times min(1, 16 / nlev))
TOL = 1e-8                                     # c m eps cond(G) with c = 64, m <= 140, cond <= 1e4
COND_MAX = 1e4
SEED = 2009                                    # a draw whose every case meets COND_MAX (test_oe_reference.py checks)

# (nlev, nblk, m).  What the list reaches is asserted, not described, by
# tests/test_oe_shape_coverage.py::test_the_shapes_reach_what_they_are_for, against the LDS plans and the launchers'
# dispatch rule as the code has them: every row-tile count ceil(m / 32) = 1 .. 5 with both sides of every tile edge, m = 1
# and the m limit, one to four state blocks, both sides of wave 0's register seams (m = 64 | 65, 128 | 129), both sides of
# the first raise of every kernel's LDS limit, the two shapes whose state vector outgrows the panel buffers it aliases, a
# panel remainder and the wave seam of the level axis.  A shape added here needs cond_2(G) <= COND_MAX for SEED
# (test_oe_reference.py checks); a shape taken away has to leave that test passing.
SHAPES = [(2, 1, 1), (2, 2, 3), (3, 3, 14), (33, 1, 17), (63, 2, 14), (64, 2, 15), (65, 2, 98), (180, 2, 98),
          (180, 3, 140), (1024, 2, 140),
          (33, 1, 32), (33, 1, 33),                      # one tile exactly | the second by one row; n = 33
          (20, 4, 40),                                   # four state blocks
          (64, 2, 64), (65, 2, 65),                      # two tiles exactly | the third by one row: v0's last lane | v1's first
          (65, 2, 64),                                   # ... and at one n, 130: the first LDS raise of k_char_gain
          (65, 2, 69), (65, 2, 70),                      # the first LDS raise of k_oe_step and k_lm_prepare at n = 130
          (129, 1, 96), (129, 1, 97),                    # three tiles exactly | the fourth by one row
          (65, 2, 122), (65, 2, 123),                    # ... of k_lm_cost with a full Se
          (65, 2, 124), (65, 2, 125),                    # ... of k_lm_solve
          (65, 2, 128), (65, 2, 129),                    # four tiles exactly | the fifth by one row: v1's last lane | v2's first
          (700, 3, 14), (909, 4, 33)]                    # n = 2100 and 3636: four doubles beyond the panel buffers of 1 and 2 tiles


# Rows dropped at the seams of m = 65 (three row tiles, row 64 alone in the third and alone in wave 0's second register):
# the last row of a tile, the first of the next, a whole tile, and every row but one.  A principal submatrix of a symmetric
# positive-definite G is no worse conditioned than G, so COND_MAX holds for every pattern (and is asserted on each).
SEAM_SHAPE = (65, 2, 65)
SEAM_DROPS = {"row-31": (31,), "row-32": (32,), "row-63": (63,), "row-64": (64,), "tile-32-63": tuple(range(32, 64)),
              "all-but-64": tuple(range(64))}


def copy_case(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else [b.copy() for b in v]) for k, v in case.items()}


def drop_rows(case, what, rows, prof):
    """A copy of ``case`` in which profile ``prof`` loses ``rows``: NaN in y ("y"), or in one element of the row in one
    K block ("k"; block and level change with the row)."""
    bad = copy_case(case)
    nblk, nlev = len(bad["k"]), bad["k"][0].shape[2]
    for row in rows:
        if what == "k":
            bad["k"][row % nblk][prof, row, (7 * row) % nlev] = np.nan
        else:
            bad[what][prof, row] = np.nan
    return bad


def one_profile(outputs, i):
    """Profile i of a dict of per-profile outputs, as a batch of one: for the error of that profile alone."""
    return {k: (None if v is None else v[i:i + 1]) for k, v in outputs.items()}


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


@functools.lru_cache(maxsize=None)
def prior_covariance(nlev, nblk):
    """Sa of the recipe: exponentially correlated blocks, the first two coupled.  It depends on (nlev, nblk) alone, so the
    cases of a shape share one array (105 MB at n = 3636) and what is derived from it once, like its inverse; nobody
    writes to it."""
    lev = np.arange(nlev, dtype=np.float64)
    n = nblk * nlev
    corr = np.exp(-np.abs(lev[:, None] - lev[None, :]) / max(nlev / 6.0, 1.0))
    sa = np.zeros((n, n))
    for b in range(nblk):
        sa[b * nlev:(b + 1) * nlev, b * nlev:(b + 1) * nlev] = SIGMA[b] ** 2 * corr
    if nblk > 1:
        cross = 0.3 * SIGMA[0] * SIGMA[1] * corr
        sa[:nlev, nlev:2 * nlev] = cross
        sa[nlev:2 * nlev, :nlev] = cross.T
    return sa


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
    sa = prior_covariance(nlev, nblk)
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
