"""NumPy float64 reference of the Levenberg-Marquardt split of the optimal-estimation step (include/mwrt.h
mwrt_oe_lm_prepare_device, mwrt_oe_lm_solve_device, mwrt_oe_cost_device) and of the whole damped loop.

Like oe_reference.py it follows the header literally: dropped observation rows are DELETED, the solves use ``np.linalg``,
and each call reports cond_2 of what it factored.  Arrays are laid out as in oe_reference.py."""
import numpy as np

EPS = np.finfo(np.float64).eps
GAMMAS = (0.0, 0.25, 4.0, 1e3)


def _unpack(k, x, xa):
    k_blocks = [np.asarray(b, dtype=np.float64) for b in k]
    nblk = len(k_blocks)
    nprof, m, nlev = k_blocks[0].shape
    n = nblk * nlev
    x = np.asarray(x, dtype=np.float64).reshape(nprof, n)
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    return k_blocks, nblk, nprof, m, nlev, n, x, xa


def tri_pack(g):
    """[m][m] symmetric -> packed lower triangle, entry (i, j <= i) at i (i + 1) / 2 + j."""
    return g[np.tril_indices(g.shape[0])]


def prepare_reference(k, x, xa, sa, se, y, fx):
    """The linearisation of a batch -> dict of g0 [nprof][m][m] (dropped rows and columns 0), r, kdx [nprof][m], keep
    [nprof][m] uint8, lin_status [nprof], and the forward error bounds of the nested sums: kdx_bound = 2 n eps |K| |dx|
    and g0_bound = 2 n eps |K| |Sa| |K|^T (rows kept)."""
    k_blocks, nblk, nprof, m, nlev, n, x, xa = _unpack(k, x, xa)
    sa, se = np.asarray(sa, dtype=np.float64), np.asarray(se, dtype=np.float64)
    y, fx = np.asarray(y, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    se_row_ok = np.isfinite(se).all(axis=1) if se.ndim == 2 else np.isfinite(se)
    out = dict(g0=np.full((nprof, m, m), np.nan), r=np.full((nprof, m), np.nan), kdx=np.full((nprof, m), np.nan),
               keep=np.zeros((nprof, m), dtype=np.uint8), lin_status=np.zeros(nprof, dtype=np.uint8),
               kdx_bound=np.zeros((nprof, m)), g0_bound=np.zeros((nprof, m, m)))
    for i in range(nprof):
        if not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all()):
            continue                                                        # status 0
        K = np.concatenate([b[i] for b in k_blocks], axis=1)
        rows = np.isfinite(y[i]) & np.isfinite(fx[i]) & np.isfinite(K).all(axis=1) & se_row_ok
        out["g0"][i], out["r"][i], out["kdx"][i] = 0.0, 0.0, 0.0
        if not rows.any():
            out["lin_status"][i] = 3
            continue
        Kk = K[rows]
        dx = x[i] - xa[i]
        out["lin_status"][i] = 1
        out["keep"][i] = rows
        out["r"][i, rows] = y[i, rows] - fx[i, rows]
        out["kdx"][i, rows] = Kk @ dx
        out["kdx_bound"][i, rows] = 2 * n * EPS * (np.abs(Kk) @ np.abs(dx))
        out["g0"][i][np.ix_(rows, rows)] = Kk @ sa @ Kk.T
        out["g0_bound"][i][np.ix_(rows, rows)] = 2 * n * EPS * (np.abs(Kk) @ np.abs(sa) @ np.abs(Kk).T)
    return out


def solve_reference(k, x, xa, sa, se, y, fx, gamma):
    """One damped trial per profile in the m-form -> dict of x_new [nprof][nblk][nlev], status, chi2, nobs and cond
    (cond_2 of G_gamma = K Sa K^T + (1 + gamma) Se on the rows kept; NaN unless status 1)."""
    k_blocks, nblk, nprof, m, nlev, n, x, xa = _unpack(k, x, xa)
    sa, se = np.asarray(sa, dtype=np.float64), np.asarray(se, dtype=np.float64)
    gamma = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (nprof,))
    lin = prepare_reference(k, x, xa, sa, se, y, fx)
    out = dict(x_new=np.full((nprof, n), np.nan), status=np.zeros(nprof, dtype=np.uint8), chi2=np.full(nprof, np.nan),
               nobs=np.zeros(nprof, dtype=np.int32), cond=np.full(nprof, np.nan))
    for i in range(nprof):
        if lin["lin_status"][i] == 0:
            continue
        rows = lin["keep"][i].astype(bool)
        g = gamma[i]
        if not (np.isfinite(g) and g >= 0.0):
            out["status"][i], out["nobs"][i] = 2, rows.sum()
            continue
        dx = x[i] - xa[i]
        if lin["lin_status"][i] == 3:
            out["status"][i], out["x_new"][i], out["chi2"][i] = 3, xa[i] + g / (1.0 + g) * dx, 0.0
            continue
        out["nobs"][i] = rows.sum()
        K = np.concatenate([b[i] for b in k_blocks], axis=1)[rows]
        S = se[np.ix_(rows, rows)] if se.ndim == 2 else np.diag(se[rows])
        G = K @ sa @ K.T + (1.0 + g) * S
        G = 0.5 * (G + G.T)
        d = lin["r"][i, rows] + lin["kdx"][i, rows] / (1.0 + g)
        try:
            if not np.isfinite(G).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            out["status"][i] = 2
            continue
        zv = np.linalg.solve(L, d)
        u = np.linalg.solve(L.T, zv)
        out["status"][i] = 1
        out["x_new"][i] = xa[i] + g / (1.0 + g) * dx + sa @ (K.T @ u)
        out["chi2"][i] = zv @ zv
        out["cond"][i] = np.linalg.cond(G)
    out["x_new"] = out["x_new"].reshape(nprof, nblk, nlev)
    return out


def n_form_damped(k, x, xa, sa, se, y, fx, gamma):
    """Rodgers eq. 5.36 as printed: x+ = x + [(1 + gamma) Sa^-1 + K^T Se^-1 K]^-1 { K^T Se^-1 r - Sa^-1 dx } (finite inputs
    only) -> x_new [nprof][n]."""
    k_blocks, nblk, nprof, m, nlev, n, x, xa = _unpack(k, x, xa)
    S = se if np.ndim(se) == 2 else np.diag(se)
    Si, Sai = np.linalg.inv(S), np.linalg.inv(sa)
    gamma = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (nprof,))
    xs = []
    for i in range(nprof):
        K = np.concatenate([b[i] for b in k_blocks], axis=1)
        dx = x[i] - xa[i]
        lhs = (1.0 + gamma[i]) * Sai + K.T @ Si @ K
        xs.append(x[i] + np.linalg.solve(lhs, K.T @ (Si @ (y[i] - fx[i])) - Sai @ dx))
    return np.array(xs)


def cost_reference(x, xa, se, y, fx, keep, sa_inv):
    """J = r^T (Se,kept)^-1 r + dx^T Sa^-1 dx -> dict of cost, obs, prior [nprof], status, cond (cond_2 of the kept Se) and
    prior_bound = 2 n eps |dx|^T |Sa^-1| |dx|."""
    y, fx = np.asarray(y, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    nprof, m = y.shape
    x = np.asarray(x, dtype=np.float64).reshape(nprof, -1)
    n = x.shape[1]
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    se = np.asarray(se, dtype=np.float64)
    keep = np.asarray(keep).astype(bool)
    out = dict(cost=np.full(nprof, np.nan), obs=np.full(nprof, np.nan), prior=np.full(nprof, np.nan),
               status=np.ones(nprof, dtype=np.uint8), cond=np.full(nprof, np.nan), prior_bound=np.zeros(nprof))
    for i in range(nprof):
        rows = keep[i]
        if not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all() and np.isfinite(y[i, rows]).all()
                and np.isfinite(fx[i, rows]).all()):
            out["cost"][i] = out["obs"][i] = out["prior"][i] = np.inf
            continue
        dx = x[i] - xa[i]
        r = y[i, rows] - fx[i, rows]
        S = se[np.ix_(rows, rows)] if se.ndim == 2 else np.diag(se[rows])
        try:
            if not np.isfinite(S).all() or (se.ndim == 1 and not (se[rows] > 0).all()):
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(S) if rows.any() else np.zeros((0, 0))
        except np.linalg.LinAlgError:
            out["status"][i] = 2
            continue
        zv = np.linalg.solve(L, r) if rows.any() else np.zeros(0)
        out["obs"][i] = zv @ zv
        out["prior"][i] = dx @ sa_inv @ dx
        out["prior_bound"][i] = 2 * n * EPS * (np.abs(dx) @ np.abs(sa_inv) @ np.abs(dx))
        out["cost"][i] = out["obs"][i] + out["prior"][i]
        out["cond"][i] = np.linalg.cond(S) if rows.any() else 1.0
    return out


def retrieve_lm_reference(linearise, forward, clamp, y, xa, sa, se, x0, max_iter=20, tol=0.05, gamma0=1.0, up=10.0, down=10.0,
                          gamma_max=1e8):
    """The damped loop of OneDVar.retrieve_lm on the host.  ``linearise(x) -> (k_blocks, fx)``, ``forward(x) -> fx``,
    ``clamp(x) -> x`` act on [nprof][nblk][nlev] arrays.  -> dict of x, cost, gamma, converged, iterations and ``history``:
    per iteration the dict of accept, cost (after the iteration), gamma, x."""
    x = np.array(x0, dtype=np.float64)
    nprof = x.shape[0]
    sa_inv = np.linalg.inv(sa)
    sa_inv = 0.5 * (sa_inv + sa_inv.T)
    sigma = np.sqrt(np.diag(sa)).reshape(x.shape[1], -1)
    gamma = np.full(nprof, float(gamma0))
    cost = np.full(nprof, np.inf)
    active, stale = np.ones(nprof, bool), np.ones(nprof, bool)
    converged, iters = np.zeros(nprof, bool), np.zeros(nprof, np.int32)
    keep = np.zeros(y.shape, dtype=np.uint8)
    lin_status = np.zeros(nprof, np.uint8)
    history = []
    for _ in range(int(max_iter)):
        if stale.any():
            k, fx = linearise(x)
            lin = prepare_reference(k, x, xa, sa, se, y, fx)
            sel = active & stale
            keep[sel], lin_status[sel] = lin["keep"][sel], lin["lin_status"][sel]
            cost[sel] = cost_reference(x, xa, se, y, fx, keep, sa_inv)["cost"][sel]
            stale[:] = False
            active &= lin_status == 1
        out = solve_reference(k, x, xa, sa, se, np.where(keep.astype(bool), y, np.nan), fx, gamma)
        ok = active & (out["status"] == 1)
        x_try = clamp(np.where(ok[:, None, None], out["x_new"], x))
        cost_try = cost_reference(x_try, xa, se, y, forward(x_try), keep, sa_inv)["cost"]
        accept = ok & (cost_try <= cost)
        move = (np.abs(x_try - x) / sigma).max(axis=(1, 2))
        iters += active
        x = np.where(accept[:, None, None], x_try, x)
        cost = np.where(accept, cost_try, cost)
        gamma = np.where(accept, gamma / down, np.where(active, gamma * up, gamma))
        done = accept & (move < tol)
        converged |= done
        stale |= accept
        active = active & ~done & ~(gamma > gamma_max)
        history.append(dict(accept=accept.copy(), cost=cost.copy(), gamma=gamma.copy(), x=x.copy()))
        if not active.any():
            break
    return dict(x=x, cost=cost, gamma=gamma, converged=converged, iterations=iters, history=history)
