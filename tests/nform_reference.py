"""NumPy float64 reference of the n-form of the optimal-estimation step (include/mwrt.h mwrt_oe_nform_prepare_device,
mwrt_oe_nform_solve_device, mwrt_oe_nform_cost_device), the seeded case recipe and the shapes the CPU and GPU
tests share.

It follows the header literally: dropped observation rows are DELETED, C = H + (1 + gamma) Sa^-1 is factorised with
``np.linalg.cholesky`` and every output comes from solves with that factor.  K, x, xa, y, fx and Sa are those of
``oe_reference.make_case``; the observation error is variances only, shared or per profile.

Bars (derived, not measured):
  solve     Cholesky and its solves are backward stable: error <~ c n eps cond with c = 64, n <= 128 and cond <= COND_MAX on
            the JACOBI-SCALED C (C_ij / sqrt(C_ii C_jj)): Cholesky's error bound is invariant under that scaling, and the
            kernels keep their bits under a change of units (tests/test_oe_scaling.py) (the
            unscaled C reaches 4e6 at four blocks, whose units differ).  TOL = 64 * 128 * eps * 1e4 = 1.8e-8 in the units of
            ``solve_errors``: max |x_ref - xa| per block for x_new, max diag Sa per block for post_var, max |C^-1| for
            post_cov, max(1, |ref|) for dfs, max(1, d^T W d) for chi2 -- the scale at which its formula subtracts.
  prepare   a length-m dot product errs by at most m eps sum |terms| and, for H, sum |terms| <= sqrt(H_ii H_jj): 64 m eps
            in units of max diag H; g in units of sum_i |K_ij w_i r_i|, r^T W r relative.
  cost      the same with m + n terms: 64 (m + n) eps of sum_kept r^2 / se + |dx|^T |Sa^-1| |dx|."""
import numpy as np

import oe_reference as oer

EPS = np.finfo(np.float64).eps
COND_MAX = 1e4                                 # on the Jacobi-scaled C, asserted per case and per profile
TOL = 64 * 128 * EPS * COND_MAX                # 1.8e-8
GAMMAS = (0.0, 0.5, 1e3)                       # beside gamma = 0 as a NULL pointer

# (nlev, nblk, m): n = nblk nlev <= 128, m unbounded.  What the list reaches is asserted by
# tests/test_nform_kernel_resources.py::test_the_shapes_keep_both_sides_of_every_edge against the plan constants of
# csrc/mwrt_nform.hip.h as built.
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 2, 3), (8, 1, 98), (31, 1, 14), (32, 1, 98), (33, 1, 141),
          (64, 1, 140), (65, 1, 300),                    # a lane's second column of K: n = 64 | 65
          (43, 2, 154), (32, 4, 98),                     # a coarse full state; n = 128 in four blocks
          (127, 1, 98), (128, 1, 513), (16, 2, 1025),
          (22, 4, 16), (89, 1, 17),                      # one tile per thread | two (n = 88 | 89); one row chunk | a second by one row
          (124, 1, 32), (125, 1, 33),                    # two tiles per thread | three (n = 124 | 125); two chunks | a third by one row
          (121, 1, 15), (122, 1, 31)]                    # the solve's first raise of its LDS limit (n = 121 | 122); a chunk short by one row


def make_case(nlev, nblk, m, nprof=4, se_per_profile=False, xa_per_profile=False):
    """oe_reference.make_case with variances alone: 0.25 shared, or 0.25 .. 0.5 per profile and row (profile i from its
    own stream, so it is the same profile whatever nprof is)."""
    case = oer.make_case(nlev, nblk, m, nprof=nprof, xa_per_profile=xa_per_profile)
    if se_per_profile:
        case["se"] = np.stack([0.25 * (1.0 + np.random.default_rng([oer.SEED, nlev, nblk, m, i, 7]).uniform(0.0, 1.0, m))
                               for i in range(nprof)])
    return case


_inverses = []


def sym_inv(sa):
    """The symmetrised inverse of Sa, computed once per array object; nobody writes to either."""
    for held, inv in _inverses:
        if held is sa:
            return inv
    inv = np.linalg.inv(sa)
    inv = 0.5 * (inv + inv.T)
    _inverses.append((sa, inv))
    return inv


def tri_pack(h):
    """[n][n] symmetric -> packed lower triangle, entry (i, j <= i) at i (i + 1) / 2 + j."""
    return h[np.tril_indices(h.shape[0])]


def _unpack(k, x, xa, se):
    k_blocks = [np.asarray(b, dtype=np.float64) for b in k]
    nblk = len(k_blocks)
    nprof, m, nlev = k_blocks[0].shape
    n = nblk * nlev
    x = np.asarray(x, dtype=np.float64).reshape(nprof, n)
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    se = np.broadcast_to(np.asarray(se, dtype=np.float64).reshape(-1, m), (nprof, m))
    return k_blocks, nblk, nprof, m, nlev, n, x, xa, se


def prepare_reference(k, x, xa, se, y, fx):
    """The linearisation of a batch -> dict of h [nprof][n][n], g [nprof][n], rwr [nprof], keep [nprof][m] uint8, nobs,
    lin_status, and the scales of the bars: h_scale [nprof] = max diag H, g_scale [nprof][n] = sum_i |K_ij w_i r_i|."""
    k_blocks, nblk, nprof, m, nlev, n, x, xa, se = _unpack(k, x, xa, se)
    y, fx = np.asarray(y, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    out = dict(h=np.full((nprof, n, n), np.nan), g=np.full((nprof, n), np.nan), rwr=np.full(nprof, np.nan),
               keep=np.zeros((nprof, m), dtype=np.uint8), nobs=np.zeros(nprof, dtype=np.int32),
               lin_status=np.zeros(nprof, dtype=np.uint8), h_scale=np.zeros(nprof), g_scale=np.zeros((nprof, n)))
    for i in range(nprof):
        if not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all()):
            continue                                                        # status 0
        K = np.concatenate([b[i] for b in k_blocks], axis=1)
        rows = np.isfinite(y[i]) & np.isfinite(fx[i]) & np.isfinite(K).all(axis=1) & np.isfinite(se[i])
        out["keep"][i], out["nobs"][i] = rows, rows.sum()
        if not rows.any():
            out["lin_status"][i], out["h"][i], out["g"][i], out["rwr"][i] = 3, 0.0, 0.0, 0.0
            continue
        if not (se[i, rows] > 0.0).all():
            out["lin_status"][i] = 2
            continue
        Kk, w, r = K[rows], 1.0 / se[i, rows], y[i, rows] - fx[i, rows]
        out["lin_status"][i] = 1
        out["h"][i] = Kk.T @ (w[:, None] * Kk)
        out["g"][i] = Kk.T @ (w * r)
        out["rwr"][i] = r @ (w * r)
        out["h_scale"][i] = np.diag(out["h"][i]).max()
        out["g_scale"][i] = np.abs(Kk * (w * r)[:, None]).sum(axis=0)
    return out


def solve_reference(k, x, xa, sa_inv, se, y, fx, gamma=None):
    """One step per profile (gamma None: 0) -> dict of x_new [nprof][nblk][nlev], status, nobs, chi2, dfs, post_var
    [nprof][nblk][nlev], post_cov [nprof][n][n] (the four at gamma = 0 only: NaN otherwise), cond (cond_2 of the
    Jacobi-scaled C; NaN unless status 1) and dwd = d^T W d with d = r + K (x - xa), the scale of chi2's bar."""
    k_blocks, nblk, nprof, m, nlev, n, x, xa, se = _unpack(k, x, xa, se)
    sa_inv = np.asarray(sa_inv, dtype=np.float64)
    diagnostics = gamma is None
    gamma = np.broadcast_to(np.asarray(0.0 if gamma is None else gamma, dtype=np.float64), (nprof,))
    lin = prepare_reference(k, x, xa, se, y, fx)
    out = dict(x_new=np.full((nprof, n), np.nan), status=np.zeros(nprof, dtype=np.uint8), nobs=lin["nobs"],
               chi2=np.full(nprof, np.nan), dfs=np.full(nprof, np.nan), post_var=np.full((nprof, n), np.nan),
               post_cov=np.full((nprof, n, n), np.nan), cond=np.full(nprof, np.nan), dwd=np.full(nprof, np.nan))
    for i in range(nprof):
        ls, g = lin["lin_status"][i], gamma[i]
        if ls == 0:
            continue
        if ls == 2 or not (np.isfinite(g) and g >= 0.0):
            out["status"][i] = 2
            continue
        dx = x[i] - xa[i]
        if ls == 3:
            out["status"][i] = 3
            out["x_new"][i] = xa[i] if g == 0.0 else xa[i] + g / (1.0 + g) * dx
            if diagnostics:
                L = np.linalg.cholesky(sa_inv)
                Li = np.linalg.solve(L, np.eye(n))
                out["chi2"][i], out["dfs"][i], out["post_cov"][i] = 0.0, 0.0, Li.T @ Li
                out["post_var"][i] = np.diag(out["post_cov"][i])
            continue
        H = lin["h"][i]
        C = H + (1.0 + g) * sa_inv
        C = 0.5 * (C + C.T)
        try:
            if not np.isfinite(C).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(C)
        except np.linalg.LinAlgError:
            out["status"][i] = 2
            continue
        rhs = lin["g"][i] - sa_inv @ dx
        s = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        out["status"][i] = 1
        out["x_new"][i] = x[i] + s
        scale = 1.0 / np.sqrt(np.diag(C))
        out["cond"][i] = np.linalg.cond(C * scale[:, None] * scale[None, :])
        if diagnostics:
            rows = lin["keep"][i].astype(bool)
            K = np.concatenate([b[i] for b in k_blocks], axis=1)[rows]
            w, r = 1.0 / se[i, rows], y[i, rows] - fx[i, rows]
            lin_res = r - K @ s                                          # the residual at the linear solution
            e = out["x_new"][i] - xa[i]
            Li = np.linalg.solve(L, np.eye(n))
            post = Li.T @ Li
            d = r + K @ dx
            out["chi2"][i] = lin_res @ (w * lin_res) + e @ sa_inv @ e
            out["dfs"][i] = np.sum(post * H)
            out["post_cov"][i], out["post_var"][i] = post, np.diag(post)
            out["dwd"][i] = d @ (w * d)
    out["x_new"] = out["x_new"].reshape(nprof, nblk, nlev)
    out["post_var"] = out["post_var"].reshape(nprof, nblk, nlev)
    return out


def solve_linearisation(h, g, rwr, lin_status, x, xa, sa_inv, gamma=None):
    """The solve entry as it is called: on a STORED linearisation (h packed [nprof][n (n + 1) / 2], g, rwr, lin_status), with
    chi2 by the header's formula (r^T W r - 2 s^T g + s^T H s) + e^T Sa^-1 e -> dict of x_new [nprof][n], status, chi2, dfs,
    post_var [nprof][n], post_cov (the four NaN when gamma is given).  What the CPU tests of retrieval.py put in the place of
    mwrt_oe_nform_solve_device."""
    x = np.asarray(x, dtype=np.float64)
    nprof = x.shape[0]
    x = x.reshape(nprof, -1)
    n = x.shape[1]
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    diagnostics = gamma is None
    gamma = np.broadcast_to(np.asarray(0.0 if gamma is None else gamma, dtype=np.float64), (nprof,))
    out = dict(x_new=np.full((nprof, n), np.nan), status=np.zeros(nprof, dtype=np.uint8), chi2=np.full(nprof, np.nan),
               dfs=np.full(nprof, np.nan), post_var=np.full((nprof, n), np.nan), post_cov=np.full((nprof, n, n), np.nan))
    il = np.tril_indices(n)
    for i in range(nprof):
        ls, gm = lin_status[i], gamma[i]
        if ls == 0 or not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all()):
            continue
        if ls not in (1, 3) or not (np.isfinite(gm) and gm >= 0.0):
            out["status"][i] = 2
            continue
        dx = x[i] - xa[i]
        H = np.zeros((n, n))
        if ls == 1:
            H[il] = h[i]
            H = H + np.tril(H, -1).T
        C = H + (1.0 + gm) * sa_inv
        try:
            if not np.isfinite(C).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(0.5 * (C + C.T))
        except np.linalg.LinAlgError:
            out["status"][i] = 2 if ls == 1 else 3
            if ls == 3:
                out["x_new"][i] = xa[i] if gm == 0.0 else xa[i] + gm / (1.0 + gm) * dx
            continue
        Li = np.linalg.solve(L, np.eye(n))
        post = Li.T @ Li
        if ls == 3:
            out["status"][i], out["x_new"][i] = 3, (xa[i] if gm == 0.0 else xa[i] + gm / (1.0 + gm) * dx)
            if diagnostics:
                out["chi2"][i], out["dfs"][i], out["post_cov"][i], out["post_var"][i] = 0.0, 0.0, post, np.diag(post)
            continue
        s = np.linalg.solve(L.T, np.linalg.solve(L, g[i] - sa_inv @ dx))
        out["status"][i], out["x_new"][i] = 1, x[i] + s
        if diagnostics:
            e = out["x_new"][i] - xa[i]
            out["chi2"][i] = (rwr[i] - 2.0 * (s @ g[i]) + s @ H @ s) + e @ sa_inv @ e
            out["dfs"][i] = np.sum(post * H)
            out["post_cov"][i], out["post_var"][i] = post, np.diag(post)
    return out


def cost_reference(x, xa, sa_inv, se, y, fx, keep):
    """J over the rows ``keep`` names -> dict of cost, obs, prior [nprof], status and scale = sum_kept r^2 / se +
    |dx|^T |Sa^-1| |dx|, the unit of the bar."""
    y, fx = np.asarray(y, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    nprof, m = y.shape
    x = np.asarray(x, dtype=np.float64).reshape(nprof, -1)
    n = x.shape[1]
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    se = np.broadcast_to(np.asarray(se, dtype=np.float64).reshape(-1, m), (nprof, m))
    keep = np.asarray(keep).astype(bool)
    out = dict(cost=np.full(nprof, np.nan), obs=np.full(nprof, np.nan), prior=np.full(nprof, np.nan),
               status=np.ones(nprof, dtype=np.uint8), scale=np.zeros(nprof))
    for i in range(nprof):
        rows = keep[i]
        if not (np.isfinite(x[i]).all() and np.isfinite(xa[i]).all() and np.isfinite(y[i, rows]).all()
                and np.isfinite(fx[i, rows]).all()):
            out["cost"][i] = out["obs"][i] = out["prior"][i] = np.inf
            continue
        if not (se[i, rows] > 0.0).all():
            out["status"][i] = 2
            continue
        dx, r = x[i] - xa[i], y[i, rows] - fx[i, rows]
        out["obs"][i] = np.sum(r * r / se[i, rows])
        out["prior"][i] = dx @ sa_inv @ dx
        out["cost"][i] = out["obs"][i] + out["prior"][i]
        out["scale"][i] = out["obs"][i] + np.abs(dx) @ np.abs(sa_inv) @ np.abs(dx)
    return out


def solve_errors(got, ref, case):
    """Largest error of every solve output given, in units of its bar's scale (no mask, no floor), over the profiles of
    status 1: x_new of max |x_ref - xa| per block, post_var of max diag Sa per block, post_cov of max |C^-1|, dfs of
    max(1, |ref|), chi2 of max(1, d^T W d) (``ref["dwd"]``; a reference without it: max(1, |ref|))."""
    nprof, nblk, nlev = ref["x_new"].shape
    xa = np.broadcast_to(case["xa"], ref["x_new"].shape)
    dsa = np.diag(case["sa"]).reshape(nblk, nlev)
    err = {key: 0.0 for key in ("x_new", "post_var", "post_cov", "chi2", "dfs") if got.get(key) is not None}
    for i in range(nprof):
        if ref["status"][i] != 1:
            continue
        for b in range(nblk):
            sx = np.abs(ref["x_new"][i, b] - xa[i, b]).max()
            err["x_new"] = max(err["x_new"], float(np.abs(got["x_new"][i, b] - ref["x_new"][i, b]).max() / sx))
            if "post_var" in err:
                e = np.abs(np.reshape(got["post_var"][i], (nblk, nlev))[b] - np.reshape(ref["post_var"][i], (nblk, nlev))[b])
                err["post_var"] = max(err["post_var"], float(e.max() / dsa[b].max()))
        if "post_cov" in err:
            err["post_cov"] = max(err["post_cov"], float(np.abs(got["post_cov"][i] - ref["post_cov"][i]).max()
                                                         / np.abs(ref["post_cov"][i]).max()))
        if "dfs" in err:
            err["dfs"] = max(err["dfs"], float(abs(got["dfs"][i] - ref["dfs"][i]) / max(1.0, abs(ref["dfs"][i]))))
        if "chi2" in err:
            scale = ref["dwd"][i] if "dwd" in ref else abs(ref["chi2"][i])
            err["chi2"] = max(err["chi2"], float(abs(got["chi2"][i] - ref["chi2"][i]) / max(1.0, scale)))
    return err


def prepare_errors(got, lin):
    """Largest error of h (``got["h"]`` packed), g and rwr in units of their bars' scales over the profiles of lin_status
    1: max diag H; sum_i |K_ij w_i r_i| per entry; |rwr|."""
    err = dict(h=0.0, g=0.0, rwr=0.0)
    for i in np.flatnonzero(lin["lin_status"] == 1):
        err["h"] = max(err["h"], float(np.abs(got["h"][i] - tri_pack(lin["h"][i])).max() / lin["h_scale"][i]))
        err["g"] = max(err["g"], float((np.abs(got["g"][i] - lin["g"][i]) / lin["g_scale"][i]).max()))
        err["rwr"] = max(err["rwr"], float(abs(got["rwr"][i] - lin["rwr"][i]) / abs(lin["rwr"][i])))
    return err
