"""A 50-digit reference of the solves of the optimal-estimation family (include/mwrt.h mwrt_oe_step_device,
mwrt_oe_lm_solve_device, mwrt_oe_gain_device, mwrt_oe_nform_prepare_device / _solve_device, mwrt_obs_whiten_device; DESIGN
4.6, 4.10, 4.11), the conditioning ladder the CPU and GPU tests share, and the yardstick their bars come from.

``decimal`` at DIGITS significant digits on NumPy object arrays, the way tests/math_reference.py works.  The float64 inputs
handed to a kernel are the exact inputs (``Decimal(float)`` is exact; the n-form takes ``sa_inv`` as given, not Sa), the
header's definition is followed literally as the float64 references do, and every output is rounded to the nearest float64
once, at the end.  The ladder uses finite inputs only, so no row is ever dropped and the row rule is not restated here.

Each reference also returns cond_2 of what it factors -- G for the m-form, the Jacobi-scaled C for the n-form, Se_p for the
whitening -- taken in float64 from the exactly formed, once-rounded matrix (good to eps cond relative: 1e-5 at cond 1e11).

The ladder.  One lever per family drives cond_2 from <= 1e4 to 1e9 .. 1e11 in steps no wider than 1e3:
  m-form     oe_reference.make_case with se *= 10^-k, one shape per k_oe_step<MR>, MR = ceil(m / 32) = 1 .. 5, the two
             widest with a short level axis (K Sa K^T of rank n = 40 < m: G is Se plus a rank-deficient term); diagonal
             and full Se alternate over the shapes.
  n-form     nform_reference.make_case with the same lever, on shapes with m < n (H rank deficient: the Jacobi-scaled C climbs
             with 1 / se; with m >= n it saturates at 3e6 .. 2e7 and there is no ladder), n = 64 | 65, 127 and 128 in four blocks.
  whitening  Se_p = S0 + a^2 J J^T of whiten_reference.make_se's S0 and J, a = 10^(j/2): shapes on both sides of the first
             LDS raise of k_wh_apply (m = 120 | 121) and of k_wh_factor (127 | 128), and one with no K block.
test_oe_exact_reference.py asserts those conditions on every rung from the references alone.

The bar of an output in a case is  max(8 c_out eps cond_case, 64 (m + n) eps)  in the unit the family already uses
(oe_reference.block_errors, oe_char_reference.char_errors, nform_reference.solve_errors, whiten_reference.column_errors):
c_out is the float64 NumPy reference's own error against the exact one over eps cond, maximised over all cases of the
family's ladder -- LAPACK's Cholesky is the yardstick of "backward stable", pooled because c varies by more than a decade
between cases; 8 covers two stable algorithms with different sum orders (fixed trees with fma on the device, blocked
LAPACK in NumPy); the floor is the project's dot-product bar, for outputs whose error does not grow with cond (chi2 of
the n-form in its unit d^T W d among them).  Nothing in a bar comes from the device."""
import decimal
import functools
from decimal import Decimal

import numpy as np
import threadpoolctl

import nform_reference as nfr
import oe_char_reference as ocr
import oe_lm_reference as lmr
import oe_reference as oer
import whiten_reference as whr

DIGITS = 50
EPS = float(np.finfo(np.float64).eps)
NPROF = 2
FACTOR = 8.0                                    # two stable algorithms, different sum orders
COND_BOTTOM, COND_TOP, GAP_MAX = 1e4, (1e9, 1e11), 1e3

_to_dec = np.frompyfunc(Decimal, 1, 1)


def one_blas_thread():
    """The yardstick runs on one BLAS thread: how a threaded gemm or potrf splits its sums depends on the thread count, and
    with it the last bits of the float64 reference -- c_out of the n-form's x_new at n = 128 came out as 1.8, 2.6 and 2.9 with
    8, 16 and 1 threads.  One thread makes the pooled constants the same wherever the same BLAS kernels run."""
    return threadpoolctl.threadpool_limits(limits=1, user_api="blas")


def dec(a):
    """float64 array -> object array of the same values, exactly."""
    return _to_dec(np.asarray(a, dtype=np.float64))


def f64(a):
    """Object array (or Decimal) -> nearest float64."""
    return np.asarray(a, dtype=object).astype(np.float64)


def _zeros(*shape):
    out = np.empty(shape, dtype=object)
    out[...] = Decimal(0)
    return out


def _eye(n):
    out = _zeros(n, n)
    for i in range(n):
        out[i, i] = Decimal(1)
    return out


def cholesky(a):
    """Lower factor of a symmetric positive-definite object matrix (the lower triangle is read)."""
    n = a.shape[0]
    l = _zeros(n, n)
    for j in range(n):
        s = a[j, j] - (l[j, :j] @ l[j, :j] if j else 0)
        if not s > 0:
            raise np.linalg.LinAlgError("not positive definite at digits = %d" % decimal.getcontext().prec)
        l[j, j] = s.sqrt()
        if j + 1 < n:
            l[j + 1:, j] = (a[j + 1:, j] - (l[j + 1:, :j] @ l[j, :j] if j else 0)) / l[j, j]
    return l


def solve_lower(l, b):
    """L^-1 b for b [n] or [n][cols]."""
    x = np.array(b, dtype=object)
    for i in range(l.shape[0]):
        if i:
            x[i] = x[i] - l[i, :i] @ x[:i]
        x[i] = x[i] / l[i, i]
    return x


def solve_upper(l, b):
    """L^-T b."""
    n = l.shape[0]
    x = np.array(b, dtype=object)
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            x[i] = x[i] - l[i + 1:, i] @ x[i + 1:]
        x[i] = x[i] / l[i, i]
    return x


def _cond(mat):
    return float(np.linalg.cond(f64(mat)))


def _unpack(k, x, xa):
    kb = [np.asarray(b, dtype=np.float64) for b in k]
    nblk = len(kb)
    nprof, m, nlev = kb[0].shape
    n = nblk * nlev
    x = np.asarray(x, dtype=np.float64).reshape(nprof, n)
    xa = np.broadcast_to(np.asarray(xa, dtype=np.float64).reshape(-1, n), (nprof, n))
    return kb, nblk, nprof, m, nlev, n, x, xa


def mform_exact(k, x, xa, sa, se, y, fx, gamma=None, gain=False, digits=DIGITS, keep_exact=False):
    """The m-form step of a batch of finite inputs: G_gamma = K Sa K^T + (1 + gamma) Se, Se [m] or [m][m]; gamma None (the
    step entry, with dfs and post_var) or one value per profile (the damped solve: x_new and chi2, the rest NaN).
    -> dict of x_new [nprof][nblk][nlev], status, nobs, chi2, dfs, post_var, cond; with ``gain`` also the outputs of
    mwrt_oe_gain_device under the keys of oe_char_reference (gain, ksa, keep, avk_diag, dfs_block, noise_var, smooth_var,
    bound_diag); with ``keep_exact`` the unrounded G, d and u of every profile under "exact"."""
    kb, nblk, nprof, m, nlev, n, x, xa = _unpack(k, x, xa)
    damped = gamma is not None
    gam = np.broadcast_to(np.asarray(0.0 if gamma is None else gamma, dtype=np.float64), (nprof,))
    nan = lambda *shape: np.full(shape, np.nan)   # noqa: E731
    out = dict(x_new=nan(nprof, n), status=np.ones(nprof, dtype=np.uint8), nobs=np.full(nprof, m, dtype=np.int32),
               chi2=nan(nprof), dfs=nan(nprof), post_var=nan(nprof, n), cond=nan(nprof), exact=[])
    if gain:
        out.update(gain=nan(nprof, m, n), ksa=nan(nprof, m, n), keep=np.ones((nprof, m), dtype=np.uint8), avk_diag=nan(nprof, n),
                   dfs_block=nan(nprof, nblk), noise_var=nan(nprof, n), smooth_var=nan(nprof, n), bound_diag=nan(nprof, n))
    with decimal.localcontext() as c:
        c.prec = digits
        sa_d, se_d = dec(sa), dec(se)
        S = se_d if se_d.ndim == 2 else None
        for i in range(nprof):
            K = dec(np.concatenate([b[i] for b in kb], axis=1))
            g1 = 1 + Decimal(float(gam[i]))
            dx = dec(x[i]) - dec(xa[i])
            r = dec(y[i]) - dec(fx[i])
            kdx = K @ dx
            d = r + kdx / g1
            W = K @ sa_d
            G = W @ K.T
            if S is None:
                for j in range(m):
                    G[j, j] = G[j, j] + g1 * se_d[j]
            else:
                G = G + g1 * S
            L = cholesky(G)
            zv = solve_lower(L, d)
            u = solve_upper(L, zv)
            out["x_new"][i] = f64(dec(xa[i]) + (g1 - 1) / g1 * dx + W.T @ u)
            out["chi2"][i] = float(zv @ zv)
            out["cond"][i] = _cond(G)
            if keep_exact:
                out["exact"].append(dict(G=G, d=d, u=u))
            if damped:
                continue
            Z = solve_lower(L, W)
            Li = solve_lower(L, _eye(m))
            if S is None:
                tr = ((Li * Li).sum(axis=0) * se_d).sum()
            else:
                tr = ((Li @ S) * Li).sum()
            out["dfs"][i] = float(m - tr)
            pv = np.diagonal(sa_d) - (Z * Z).sum(axis=0)
            out["post_var"][i] = f64(pv)
            if gain:
                g = solve_upper(L, Z)                                       # G^-1 K Sa = gain^T
                avk = (g * K).sum(axis=0)
                noise = ((S @ g) * g).sum(axis=0) if S is not None else ((g * g) * se_d[:, None]).sum(axis=0)
                out["gain"][i], out["ksa"][i] = f64(g), f64(W)
                out["avk_diag"][i], out["noise_var"][i], out["smooth_var"][i] = f64(avk), f64(noise), f64(pv - noise)
                out["bound_diag"][i] = f64((abs(g) * abs(K)).sum(axis=0))
                out["dfs_block"][i] = f64(avk.reshape(nblk, nlev).sum(axis=1))
    for key in ("x_new", "post_var") + (("avk_diag", "noise_var", "smooth_var") if gain else ()):
        out[key] = out[key].reshape(nprof, nblk, nlev)
    if not keep_exact:
        del out["exact"]
    return out


def nform_exact(k, x, xa, sa_inv, se, y, fx, gamma=None, digits=DIGITS):
    """The n-form of a batch of finite inputs: H = K^T W K, g = K^T W r and r^T W r formed exactly from K (W = diag 1 / se,
    se [m] or [nprof][m]), C = H + (1 + gamma) Sa^-1 with ``sa_inv`` as given.  gamma None: every output; else x_new alone.
    -> dict of h [nprof][n][n], g, rwr, x_new [nprof][nblk][nlev], status, nobs, chi2, dfs, post_var, post_cov, cond (cond_2
    of the Jacobi-scaled C) and dwd, the keys of nform_reference.solve_reference and prepare_reference."""
    kb, nblk, nprof, m, nlev, n, x, xa = _unpack(k, x, xa)
    se = np.broadcast_to(np.asarray(se, dtype=np.float64).reshape(-1, m), (nprof, m))
    damped = gamma is not None
    gam = np.broadcast_to(np.asarray(0.0 if gamma is None else gamma, dtype=np.float64), (nprof,))
    nan = lambda *shape: np.full(shape, np.nan)   # noqa: E731
    out = dict(h=nan(nprof, n, n), g=nan(nprof, n), rwr=nan(nprof), x_new=nan(nprof, n), status=np.ones(nprof, dtype=np.uint8),
               nobs=np.full(nprof, m, dtype=np.int32), lin_status=np.ones(nprof, dtype=np.uint8),
               keep=np.ones((nprof, m), dtype=np.uint8), chi2=nan(nprof), dfs=nan(nprof), post_var=nan(nprof, n),
               post_cov=nan(nprof, n, n), cond=nan(nprof), dwd=nan(nprof), h_scale=nan(nprof), g_scale=nan(nprof, n))
    with decimal.localcontext() as c:
        c.prec = digits
        sai = dec(sa_inv)
        for i in range(nprof):
            K = dec(np.concatenate([b[i] for b in kb], axis=1))
            w = 1 / dec(se[i])
            g1 = 1 + Decimal(float(gam[i]))
            dx = dec(x[i]) - dec(xa[i])
            r = dec(y[i]) - dec(fx[i])
            WK = K * w[:, None]
            H = K.T @ WK
            g = WK.T @ r
            out["h"][i], out["g"][i], out["rwr"][i] = f64(H), f64(g), float(r @ (w * r))
            out["h_scale"][i] = float(max(np.diagonal(H)))
            out["g_scale"][i] = f64(abs(WK * r[:, None]).sum(axis=0))
            C = H + g1 * sai
            L = cholesky(C)
            s = solve_upper(L, solve_lower(L, g - sai @ dx))
            out["x_new"][i] = f64(dec(x[i]) + s)
            scale = np.array([1 / v.sqrt() for v in np.diagonal(C)], dtype=object)
            out["cond"][i] = _cond(C * scale[:, None] * scale[None, :])
            if damped:
                continue
            Li = solve_lower(L, _eye(n))
            post = Li.T @ Li
            lin_res = r - K @ s
            e = dx + s
            d = r + K @ dx
            out["chi2"][i] = float(lin_res @ (w * lin_res) + e @ (sai @ e))
            out["dfs"][i] = float((post * H).sum())
            out["post_cov"][i], out["post_var"][i] = f64(post), f64(np.diagonal(post))
            out["dwd"][i] = float(d @ (w * d))
    out["x_new"] = out["x_new"].reshape(nprof, nblk, nlev)
    out["post_var"] = out["post_var"].reshape(nprof, nblk, nlev)
    return out


def whiten_exact(k, se, y, fx, digits=DIGITS):
    """The whitening of a batch of finite inputs with a full Se_p [nprof][m][m] (its lower triangle is what is read): L and
    L^-1 applied to y, F and the K blocks, under the keys of whiten_reference.whiten_reference."""
    kb = [np.asarray(b, dtype=np.float64) for b in k]
    se, y, fx = (np.asarray(a, dtype=np.float64) for a in (se, y, fx))
    nprof, m = y.shape
    out = dict(l=np.full((nprof, m * (m + 1) // 2), np.nan), keep=np.ones((nprof, m), dtype=np.uint8),
               status=np.ones(nprof, dtype=np.uint8), y_out=np.full((nprof, m), np.nan), fx_out=np.full((nprof, m), np.nan),
               k_out=[np.full(b.shape, np.nan) for b in kb], cond=np.full(nprof, np.nan), se_kept=[None] * nprof)
    with decimal.localcontext() as c:
        c.prec = digits
        for p in range(nprof):
            s64 = np.tril(se[p]) + np.tril(se[p], -1).T
            L = cholesky(dec(s64))
            rhs = np.concatenate([dec(y[p])[:, None], dec(fx[p])[:, None]] + [dec(b[p]) for b in kb], axis=1)
            sol = f64(solve_lower(L, rhs))
            out["l"][p] = whr.tri_pack(f64(L))
            out["y_out"][p], out["fx_out"][p] = sol[:, 0], sol[:, 1]
            col = 2
            for o in out["k_out"]:
                o[p] = sol[:, col:col + o.shape[2]]
                col += o.shape[2]
            out["cond"][p], out["se_kept"][p] = float(np.linalg.cond(s64)), s64
    return out


# ---- the ladder ----
# (nlev, nblk, m), se_full, rungs k of se *= 10^-k.  MR = ceil(m / 32) = 1 .. 5 in this order.
MFORM_LADDER = [((12, 1, 31), False, (0, 2, 4, 6, 8, 10)),
                ((33, 1, 33), True, (0, 2, 4, 6, 8, 10)),
                ((65, 2, 65), False, (0, 2, 4, 6, 8)),
                ((20, 2, 98), True, (0, 2, 4, 6, 7)),
                ((20, 2, 140), False, (0, 2, 4, 6, 7))]
MFORM_DAMPED = ((33, 1, 33), True, 8, 0.5)      # one rung through mwrt_oe_lm_*: shape, se_full, k, gamma
MFORM_GAIN_SHAPE = (33, 1, 33)                  # the shape whose rungs also go through mwrt_oe_gain_device
NFORM_LADDER = [((32, 4, 98), (0, 2, 4, 6, 8)),                 # n = 128 in four blocks
                ((64, 1, 33), (0, 4, 6, 8, 10, 12)),            # a lane's second column of K: n = 64 | 65
                ((65, 1, 40), (0, 4, 6, 8, 10, 12)),
                ((127, 1, 98), (0, 4, 6, 8, 10, 12))]
NFORM_DAMPED = ((32, 4, 98), 8, 0.5)
WHITEN_LADDER = [((33, 0, 17), tuple(range(0, 10))),
                 ((3, 1, 120), tuple(range(0, 10))),
                 ((2, 2, 121), tuple(range(0, 10))),
                 ((2, 1, 127), tuple(range(0, 10))),
                 ((2, 2, 128), tuple(range(0, 10)))]


def mform_cases():
    """-> list of (shape, se_full, k, gamma or None), the damped rung last."""
    out = [(shape, se_full, k, None) for shape, se_full, rungs in MFORM_LADDER for k in rungs]
    return out + [MFORM_DAMPED]


def nform_cases():
    out = [(shape, k, None) for shape, rungs in NFORM_LADDER for k in rungs]
    return out + [NFORM_DAMPED]


def whiten_cases():
    return [(shape, j) for shape, rungs in WHITEN_LADDER for j in rungs]


def case_id(key):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else ("full" if p is True else "diag" if p is False else
                                                                         "g0" if p is None else str(p)) for p in key)


def mform_case(shape, se_full, k):
    case = oer.make_case(*shape, nprof=NPROF, se_full=se_full)
    case["se"] = case["se"] * 10.0 ** -k
    return case


def nform_case(shape, k):
    """... with ``sa_inv``, the symmetrised inverse of Sa the kernel is handed, taken on one BLAS thread (one_blas_thread)."""
    case = nfr.make_case(*shape, nprof=NPROF)
    case["se"] = case["se"] * 10.0 ** -k
    with one_blas_thread():
        inv = np.linalg.inv(case["sa"])
    case["sa_inv"] = 0.5 * (inv + inv.T)
    return case


def whiten_case(shape, j):
    """whiten_reference.make_case with Se_p = S0 + a^2 J J^T, a = 10^(j/2); S0 and J are those of make_se (profile p from its
    own stream, without make_se's factor 1 + 0.5 p on S0)."""
    nlev, nblk, m = shape
    case = whr.make_case(shape, se_full=True, nprof=NPROF)
    s0 = np.asarray(case["se"], dtype=np.float64)
    a2 = 10.0 ** j
    for p in range(NPROF):
        rng = np.random.default_rng([oer.SEED, 77, m, p])
        jm = 0.5 * np.sqrt(np.diag(s0))[:, None] * rng.standard_normal((m, whr.NFACTORS))
        case["se_p"][p] = s0 + a2 * (jm @ jm.T)
    return case


# ---- the yardstick: NumPy float64 against the exact reference, per case and per profile ----
MFORM_OUT = ("x_new", "chi2", "dfs", "post_var")
GAIN_OUT = ("gain", "ksa", "avk_diag", "dfs_block", "noise_var", "smooth_var")
NFORM_OUT = ("x_new", "chi2", "dfs", "post_var", "post_cov")
WHITEN_OUT = ("l", "y", "fx", "k")
_IN = ("k", "x", "xa", "sa", "se", "y", "fx")


def one(outputs, i):
    """Profile i of a dict of per-profile outputs as a batch of one (lists of blocks included)."""
    return {key: (None if v is None else [b[i:i + 1] for b in v] if isinstance(v, list) else v[i:i + 1])
            for key, v in outputs.items() if key != "exact"}


def one_case(case, i):
    out = dict(case)
    out.update(k=[b[i:i + 1] for b in case["k"]], x=case["x"][i:i + 1], y=case["y"][i:i + 1], fx=case["fx"][i:i + 1])
    if np.ndim(case["xa"]) == 3:
        out["xa"] = case["xa"][i:i + 1]
    if "se_p" in case:
        out["se_p"] = case["se_p"][i:i + 1]
    return out


def mform_errors(got, ref, case, keys=MFORM_OUT):
    """Per profile: dict of the errors of ``keys`` in the units of oe_reference.block_errors."""
    return [{key: v for key, v in oer.block_errors(one({q: got.get(q) for q in keys}, i), one(ref, i), one_case(case, i)).items()
             if key in keys} for i in range(NPROF)]


def gain_errors(got, ref, case):
    return [ocr.char_errors(one({q: got[q] for q in GAIN_OUT}, i), one(ref, i), one_case(case, i)) for i in range(NPROF)]


def nform_errors(got, ref, case, keys=NFORM_OUT):
    return [nfr.solve_errors(one({q: got[q] for q in keys}, i), one(ref, i), one_case(case, i)) for i in range(NPROF)]


def whiten_errors(got, ref):
    """Per profile: L in units of its largest entry, y~, F~ and the K~ blocks in those of whiten_reference.column_errors."""
    out = []
    for p in range(NPROF):
        e = dict(l=float(np.abs(got["l"][p] - ref["l"][p]).max() / np.abs(ref["l"][p]).max()),
                 y=whr.column_errors(got["y_out"][p:p + 1], ref["y_out"][p:p + 1]),
                 fx=whr.column_errors(got["fx_out"][p:p + 1], ref["fx_out"][p:p + 1]))
        if got["k_out"]:
            e["k"] = max(whr.column_errors(g[p:p + 1], r[p:p + 1]) for g, r in zip(got["k_out"], ref["k_out"]))
        out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def mform_entry(key):
    """-> dict of case, exact, numpy (the float64 reference's outputs), cond [NPROF] and err (the yardstick's error per
    profile and output) for one case of mform_cases()."""
    shape, se_full, k, gamma = key
    case = mform_case(shape, se_full, k)
    ins = {q: case[q] for q in _IN}
    with_gain = gamma is None and shape == MFORM_GAIN_SHAPE
    exact = mform_exact(**ins, gamma=None if gamma is None else np.full(NPROF, gamma), gain=with_gain)
    with one_blas_thread():
        ref = oer.oe_step_reference(**ins) if gamma is None else lmr.solve_reference(**ins, gamma=np.full(NPROF, gamma))
        ref_gain = ocr.oe_char_reference(**ins, products=False) if with_gain else None
    err = mform_errors(ref, exact, case, keys=MFORM_OUT if gamma is None else ("x_new",))
    if with_gain:
        for e, g in zip(err, gain_errors(ref_gain, exact, case)):
            e.update(g)
    return dict(case=case, exact=exact, numpy=ref, cond=exact["cond"], err=err, m=shape[2], n=shape[0] * shape[1])


@functools.lru_cache(maxsize=None)
def nform_entry(key):
    shape, k, gamma = key
    case = nform_case(shape, k)
    ins = {q: case[q] for q in nfd_keys()}
    sa_inv = case["sa_inv"]
    gam = None if gamma is None else np.full(NPROF, gamma)
    exact = nform_exact(sa_inv=sa_inv, gamma=gam, **ins)
    with one_blas_thread():
        ref = nfr.solve_reference(sa_inv=sa_inv, gamma=gam, **ins)
    err = nform_errors(ref, exact, case, keys=NFORM_OUT if gamma is None else ("x_new",))
    return dict(case=case, exact=exact, numpy=ref, cond=exact["cond"], err=err, m=shape[2], n=shape[0] * shape[1])


def nfd_keys():
    return ("k", "x", "xa", "se", "y", "fx")


@functools.lru_cache(maxsize=None)
def whiten_entry(key):
    shape, j = key
    case = whiten_case(shape, j)
    exact = whiten_exact(case["k"], case["se_p"], case["y"], case["fx"])
    with one_blas_thread():
        ref = whr.whiten_reference(case["k"], case["se_p"], case["y"], case["fx"])
    return dict(case=case, exact=exact, numpy=ref, cond=exact["cond"], err=whiten_errors(ref, exact), m=shape[2],
                n=shape[0] * shape[1])


FAMILIES = {"mform": (mform_cases, mform_entry), "nform": (nform_cases, nform_entry), "whiten": (whiten_cases, whiten_entry)}


@functools.lru_cache(maxsize=None)
def pooled(family):
    """c_out of every output of a family: the yardstick's error over eps cond, maximised over the ladder's cases and
    profiles.  Computes (and caches) every case of the family."""
    cases, entry = FAMILIES[family]
    c = {}
    for key in cases():
        e = entry(key)
        for i in range(NPROF):
            for out, v in e["err"][i].items():
                c[out] = max(c.get(out, 0.0), v / (EPS * e["cond"][i]))
    return c


def bar(family, key, out, i):
    """The bar of output ``out`` of profile i of a case: max(8 c_out eps cond, 64 (m + n) eps)."""
    e = FAMILIES[family][1](key)
    return max(FACTOR * pooled(family)[out] * EPS * e["cond"][i], 64 * (e["m"] + e["n"]) * EPS)


# ---- a change of units: D on the state, E on the observation rows, both diagonal powers of two ----
def unit_exponents(nblk, nlev, m, seed=7, lo=-40, hi=40):
    """-> (D [nblk nlev], E [m]): 2^e with e in [lo, hi], one draw per block plus one per element (clipped to the range),
    one per row."""
    rng = np.random.default_rng([oer.SEED, seed, nblk, nlev, m])
    e_state = np.clip(rng.integers(lo, hi + 1, size=(nblk, 1)) + rng.integers(-8, 9, size=(nblk, nlev)), lo, hi)
    e_rows = rng.integers(lo, hi + 1, size=m)
    return np.ldexp(1.0, e_state.ravel()), np.ldexp(1.0, e_rows)


def rescale_case(case, D, E, se_full):
    """The same problem in other units: K -> E K D^-1, x, xa -> D x, D xa, Sa -> D Sa D, y, F -> E y, E F, Se -> E Se E
    (``se_full``: se is [m][m]; else variances [m] or [nprof][m], times E^2), se_p likewise; a ``sa_inv`` in the case goes to
    D^-1 Sa^-1 D^-1.  Every factor is a power of two, so every entry is exact."""
    nblk, nlev = len(case["k"]), (case["k"][0].shape[2] if case["k"] else 0)
    Db = D.reshape(nblk, nlev) if nblk else D
    out = dict(case)
    out["k"] = [b * E[None, :, None] / Db[i][None, None, :] for i, b in enumerate(case["k"])]
    out["y"], out["fx"] = case["y"] * E, case["fx"] * E
    if nblk:
        out["x"], out["xa"] = case["x"] * Db, case["xa"] * Db
        out["sa"] = case["sa"] * D[:, None] * D[None, :]
        if "sa_inv" in case:
            out["sa_inv"] = case["sa_inv"] / D[:, None] / D[None, :]
    se = np.asarray(case["se"])
    out["se"] = se * E[:, None] * E[None, :] if se_full else se * E * E
    if "se_p" in case:
        sp = case["se_p"]
        out["se_p"] = sp * E[:, None] * E[None, :] if sp.ndim == 3 else sp * E * E
    return out


def rescale_outputs(out, D, E, inverse=False):
    """What the outputs of the original problem become in the units of rescale_case (``inverse``: back again), exactly:
    x_new times D; post_var, noise_var and smooth_var times D^2; post_cov D_i D_j; gain D_j / E_i; ksa E_i D_j; h (packed or
    full) and g divided by D_i D_j and D; L (packed) times E_i by row; the whitened K blocks divided by D.  chi2, dfs, the
    costs, the whitened vectors, avk_diag, dfs_block and every count, flag and status stay as they are."""
    n, m = D.size, E.size
    if inverse:
        D, E = 1.0 / D, 1.0 / E
    res = dict(out)
    for key, v in out.items():
        if v is None:
            continue
        if key == "x_new":
            res[key] = (v.reshape(len(v), n) * D).reshape(v.shape)
        elif key in ("post_var", "noise_var", "smooth_var"):
            res[key] = (v.reshape(len(v), n) * D * D).reshape(v.shape)
        elif key == "post_cov":
            res[key] = v * D[:, None] * D[None, :]
        elif key == "gain":
            res[key] = v * D[None, None, :] / E[None, :, None]
        elif key == "ksa":
            res[key] = v * D[None, None, :] * E[None, :, None]
        elif key == "g":
            res[key] = v / D
        elif key == "h":
            i, j = np.tril_indices(n)
            res[key] = v / D[:, None] / D[None, :] if v.ndim == 3 else v / D[i] / D[j]
        elif key == "l":
            i, _ = np.tril_indices(m)
            res[key] = v * E[i]
        elif key == "k_out":
            nlev = v[0].shape[2] if v else 0
            res[key] = [b / D[q * nlev:(q + 1) * nlev] for q, b in enumerate(v)]
    return res
