"""np.longdouble reference of the observation selection by information content (include/mwrt.h mwrt_oe_select_device,
DESIGN 4.12), the seeded case recipe and the shapes the CPU and GPU tests share.

It is NOT the incremental form the kernel is specified in: every round recomputes q_i = k_i^T S k_i / se_i of every
candidate directly from the current S, in extended precision, and S itself is carried in extended precision.  K, Sa and the
variances are those of ``nform_reference.make_case``; S0 = Sa.

``select_reference`` is one profile, ``select_batch`` a case.  ``replay`` follows a GIVEN order (the device's) and returns
at each round the reference q of that pick and the largest reference q among the unchosen, so a device order is judged by
what it gave up, whatever the reference's own order is.

Bars (the project's 64x convention on the error of the incremental form in double precision; in a NumPy emulation of that
form against this reference the worst q error was 0.23 (n + nsel) eps b_i and the worst post_cov error 0.08 (n + nsel) eps
max |S0|, at cond(S0) = 1e4):
  q, q_pick   64 (n + nsel) eps b_i,   b_i = |k_i|^T |S0| |k_i| / se_i
  dfs_gain    64 (n + nsel) eps |v|^T |Sa^-1| |v| / d
  post_cov, post_var   64 (n + nsel) eps max |S0|
``select_errors`` returns the device's errors in units of these bars: at most 1.0 passes."""
import numpy as np

import nform_reference as nfr

LD = np.longdouble
EPS = np.finfo(np.float64).eps
MIN_MARGIN = 1e-6                              # (best - runner-up) / best of every round, asserted over SHAPES x profiles
NPROF = 4

# (nlev, nblk, m, nsel): n = nblk nlev <= 128, m unbounded, nsel <= m.  What the list reaches is asserted by
# tests/test_select_kernel_resources.py::test_the_shapes_keep_both_sides_of_every_edge against csrc/mwrt_select.hip.h.
SHAPES = [(1, 1, 5, 5),
          (8, 1, 20, 20),                      # everything picked, m > n
          (12, 2, 224, 24),
          (33, 1, 16, 16),                     # m < n
          (64, 1, 140, 40), (65, 1, 300, 32),  # a lane's second column: n = 64 | 65
          (32, 4, 513, 32),                    # n at the limit in four blocks; m past two row tiles of the other units
          (124, 1, 30, 12), (125, 1, 31, 12)]  # the first raise of the LDS limit: n = 124 | 125


def bar_factor(n, nsel):
    return 64.0 * (n + nsel) * EPS


def make_case(nlev, nblk, m, nprof=NPROF, se_per_profile=False):
    """nform_reference.make_case plus ``s0`` = Sa and ``sa_inv``.  Profile i is its own stream whatever nprof is."""
    case = nfr.make_case(nlev, nblk, m, nprof=nprof, se_per_profile=se_per_profile)
    case["s0"] = case["sa"]
    case["sa_inv"] = nfr.sym_inv(case["sa"])
    return case


def candidates(K, se, keep=None, candidate=None):
    ok = np.isfinite(K).all(axis=1) & np.isfinite(se)
    if keep is not None:
        ok &= np.asarray(keep) != 0
    if candidate is not None:
        ok &= np.asarray(candidate) != 0
    return ok


def _direct_q(K, S, se):
    return np.einsum("ij,ij->i", K @ S, K) / se


def select_reference(K, se, s0, nsel, keep=None, candidate=None, sa_inv=None, follow=None):
    """One profile: K [m][n], se [m], s0 [n][n], optional masks and Sa^-1.  ``follow``: an order to follow instead of the
    argmax (-1 ends it).  Returns a dict: status, count, order [nsel] (-1), q [nsel] (0), dfs_gain [nsel] (0; NaN without
    sa_inv), rank [m], q_left [m], S (longdouble, the last one), b [m] and dfs_bound [nsel] (the bound vectors), best
    [nsel] (the largest q among the unchosen at that round) and margin [nsel] ((best - runner-up) / best; 1 when one
    candidate is left; NaN in unused slots)."""
    K64, se64 = np.asarray(K, dtype=np.float64), np.asarray(se, dtype=np.float64)
    m, n = K64.shape
    out = dict(status=1, count=0, order=np.full(nsel, -1, dtype=np.int32), q=np.zeros(nsel), dfs_gain=np.zeros(nsel),
               rank=np.full(m, -1, dtype=np.int32), q_left=np.zeros(m), S=np.full((n, n), np.nan, dtype=LD), b=np.zeros(m),
               dfs_bound=np.zeros(nsel), best=np.full(nsel, np.nan), margin=np.full(nsel, np.nan))

    def failed(status):
        out.update(status=status, count=0, q=np.full(nsel, np.nan), dfs_gain=np.full(nsel, np.nan),
                   q_left=np.full(m, np.nan), S=np.full((n, n), np.nan, dtype=LD))
        out["order"][:] = -1
        out["rank"][:] = -1
        return out

    if not np.isfinite(s0).all() or (sa_inv is not None and not np.isfinite(sa_inv).all()):
        return failed(0)
    cand = candidates(K64, se64, keep, candidate)
    S = np.tril(np.asarray(s0, dtype=LD))
    S = S + np.tril(S, -1).T
    out["S"] = S
    if not cand.any():
        out["status"] = 3
        return out
    if (se64[cand] <= 0.0).any():
        return failed(2)
    Kc = np.where(cand[:, None], K64, 0.0).astype(LD)          # the select: a row that is no candidate may hold NaN
    sec = np.where(cand, se64, 1.0).astype(LD)
    out["b"] = np.where(cand, np.einsum("ij,ij->i", np.abs(Kc) @ np.abs(S), np.abs(Kc)) / sec, 0.0).astype(np.float64)
    sinv = None if sa_inv is None else np.asarray(sa_inv, dtype=LD)
    if sinv is None:
        out["dfs_gain"][:] = np.nan
    free = cand.copy()
    for t in range(nsel):
        q = np.where(free, _direct_q(Kc, S, sec), -np.inf)
        best = q.max()
        if follow is None:
            if not best > 0:
                break
            j = int(np.argmax(q))                              # the first maximum: the lowest index
        else:
            j = int(follow[t])
            if j < 0:
                break
            assert free[j], "the order names a row twice or one that is no candidate"
        rest = np.delete(q, j)
        runner = rest.max() if free.sum() > 1 else LD(0)
        out["best"][t] = best
        out["margin"][t] = (best - max(runner, LD(0))) / best if best > 0 else np.nan
        v = S @ Kc[j]
        d = sec[j] + Kc[j] @ v
        if not (np.isfinite(np.float64(d)) and d > 0):                 # the verdict is double precision's: d may overflow there
            return failed(2)
        out["order"][t], out["q"][t], out["rank"][j] = j, q[j], t
        if sinv is not None:
            out["dfs_gain"][t] = v @ sinv @ v / d
            out["dfs_bound"][t] = np.abs(v) @ np.abs(sinv) @ np.abs(v) / d
        S = S - np.outer(v, v) / d
        free[j] = False
        out["count"] = t + 1
    out["S"] = S
    left = np.where(free, np.maximum(_direct_q(Kc, S, sec), 0), 0).astype(np.float64)
    chosen = out["rank"] >= 0
    left[chosen] = out["q"][out["rank"][chosen]]
    out["q_left"] = left
    return out


def _profile_inputs(case, i, keep, candidate):
    K = np.concatenate([b[i] for b in case["k"]], axis=1)
    se = case["se"][i] if case["se"].ndim == 2 else case["se"]
    s0 = case["s0"][i] if case["s0"].ndim == 3 else case["s0"]
    return K, se, s0, None if keep is None else keep[i], candidate


def select_batch(case, nsel, keep=None, candidate=None, dfs=True, follow=None):
    """A case of ``make_case`` (or one edited by a test) -> the list of its profiles' ``select_reference`` results."""
    nprof = case["k"][0].shape[0]
    res = []
    for i in range(nprof):
        K, se, s0, kp, cd = _profile_inputs(case, i, keep, candidate)
        with np.errstate(over="ignore", invalid="ignore"):       # a test's overflowing row, on its way to status 2
            res.append(select_reference(K, se, s0, nsel, kp, cd, case["sa_inv"] if dfs else None,
                                        None if follow is None else follow[i]))
    return res


def replay(case, i, order, greedy=None, keep=None, candidate=None, dfs=True):
    """Profile i of ``case`` along the given ``order``.  ``greedy``: that profile's own ``select_reference`` result, handed
    back when the order is the same (the replay would repeat it step by step)."""
    order = np.asarray(order)
    if greedy is not None and np.array_equal(order, greedy["order"]):
        return greedy
    K, se, s0, kp, cd = _profile_inputs(case, i, keep, candidate)
    return select_reference(K, se, s0, len(order), kp, cd, case["sa_inv"] if dfs else None, follow=order)


def select_errors(got, ref, n, s0):
    """Largest error of one profile's device outputs in units of the bars (no mask, no floor).  ``got``: q_pick, q,
    dfs_gain, post_cov, post_var; ``ref``: the replay of the device's order."""
    nsel = len(ref["order"])
    f = bar_factor(n, nsel)
    picked = ref["order"] >= 0
    b_pick = ref["b"][ref["order"][picked]]
    err = dict(q_pick=0.0, q=0.0, dfs_gain=0.0, post_cov=0.0, post_var=0.0)

    def ratio(diff, scale):
        diff, scale = np.abs(np.asarray(diff, dtype=np.float64)), np.asarray(scale, dtype=np.float64) * f
        both_zero = (diff == 0.0) & (scale == 0.0)
        return float(np.max(np.where(both_zero, 0.0, diff / np.where(both_zero, 1.0, scale)), initial=0.0))

    err["q_pick"] = max(ratio(got["q_pick"][picked] - ref["q"][picked], b_pick), ratio(got["q_pick"][~picked], 0.0))
    err["q"] = ratio(got["q"] - ref["q_left"], ref["b"])
    if "dfs_gain" in got and not np.isnan(ref["dfs_gain"]).any():
        err["dfs_gain"] = ratio(got["dfs_gain"] - ref["dfs_gain"], ref["dfs_bound"])
    smax = np.abs(s0).max()
    S = ref["S"]
    if "post_cov" in got:
        err["post_cov"] = ratio((got["post_cov"].astype(LD) - S).astype(np.float64), smax)
    if "post_var" in got:
        err["post_var"] = ratio((got["post_var"].reshape(-1).astype(LD) - np.diag(S)).astype(np.float64), smax)
    return err


_cases = {}


def seeded(nlev, nblk, m, nsel, se_pp=False, nprof=NPROF):
    """The case and its greedy reference, computed once per shape and variant; nobody writes to either."""
    key = (nlev, nblk, m, nsel, se_pp, nprof)
    if key not in _cases:
        case = make_case(nlev, nblk, m, nprof=nprof, se_per_profile=se_pp)
        _cases[key] = (case, select_batch(case, nsel))
    return _cases[key]
