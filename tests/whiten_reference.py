"""NumPy float64 reference of the pre-whitening entries (include/mwrt.h mwrt_obs_whiten_device and
mwrt_obs_whiten_apply_device) and the seeded recipe of a per-profile Se the CPU and GPU tests share.

``whiten_reference`` follows the header's definition literally: the dropped rows are DELETED from Se_p, the rest is
factorised with ``np.linalg.cholesky`` and every output comes from ``solve`` with that factor; the deleted rows are put back
as the header says (NaN in the vectors, 0.0 in the K blocks, rows of the identity in L)."""
import numpy as np

import oe_reference as oer

EPS = np.finfo(np.float64).eps
SE_COND_MAX = 1e2                              # cond_2 of the kept Se_p of the recipe (test_whiten_reference.py checks)
BAR = 1e-9                                     # c m eps cond_2(Se) with c = 64, m <= 140, cond <= 1e2: 2e-10, rounded up
NFACTORS = 6                                   # columns of J in Se_p = (1 + 0.5 p) S0 + J J^T

# (nlev, nblk, m) for the seams of the plan in csrc/mwrt_whiten.hip.h, not for the workload: m = 1; both sides of the row
# block of k_wh_apply (3 | 4 | 5) and a remainder of every length; its load batch (13 | 14 | 15); 32 | 33; the wave of the row
# rule and the first word of the row flags (63 | 64 | 65); the second word and the first raise of both kernels' LDS limit (120 | 121, 127 | 128 | 129); the m limit; a
# level axis of 1, 2, both sides of the column tile (63 | 64 | 65) and three tiles (180); no block (vectors only) to four.
# tests/test_whiten_kernel_resources.py::test_the_shapes_straddle_every_seam holds the list against the header.
SHAPES = [(2, 1, 1), (1, 1, 3), (2, 2, 4), (3, 3, 5), (2, 1, 13), (3, 2, 14), (2, 1, 15), (63, 2, 32), (64, 2, 33), (33, 0, 17),
          (20, 4, 40), (65, 1, 63), (64, 2, 64), (65, 2, 65), (180, 2, 98), (3, 1, 120), (2, 2, 121), (65, 1, 127), (65, 2, 128), (65, 2, 129), (180, 3, 140)]

# Rows dropped at the seams of m = 65 (sixteen row blocks of four and row 64 alone behind them, alone in the second word of
# the row flags): the first row, the last, both neighbours of a block seam and of the word seam, a whole block, every row
# but one, and all of them (status 3).
SEAM_SHAPE = (65, 2, 65)
SEAM_DROPS = {"first": (0,), "last": (64,), "row-3": (3,), "row-4": (4,), "row-63": (63,), "block-4-7": (4, 5, 6, 7),
              "all-but-64": tuple(range(64)), "all": tuple(range(65))}


def nprof_of(shape):
    return 4 if shape[2] <= 65 else 3


def make_se(case_se, m, nprof, seed=oer.SEED):
    """Se_p = (1 + 0.5 p) S0 + J J^T with J = 0.5 sqrt(diag S0) N(0, 1) of shape [m][6], profile p from its own stream; S0
    is the case's ``se`` as a matrix.  -> [nprof][m][m]."""
    s0 = np.diag(case_se) if np.ndim(case_se) == 1 else np.asarray(case_se, dtype=np.float64)
    out = np.empty((nprof, m, m))
    for p in range(nprof):
        rng = np.random.default_rng([seed, 77, m, p])
        j = 0.5 * np.sqrt(np.diag(s0))[:, None] * rng.standard_normal((m, NFACTORS))
        out[p] = (1.0 + 0.5 * p) * s0 + j @ j.T
    return out


def make_case(shape, se_full=True, nprof=None):
    """The case of oe_reference.make_case for the shape (with no K block: one block made and set aside, for its y and
    F), with ``se_p`` [nprof][m][m], or its diagonal [nprof][m] when not ``se_full``."""
    nlev, nblk, m = shape
    nprof = nprof_of(shape) if nprof is None else nprof
    c = oer.make_case(nlev, max(nblk, 1), m, nprof=nprof, se_full=se_full)
    if nblk == 0:
        c["k"] = []
    full = make_se(c["se"], m, nprof)
    c["se_p"] = full if se_full else np.diagonal(full, axis1=1, axis2=2).copy()
    return c


def tri_pack(mat):
    m = mat.shape[0]
    return np.concatenate([mat[i, :i + 1] for i in range(m)])


def tri_unpack(packed, m):
    out = np.zeros((m, m))
    for i in range(m):
        out[i, :i + 1] = packed[i * (i + 1) // 2:i * (i + 1) // 2 + i + 1]
    return out


def row_rule(k, se, y, fx):
    """[nprof][m] bool: the rows each profile keeps."""
    se = np.asarray(se, dtype=np.float64)
    rows = np.isfinite(y) & np.isfinite(fx)
    rows &= np.isfinite(se).all(axis=2) if se.ndim == 3 else np.isfinite(se)
    for b in k:
        rows &= np.isfinite(b).all(axis=2)
    return rows


def whiten_reference(k, se, y, fx):
    """-> dict of l [nprof][m (m + 1) / 2], keep [nprof][m] uint8, status [nprof] uint8, y_out, fx_out [nprof][m], k_out (list
    of [nprof][m][nlev]), cond [nprof] (cond_2 of the kept Se_p; NaN unless status 1) and se_kept (list of the kept
    sub-matrices, None unless status 1)."""
    k = [np.asarray(b, dtype=np.float64) for b in k]
    se, y, fx = (np.asarray(a, dtype=np.float64) for a in (se, y, fx))
    nprof, m = y.shape
    rows = row_rule(k, se, y, fx)
    out = dict(l=np.full((nprof, m * (m + 1) // 2), np.nan), keep=np.zeros((nprof, m), dtype=np.uint8),
               status=np.zeros(nprof, dtype=np.uint8), y_out=np.full((nprof, m), np.nan), fx_out=np.full((nprof, m), np.nan),
               k_out=[np.full(b.shape, np.nan) for b in k], cond=np.full(nprof, np.nan), se_kept=[None] * nprof)
    for p in range(nprof):
        kept = rows[p]
        if not kept.any():
            out["status"][p] = 3
            out["l"][p] = tri_pack(np.eye(m))
            for b in out["k_out"]:
                b[p] = 0.0
            continue
        s = se[p][np.ix_(kept, kept)] if se.ndim == 3 else np.diag(se[p][kept])
        s = np.tril(s) + np.tril(s, -1).T                                   # the lower triangle is what is read
        try:
            lk = np.linalg.cholesky(s)
        except np.linalg.LinAlgError:
            out["status"][p] = 2
            continue
        out["status"][p], out["keep"][p], out["cond"][p], out["se_kept"][p] = 1, kept, np.linalg.cond(s), s
        full = np.eye(m)
        full[np.ix_(kept, kept)] = lk
        out["l"][p] = tri_pack(full)
        out["y_out"][p, kept] = np.linalg.solve(lk, y[p, kept])
        out["fx_out"][p, kept] = np.linalg.solve(lk, fx[p, kept])
        for b, o in zip(k, out["k_out"]):
            o[p] = 0.0
            o[p, kept] = np.linalg.solve(lk, b[p, kept])
    return out


def apply_reference(l, keep, v, mode):
    """L^-1 v (mode 0) or L^-T v (mode 1) on the kept rows of v [nprof][m] or [nprof][m][ncol]; a dropped row is NaN in a
    vector and 0.0 in a block, a profile whose L is NaN is NaN throughout."""
    v = np.asarray(v, dtype=np.float64)
    nprof, m = v.shape[:2]
    out = np.full(v.shape, np.nan)
    for p in range(nprof):
        if np.isnan(l[p][0]):
            continue
        kept = keep[p] != 0
        if v.ndim == 3:
            out[p] = 0.0
        if not kept.any():
            continue
        lk = tri_unpack(l[p], m)[np.ix_(kept, kept)]
        out[p, kept] = np.linalg.solve(lk if mode == 0 else lk.T, v[p, kept])
    return out


def whitened_case(case, ref=None):
    """The case the optimal-estimation references take after whitening: K~, y~, F~ of ``whiten_reference`` and se = ones."""
    ref = whiten_reference(case["k"], case["se_p"], case["y"], case["fx"]) if ref is None else ref
    out = dict(case)
    out.update(k=ref["k_out"], y=ref["y_out"], fx=ref["fx_out"], se=np.ones(case["y"].shape[1]))
    return out


def own_case(case, p):
    """Profile p alone with its own Se_p as the shared se: the yardstick the whitened batch is held against."""
    out = dict(case)
    out.update(k=[b[p:p + 1] for b in case["k"]], x=case["x"][p:p + 1], y=case["y"][p:p + 1], fx=case["fx"][p:p + 1],
               se=case["se_p"][p])
    if np.ndim(case["xa"]) == 3:
        out["xa"] = case["xa"][p:p + 1]
    return out


def column_errors(got, ref):
    """Largest |got - ref| of a vector [nprof][m] or block [nprof][m][ncol] in units of its column's largest |ref| entry,
    over the finite reference entries; the non-finite ones and the exact zeros of dropped rows have to agree exactly."""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin):
        return np.inf
    scale = np.where(fin, np.abs(ref), 0.0).max(axis=1, keepdims=True)
    scale = np.broadcast_to(np.where(scale > 0, scale, 1.0), ref.shape)
    if not fin.any():
        return 0.0
    return float((np.abs(got - ref)[fin] / scale[fin]).max())
