"""NumPy float64 reference of the reduced-basis state map (include/mwrt.h mwrt_basis_project_device and
mwrt_basis_expand_device), its error bar, and the seeded cases and shapes the CPU and GPU tests share.

The bar of the projection, every element, no mask and no floor: |got - ref| <= 2 n 2^-53 S with n = nblk nlev and
S = sum |K||B| -- gamma_n of a dot product of n terms in any order (Higham 2002, eq. 3.5: n u / (1 - n u)), doubled for
the reference's own rounding; where S = 0 the result is exactly 0.  The expansion adds x_ref to a sum of r products: r + 1
terms <= 2 r, so the same bar with n := r holds once x_ref is counted as a term of the sum, S = |x_ref| + sum |B||c|."""
import numpy as np

U = 2.0 ** -53

# (nprof, m, nlev, nblk, r).  What the list reaches is asserted by tests/test_basis_kernel_resources.py::
# test_the_shapes_straddle_every_tile_edge against the tile constants of csrc/mwrt_basis.hip.h as the code has them: both
# sides of the row tile (nprof m = 127 | 128 | 129, and 129 again from three profiles, which is no multiple of the tile),
# of the column tile (r = 31 | 32 | 33, a last tile of width 1 behind two full ones, r = 1) and of the contraction chunk
# (n = 15 | 16 | 17 and 31 | 32 | 33, a chunk that runs from one K block into the next), more than one tile in both grid
# dimensions at once, one to four blocks and the design shape's 98 x 2 x 180.
SHAPES = [(1, 1, 1, 1, 1),
          (3, 14, 15, 1, 31), (3, 14, 16, 1, 32), (3, 14, 17, 1, 33),
          (1, 14, 15, 2, 33),                            # n = 30: chunk 0 ends in block 1, chunk 1 is 14 wide
          (1, 1, 31, 1, 1), (3, 14, 16, 2, 32), (1, 1, 33, 1, 1),
          (1, 127, 16, 1, 32), (1, 128, 16, 1, 32), (1, 129, 16, 1, 32),
          (3, 43, 8, 2, 64),                             # 129 rows from three profiles; two full column tiles
          (1, 98, 180, 2, 32),                           # one profile of the design shape
          (3, 98, 180, 2, 65),                           # three row tiles x three column tiles, the last one column wide
          (1, 140, 17, 4, 33),                           # four blocks, two row tiles, a chunk seam inside every block
          (1, 14, 180, 4, 1)]


def project_reference(k_blocks, b):
    """k_blocks: sequence of [nprof][m][nlev]; b [nblk nlev][r]  ->  (K B [nprof][m][r], S = |K| |B| of the same shape)."""
    k = np.concatenate([np.asarray(x, dtype=np.float64) for x in k_blocks], axis=2)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return k @ b, np.abs(k) @ np.abs(b)


def project_bar(n, scale):
    return 2.0 * n * U * scale


def expand_reference(b, c, x_ref):
    """b [n][r]; c [nprof][r]; x_ref [n] or [nprof][n]  ->  (x_ref + c B^T [nprof][n], S = |x_ref| + |c| |B|^T)."""
    b, c = np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    x_ref = np.broadcast_to(np.asarray(x_ref, dtype=np.float64).reshape(-1, b.shape[0]), (c.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore"):
        return x_ref + c @ b.T, np.abs(x_ref) + np.abs(c) @ np.abs(b).T


def expand_bar(r, scale):
    return 2.0 * r * U * scale


def make_case(nprof, m, nlev, nblk, r, seed=4):
    """Seeded K blocks (amplitudes over nine decades by row, both signs), a basis of both signs and coefficients.  Profile i
    is drawn from its own stream, so it is the same profile whatever nprof is.  The last row of every profile is all zero
    (S = 0 there), and so is column 0 of the basis when r > 1."""
    n = nblk * nlev
    rng = np.random.default_rng([seed, m, nlev, nblk, r, 10 ** 6])
    b = rng.standard_normal((n, r)) * 10.0 ** rng.integers(-3, 2, (1, r))
    if r > 1:
        b[:, 0] = 0.0
    x_ref = 250.0 + 30.0 * rng.standard_normal(n)
    k = [np.empty((nprof, m, nlev)) for _ in range(nblk)]
    c = np.empty((nprof, r))
    for i in range(nprof):
        ri = np.random.default_rng([seed, m, nlev, nblk, r, i])
        for blk in k:
            blk[i] = ri.standard_normal((m, nlev)) * 10.0 ** ri.integers(-6, 3, (m, 1))
            blk[i, m - 1] = 0.0
        c[i] = ri.standard_normal(r) * 10.0 ** ri.integers(-2, 2, r)
    return dict(k=k, b=b, c=c, x_ref=x_ref, shape=(nprof, m, nlev, nblk, r))
