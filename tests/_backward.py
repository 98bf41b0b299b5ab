"""Host-side evaluation of backward errors of the dense path's stages (test
infrastructure; numpy and scipy only, no device).

A backward-error test is only as good as the arithmetic that evaluates the residual: a
float64 BLAS product has the error of the thing being measured, and a numpy.longdouble
matmul of n = 2100 takes minutes. exact_product splits each operand into 20-bit slices
whose products float64 BLAS forms without rounding, and sums them in longdouble.

Here u = 2^-53, |.| is entrywise, and every residual is in longdouble:
  omega_chol(A, L)        max_ij |A - L L^T|_ij / (|L| |L^T|)_ij                 full matrix
  omega_inv(L, W)         min over the two products W^T L and L W^T of
                          max_ij |P - I|_ij / (|.| |.|)_ij                  lower triangle
  omega_gram(W, T)        max_ij |T - W W^T|_ij / (|W| |W^T|)_ij               full matrix
  omega_solve(A, L, x, b) max_i |b - A x|_i / ((|L| |L^T|) |x|)_i
Each has a `tiles=True` form that also returns the per-128-tile maxima of the ratio, so
that a failure names the tile.

blocked_reference restates the device's *algorithm* (right-looking blocked Cholesky on
128-tiles whose panel step multiplies by the explicit inverse of the diagonal tile, and
the blocked W = L^-T from the same inverses) in plain float64 numpy: the reference the
device's backward error is measured against.
"""

import numpy
import scipy.linalg

U = 2.0 ** -53
TS = 128
BITS = 20
LD = numpy.longdouble


def _split_rows(A, slices):
    """A = S_1 + ... + S_slices + R exactly, row by row: with 2^e_i > max_j |A_ij|,
    S_p holds integer multiples, of magnitude <= 2^BITS, of 2^(e_i - p BITS).
    -> ([S_1, ...], [R_0 = A, R_1, ..., R_slices]) with R_p = A - S_1 - ... - S_p."""
    A = numpy.asarray(A, dtype=numpy.float64)
    amax = numpy.max(numpy.abs(A), axis=1, initial=0.0)
    e = numpy.frexp(numpy.where(amax > 0, amax, 1.0))[1].astype(numpy.float64)
    S, R = [], [A]
    for p in range(1, slices + 1):
        unit = numpy.exp2(e - p * BITS)[:, None]
        s = numpy.rint(R[-1] / unit) * unit
        S.append(s)
        R.append(R[-1] - s)       # exact: both are multiples of ulp(R), |R - s| <= unit / 2
    return S, R


def exact_product(A, B, slices=3):
    """A @ B as longdouble, far below u |A| |B|.

    A is split by rows, B by columns, into `slices` slices of BITS bits and a remainder.
    A product of two slices is, per entry, a power of two times a sum of k <= 8192 integer
    products below 2^40, which float64 holds exactly in any order: BLAS forms it without
    rounding. These are taken for every pair of slice levels p + q <= slices + 1; what is
    left of B after those (its remainder R_{slices + 1 - p}) meets S_p in one rounded
    float64 product of relative size 2^(-BITS slices), whose rounding error
    k u 2^(-BITS slices) |A| |B| does not matter, and so does A's remainder times B."""
    A = numpy.asarray(A, dtype=numpy.float64)
    B = numpy.asarray(B, dtype=numpy.float64)
    assert A.shape[1] == B.shape[0] and A.shape[1] <= 8192
    SA, RA = _split_rows(A, slices)
    SBt, RBt = _split_rows(B.T, slices)
    acc = numpy.zeros((A.shape[0], B.shape[1]), dtype=LD)
    # smallest terms first
    acc += RA[slices] @ B
    for p in range(slices, 0, -1):
        acc += SA[p - 1] @ RBt[slices + 1 - p].T
    for level in range(slices + 1, 1, -1):
        for p in range(1, level):
            acc += SA[p - 1] @ SBt[level - p - 1].T
    return acc


def exact_gram(L, slices=3):
    """L @ L.T as longdouble (exact_product; the slice pairs (p, q) and (q, p) are each
    other's transposes and are formed once), exactly symmetric."""
    L = numpy.asarray(L, dtype=numpy.float64)
    assert L.shape[1] <= 8192
    S, R = _split_rows(L, slices)
    acc = numpy.zeros((L.shape[0], L.shape[0]), dtype=LD)
    # the rounded part: sum_p S_p R_{slices+1-p}^T + R_slices L^T, symmetric up to its
    # (irrelevant) rounding; symmetrised
    t = R[slices] @ L.T
    for p in range(slices, 0, -1):
        t += S[p - 1] @ R[slices + 1 - p].T
    acc += 0.5 * (t + t.T)
    for level in range(slices + 1, 1, -1):
        for p in range(1, level):
            q = level - p
            if p > q:
                continue
            m = S[p - 1] @ S[q - 1].T
            acc += m if p == q else m + m.T
    return acc


def tile_max(ratio, ts=TS):
    """Per-tile maxima of an entrywise ratio (n x n -> nt x nt, float64)."""
    n = ratio.shape[0]
    nt = (n + ts - 1) // ts
    out = numpy.zeros((nt, nt))
    for i in range(nt):
        for j in range(nt):
            blk = ratio[i * ts:(i + 1) * ts, j * ts:(j + 1) * ts]
            out[i, j] = float(numpy.max(blk)) if blk.size else 0.0
    return out


def _ratio(res, den):
    """|res| / den entrywise (longdouble); an entry with den == 0 must have res == 0."""
    res = numpy.abs(res)
    assert not numpy.any((den == 0) & (res != 0)), 'a residual where the bound is zero'
    return res / numpy.where(den == 0, 1.0, den)


def abs_gram(L):
    """(|L| |L^T|) in float64 (a denominator: its own rounding, n u relative, is
    immaterial)."""
    a = numpy.abs(numpy.asarray(L, dtype=numpy.float64))
    return a @ a.T


def omega_chol(A, L, tiles=False):
    r = _ratio(numpy.asarray(A, dtype=LD) - exact_gram(L), abs_gram(L))
    return (float(r.max()), tile_max(r)) if tiles else float(r.max())


def omega_inv(L, W, tiles=False, both=False):
    """The smaller of the two residuals of W^T = L^-1 (both=True: the pair), over the
    lower triangle; the strict upper triangle of either product is structurally zero
    (exact zeros times anything) and is asserted to be so."""
    L = numpy.asarray(L, dtype=numpy.float64)
    Y = numpy.ascontiguousarray(numpy.asarray(W, dtype=numpy.float64).T)
    n = L.shape[0]
    eye = numpy.eye(n, dtype=LD)
    low = numpy.tril(numpy.ones((n, n), dtype=bool))
    out = []
    for P, Q in ((Y, L), (L, Y)):
        prod = exact_product(P, Q)
        assert not numpy.any(prod[~low]), 'the product of two lower triangles has an upper part'
        r = _ratio(numpy.where(low, prod - eye, 0.0), numpy.abs(P) @ numpy.abs(Q))
        out.append((float(r.max()), tile_max(r)))
    if both:
        return out[0][0], out[1][0]
    best = min(out, key=lambda o: o[0])
    return best if tiles else best[0]


def omega_gram(W, T, tiles=False):
    r = _ratio(numpy.asarray(T, dtype=LD) - exact_gram(W), abs_gram(W))
    return (float(r.max()), tile_max(r)) if tiles else float(r.max())


def omega_solve(A, L, x, b):
    """max over rows and columns of |b - A x| / ((|L| |L^T|) |x|)."""
    x = numpy.asarray(x, dtype=numpy.float64)
    b = numpy.asarray(b, dtype=numpy.float64)
    x2 = x[:, None] if x.ndim == 1 else x
    b2 = b[:, None] if b.ndim == 1 else b
    res = b2.astype(LD) - exact_product(A, x2)
    a = numpy.abs(numpy.asarray(L, dtype=numpy.float64))
    return float(_ratio(res, a @ (a.T @ numpy.abs(x2))).max())


def logdet_from_factor(L):
    """-> (2 sum log l_ii, 2 sum |log l_ii|) in longdouble."""
    lg = numpy.log(numpy.diag(L).astype(LD))
    return 2 * numpy.sum(lg), 2 * numpy.sum(numpy.abs(lg))


def blocked_reference(A, ts=TS):
    """-> (L, W): the device's algorithm in plain float64 numpy.

    Right-looking blocked Cholesky on ts-tiles: the diagonal tile by numpy.linalg.cholesky,
    its explicit inverse X by a triangular solve of I, the panel as A_ik @ X^T, then the
    trailing update. W = L^-T the way the device builds it, from the same X: Y = L^-1 by
    Y_kj = X_kk B_kj (j <= k), B_ij -= L_ik Y_kj (i > k), B = I at the start."""
    A = numpy.array(A, dtype=numpy.float64)
    n = A.shape[0]
    L = numpy.zeros((n, n))
    Y = numpy.zeros((n, n))
    B = numpy.eye(n)
    for k0 in range(0, n, ts):
        k1 = min(n, k0 + ts)
        s = slice(k0, k1)
        Lkk = numpy.linalg.cholesky(A[s, s])
        X = scipy.linalg.solve_triangular(Lkk, numpy.eye(k1 - k0), lower=True)
        L[s, s] = Lkk
        if k1 < n:
            P = A[k1:, s] @ X.T
            L[k1:, s] = P
            A[k1:, k1:] -= P @ P.T
        Y[s, :k0] = X @ B[s, :k0]
        Y[s, s] = X                    # B_kk = I
        if k1 < n:
            B[k1:, :k1] -= L[k1:, s] @ Y[s, :k1]
    return L, numpy.ascontiguousarray(Y.T)


def kappa_max(L, ts=TS):
    """max over the diagonal ts-tiles of cond_2(L_kk)."""
    n = L.shape[0]
    return max(float(numpy.linalg.cond(L[k:k + ts, k:k + ts])) for k in range(0, n, ts))
