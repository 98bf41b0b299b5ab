"""Host-side evaluation of backward errors of the dense path's and the band path's
stages (test infrastructure; numpy and scipy only, no device; the band path's part has
its own notes further down).

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


def _hi_lo(A):
    """A longdouble operand as float64 hi + lo, exactly (lo None where it is zero:
    every float64 operand)."""
    A = numpy.asarray(A)
    if A.dtype != LD:
        return numpy.asarray(A, dtype=numpy.float64), None
    hi = A.astype(numpy.float64)
    lo = (A - hi).astype(numpy.float64)      # exact: 11 bits
    return hi, (lo if numpy.any(lo) else None)


def exact_product(A, B, slices=3):
    """A @ B as longdouble, far below u |A| |B|, for float64 or longdouble operands.

    A longdouble operand is hi + lo in float64; hi @ hi is the sliced product below, and
    the terms with a lo, of relative size 2^-53, are plain float64 products (their
    rounding, k u 2^-53 |A| |B|, is below the longdouble sum's own)."""
    Ah, Al = _hi_lo(A)
    Bh, Bl = _hi_lo(B)
    acc = _exact_product64(Ah, Bh, slices)
    if Al is not None:
        acc += Al @ Bh
    if Bl is not None:
        acc += Ah @ Bl
    if Al is not None and Bl is not None:
        acc += Al @ Bl
    return acc


def _exact_product64(A, B, slices=3):
    """A @ B of float64 operands as longdouble, far below u |A| |B|.

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


# ------------------------------------------------------------------ band path --
# The stages of the band path (K_pad = Q B Q^T, Y = Q^T R, the solves and the selected
# inverse of B + eta I, the tridiagonal and its eigenvalues), each on what the device
# read back. N = n_pad; K_pad is K padded by the identity. Every metric returns
# (value, where): `where` names the 128-block (or the index) of its maximum.
#   omega_orth   ||Q^T Q - I||_F            Q = prod_j (I - V_j T_j V_j^T), longdouble
#   omega_sim    ||K Q - Q B||_F / ||K||_F
#   omega_rhs    ||Y - Q^T R||_F / ||R||_F
#   omega_band_solve   max |Y - A x| / (|A| |x| + |Y|), A = B + eta I
#   gram_residual      max |G - P^T Q| / (|P|^T |Q|)
#   omega_sinv   max over block columns k of |sum_j A_kj Z_jk - I| / sum_j |A_kj| |Z_jk|
#   sturm_ok     count(lam_i - delta) <= i < count(lam_i + delta) for every i
# The restatements the bars come from are tools/band_proto.py, tools/cholqr_proto.py,
# tools/chase_proto.py and bcr_sinv_reference below (tools/bcr_sinv_proto.py returning
# the off-diagonal blocks as well).

def band_q(V, T, ts=TS):
    """Q = (I - V_0 T_0 V_0^T) (I - V_1 T_1 V_1^T) ... in longdouble; V [N][N] with panel
    j in columns [ts j, +ts) and rows from ts (j + 1), T [nt - 1][ts][ts] as stored."""
    N = V.shape[0]
    Q = numpy.eye(N, dtype=LD)
    for j in range(N // ts - 1):
        r0, c0 = (j + 1) * ts, j * ts
        Vj = numpy.ascontiguousarray(V[r0:, c0:c0 + ts])
        QVT = exact_product(exact_product(Q[:, r0:], Vj), T[j])
        Q[:, r0:] -= exact_product(QVT, Vj.T)
    return Q


def _fro(R):
    return float(numpy.sqrt(numpy.sum(numpy.asarray(R, dtype=LD) ** 2)))


def _worst_tile(R, ts=TS):
    """The 128-tile (block row alone for a tall R) with the largest Frobenius norm."""
    R2 = numpy.asarray(R, dtype=LD) ** 2
    nr = (R2.shape[0] + ts - 1) // ts
    nc = (R2.shape[1] + ts - 1) // ts if R2.shape[1] > ts else 1
    best, at = -1.0, (0, 0)
    for i in range(nr):
        for j in range(nc):
            blk = R2[i * ts:(i + 1) * ts, j * ts:(j + 1) * ts] if nc > 1 else \
                R2[i * ts:(i + 1) * ts]
            v = float(numpy.sum(blk))
            if v > best:
                best, at = v, (i, j)
    return at


def omega_orth(Q):
    R = exact_product(Q.T, Q) - numpy.eye(Q.shape[0], dtype=LD)
    return _fro(R), _worst_tile(R)


def omega_sim(K, Q, B):
    R = exact_product(K, Q) - exact_product(Q, B)
    return _fro(R) / _fro(K), _worst_tile(R)


def omega_rhs(Q, R, Y):
    res = numpy.asarray(Y, dtype=LD) - exact_product(Q.T, R)
    return _fro(res) / _fro(R), _worst_tile(res)


def band_structure(B, V, n, ts=TS):
    """The exact properties of the read-back: B symmetric and zero outside the band, its
    pad block the identity and decoupled; the pad rows of V zero but for the unit
    diagonal written there (a ragged last panel: identity reflectors), V unit lower
    trapezoidal per panel. -> list of the violated ones (empty: none)."""
    N = B.shape[0]
    i, j = numpy.indices((N, N))
    bad = []
    if not numpy.array_equal(B, B.T):
        bad.append('B is not symmetric')
    if numpy.any(B[numpy.abs(i - j) > ts]):
        bad.append('B is not zero outside the band')
    if not numpy.array_equal(B[n:, n:], numpy.eye(N - n)) or numpy.any(B[n:, :n]):
        bad.append('the pad block of B is not a decoupled identity')
    if numpy.any(V[n:][(i - j != ts)[n:]]):
        bad.append('the pad rows of V are not zero')
    for p in range(N // ts - 1):
        r0, c0 = (p + 1) * ts, p * ts
        top = V[r0:r0 + ts, c0:c0 + ts]
        if numpy.any(numpy.triu(top, 1)) or not numpy.all(numpy.diag(top) == 1.0):
            bad.append('panel %d of V is not unit lower trapezoidal' % p)
        if numpy.any(V[:r0, c0:c0 + ts]):
            bad.append('panel %d of V reaches above its first row' % p)
    if numpy.any(V[:, N - ts:]):
        bad.append('V has a panel past the last one')
    return bad


def band_of(A, ts=TS):
    """The symmetric band matrix a reduction left in the lower triangle of A (below the
    band A may hold reflectors)."""
    N = A.shape[0]
    i, j = numpy.indices((N, N))
    L = numpy.where((i >= j) & (i - j <= ts), A, 0.0)
    return L + numpy.tril(L, -1).T


def panels_to_v(Vs, Ts, N, ts=TS):
    """A restatement's per-panel V, T in the read-back's layout."""
    V = numpy.zeros((N, N))
    for p, Vp in enumerate(Vs):
        V[(p + 1) * ts:, p * ts:(p + 1) * ts] = Vp
    return V, numpy.array(Ts).reshape(len(Ts), ts, ts)


def reduction_metrics(K, B, V, T, R=None, Y=None):
    """-> dict(orth, sim, rhs) of (value, where)."""
    Q = band_q(V, T)
    out = dict(orth=omega_orth(Q), sim=omega_sim(K, Q, B))
    if R is not None:
        out['rhs'] = omega_rhs(Q, R, Y)
    return out


def omega_band_solve(A, x, y, ts=TS):
    """Componentwise residual of A x = y, A = B + eta I: max |y - A x| / (|A| |x| + |y|)
    (0 / 0 = 0; a residual over a zero bound fails) -> (value, block row of the
    maximum)."""
    x = numpy.asarray(x, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    res = y.astype(LD) - exact_product(A, x)
    r = _ratio(res, numpy.abs(A) @ numpy.abs(x) + numpy.abs(y))
    return float(r.max()), int(numpy.argmax(r.max(axis=1))) // ts


def gram_residual(P, Q, G):
    """max |G - P^T Q| / (|P|^T |Q|) for the Gram block G the device returned."""
    P = numpy.asarray(P, dtype=numpy.float64)
    Q = numpy.asarray(Q, dtype=numpy.float64)
    r = _ratio(numpy.asarray(G, dtype=LD) - exact_product(P.T, Q), numpy.abs(P).T @ numpy.abs(Q))
    return float(r.max())


def band_chol_solve(A, Y, ts=TS):
    """The sequential explicit-inverse band Cholesky of band_proto.band_chol with its back
    substitution (band_chol_kernel, band_der_kernel) in float64 -> x = A^-1 Y."""
    N = A.shape[0]
    nt = N // ts
    Li, C, z = [], [], []
    D = A[:ts, :ts].copy()
    r = Y[:ts].copy()
    for k in range(nt):
        L = numpy.linalg.cholesky(D)
        Li.append(scipy.linalg.solve_triangular(L, numpy.eye(ts), lower=True))
        z.append(Li[k] @ r)
        if k + 1 == nt:
            break
        s, t = slice(k * ts, (k + 1) * ts), slice((k + 1) * ts, (k + 2) * ts)
        C.append(A[t, s] @ Li[k].T)
        r = Y[t] - C[k] @ z[k]
        D = A[t, t] - C[k] @ C[k].T
    x = numpy.zeros_like(Y)
    for k in range(nt - 1, -1, -1):
        rhs = z[k] if k + 1 == nt else z[k] - C[k].T @ x[(k + 1) * ts:(k + 2) * ts]
        x[k * ts:(k + 1) * ts] = Li[k].T @ rhs
    return x


def band_logdet(A, bw=TS):
    """2 sum log l_ii of the banded Cholesky of A in longdouble (a column loop,
    O(n bw^2)) -> (logdet, the factor's diagonal)."""
    n = A.shape[0]
    A = numpy.asarray(A, dtype=LD)
    L = numpy.zeros((n, n), dtype=LD)
    for j in range(n):
        k0, i1 = max(0, j - bw), min(n, j + bw + 1)
        v = A[j:i1, j] - L[j:i1, k0:j] @ L[j, k0:j]
        assert v[0] > 0, 'not positive definite at %d' % j
        L[j:i1, j] = v / numpy.sqrt(v[0])
    dg = numpy.diag(L)
    return 2 * numpy.sum(numpy.log(dg)), dg


def logdet_bar(A, eps):
    """First-order bound of |delta logdet| under a Cholesky backward error eps:
    eps tr(|A^-1| |L| |L^T|), float64 with LAPACK's L."""
    a = numpy.abs(numpy.linalg.cholesky(A))
    return eps * float(numpy.sum(numpy.abs(numpy.linalg.inv(A)) * (a @ a.T)))


def band_blocks(B, ts=TS):
    """-> (D[k] = B_kk, F[k] = B_{k+1,k})."""
    nt = B.shape[0] // ts
    D = [B[k * ts:(k + 1) * ts, k * ts:(k + 1) * ts] for k in range(nt)]
    F = [B[(k + 1) * ts:(k + 2) * ts, k * ts:(k + 1) * ts] for k in range(nt - 1)]
    return D, F


def omega_sinv(B, eta, Zd, Zsub, ts=TS, tangent=None):
    """Residual of the block-tridiagonal part of Z = (B + eta I)^-1, Zd[k] = Z_kk and
    Zsub[k] = Z_{k+1,k}: max over block columns k and entries of
    |A_k,k-1 Z_k-1,k + A_kk Z_kk + A_k,k+1 Z_k+1,k - I| / (the same with |.|)
    -> (value, k of the maximum). tangent = (dZd, dZsub): the residual of
    Z + A dZ = 0 on the same blocks, |Z_kk + sum_j A_kj dZ_jk| / (|Z_kk| + sum_j
    |A_kj| |dZ_jk|)."""
    D, F = band_blocks(B, ts)
    nt = len(D)
    eye = numpy.eye(ts)
    Xd, Xsub = (Zd, Zsub) if tangent is None else tangent
    best, at = 0.0, 0
    for k in range(nt):
        terms = [(D[k] + eta * eye, Xd[k])]
        if k > 0:
            terms.append((F[k - 1], Xsub[k - 1].T))
        if k + 1 < nt:
            terms.append((F[k].T, Xsub[k]))
        if tangent is None:
            acc, den = -eye.astype(LD), numpy.zeros((ts, ts))
        else:
            acc, den = numpy.asarray(Zd[k], dtype=LD), numpy.abs(Zd[k])
        for a, z in terms:
            a, z = numpy.ascontiguousarray(a), numpy.ascontiguousarray(z)
            acc = acc + exact_product(a, z)
            den = den + numpy.abs(a) @ numpy.abs(z)
        v = float(_ratio(acc, den).max())
        if v > best:
            best, at = v, k
    return best, at


def sinv_asymmetry(Zd):
    """max over the diagonal blocks k of max |Zd_k - Zd_k^T| / max |Zd_k| -> (value, k)."""
    v = [float(numpy.max(numpy.abs(z - z.T)) / numpy.max(numpy.abs(z))) for z in Zd]
    k = int(numpy.argmax(v))
    return v[k], k


def sub_blocks(Zo):
    """Z_{k+1,k} in original order from the selected inversion's Zo (by original block o:
    Z_lo, Z_ro): odd k its own right block, even k the transpose of the left block of
    k + 1 (the mapping of Band.sinv_blocks)."""
    nt = len(Zo)
    return numpy.array([Zo[k][1] if k % 2 == 1 else numpy.asarray(Zo[k + 1][0]).T
                        for k in range(nt - 1)]).reshape(nt - 1, TS, TS)


def bcr_sinv_reference(B, eta, ts=TS, swap=None):
    """tools/bcr_sinv_proto.py on B + eta I (the cyclic reduction's factor, then the
    selected inversion down its tree, float64) -> (Zd [nt], Zsub [nt - 1], Zo): the first
    two in original order, as Band.sinv_blocks returns them. swap = o (test_backward_host:
    an injected defect): the selected inversion reads W_l and W_r of block o in each other's
    place (in the factorization itself the swap ends in a failed pivot, which is reported)."""
    D, F = band_blocks(B, ts)
    nt = len(D)
    D = [d + eta * numpy.eye(ts) for d in D]
    inv = lambda L: scipy.linalg.solve_triangular(L, numpy.eye(ts), lower=True)  # noqa: E731
    Linv = [None] * nt
    W = [[None, None] for _ in range(nt)]
    Dl, Fl = list(D), list(F)
    m, lvl, ms = nt, 0, []
    while m > 1:
        ms.append(m)
        for p in range(1, m, 2):
            o = p << lvl
            Linv[o] = inv(numpy.linalg.cholesky(Dl[p]))
            W[o][0] = Linv[o] @ Fl[p - 1]
            W[o][1] = Linv[o] @ Fl[p].T if p + 1 < m else None
        D2, F2 = [], []
        for j in range(0, m, 2):
            Dj = Dl[j].copy()
            if j >= 1:
                Dj -= W[(j - 1) << lvl][1].T @ W[(j - 1) << lvl][1]
            if j + 1 < m:
                Dj -= W[(j + 1) << lvl][0].T @ W[(j + 1) << lvl][0]
            D2.append(Dj)
            if j + 2 < m:
                F2.append(-W[(j + 1) << lvl][1].T @ W[(j + 1) << lvl][0])
        Dl, Fl = D2, F2
        m = (m + 1) // 2
        lvl += 1
    Linv[0] = inv(numpy.linalg.cholesky(Dl[0]))
    if swap is not None:
        W[swap][0], W[swap][1] = W[swap][1], W[swap][0]
    Zd = [None] * nt
    Zo = [[None, None] for _ in range(nt)]
    Zd[0] = Linv[0].T @ Linv[0]
    for lv in range(lvl - 1, -1, -1):
        m = ms[lv]
        for p in range(1, m, 2):
            o, ol = p << lv, (p - 1) << lv
            Xl = W[o][0].T @ Linv[o]
            if p + 1 < m:
                orr = (p + 1) << lv
                Xr = W[o][1].T @ Linv[o]
                # the parents' coupling one level up: the left block of r' if r' is odd
                # there, else the right block of l', transposed
                Zlr = Zo[orr][0] if ((p - 1) // 2 + 1) % 2 == 1 else Zo[ol][1].T
                Zlp = -(Zd[ol] @ Xl + Zlr @ Xr)
                Zrp = -(Zlr.T @ Xl + Zd[orr] @ Xr)
                Zo[o] = [Zlp, Zrp]
                Zd[o] = Linv[o].T @ Linv[o] - Xl.T @ Zlp - Xr.T @ Zrp
            else:
                Zlp = -(Zd[ol] @ Xl)
                Zo[o] = [Zlp, None]
                Zd[o] = Linv[o].T @ Linv[o] - Xl.T @ Zlp
    Zsub = [Zo[k][1] if k % 2 == 1 else Zo[k + 1][0].T for k in range(nt - 1)]
    return numpy.array(Zd), numpy.array(Zsub).reshape(nt - 1, ts, ts), Zo


def bcr_dsinv_reference(B, eta, ts=TS, drop=None):
    """tools/bcr_dsinv_proto.py on B + eta I (the factor and the selected inversion with
    their eta-tangents, float64) -> (Zd, Zsub, dZd, dZsub) in original order. drop = o
    (test_backward_host: an injected defect): dZ_{l,o} of block o is left zero."""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import bcr_dsinv_proto
    D, F = band_blocks(B, ts)
    D = [d + eta * numpy.eye(ts) for d in D]
    Zd, Zo, dZd, dZo = bcr_dsinv_proto.sinv_tan(*bcr_dsinv_proto.bcr_factor_tan(D, F),
                                                want_blocks=True)
    if drop is not None:
        dZo[drop][0] = numpy.zeros((ts, ts))
    return numpy.array(Zd), sub_blocks(Zo), numpy.array(dZd), sub_blocks(dZo)


def sturm_count(d, e2, x):
    """The number of eigenvalues below each x of the tridiagonal (d, e2 = squared
    subdiagonal), by the Sturm sequence in longdouble (a zero pivot is replaced by
    -pivmin, as dstebz does)."""
    d = numpy.asarray(d, dtype=LD)
    e2 = numpy.asarray(e2, dtype=LD)
    x = numpy.asarray(x, dtype=LD)
    pivmin = LD(numpy.finfo(numpy.float64).tiny) * max(LD(1), e2.max() if e2.size else LD(1))
    q = d[0] - x
    q = numpy.where(numpy.abs(q) < pivmin, -pivmin, q)
    cnt = (q < 0).astype(numpy.int64)
    for i in range(1, d.shape[0]):
        q = d[i] - x - e2[i - 1] / q
        q = numpy.where(numpy.abs(q) < pivmin, -pivmin, q)
        cnt += q < 0
    return cnt


def sturm_ok(d, e2, lam, delta):
    """count(lam_i - delta) <= i < count(lam_i + delta) for every i -> (ok, first i that
    fails or -1)."""
    lam = numpy.asarray(lam, dtype=LD)
    i = numpy.arange(lam.shape[0])
    lo = sturm_count(d, e2, lam - delta)
    hi = sturm_count(d, e2, lam + delta)
    bad = numpy.flatnonzero(~((lo <= i) & (i < hi)))
    return bad.size == 0, (int(bad[0]) if bad.size else -1)


def sturm_margin(d, e2, lam, scale, m_max=2 ** 20):
    """The smallest power of two m at which lam passes sturm_ok with delta = m u scale."""
    m = 1
    while m <= m_max:
        if sturm_ok(d, e2, lam, m * U * scale)[0]:
            return m
        m *= 2
    return None


def chase_invariants(B, d, e2):
    """What an orthogonal similarity keeps, in longdouble: -> (|tr T - tr B| / sum |b_ii|,
    | ||T||_F - ||B||_F | / ||B||_F)."""
    B = numpy.asarray(B, dtype=LD)
    d = numpy.asarray(d, dtype=LD)
    e2 = numpy.asarray(e2, dtype=LD)
    tr = abs(numpy.sum(d) - numpy.trace(B)) / numpy.sum(numpy.abs(numpy.diag(B)))
    fb = numpy.sqrt(numpy.sum(B * B))
    ft = numpy.sqrt(numpy.sum(d * d) + 2 * numpy.sum(e2))
    return float(tr), float(abs(ft - fb) / fb)
