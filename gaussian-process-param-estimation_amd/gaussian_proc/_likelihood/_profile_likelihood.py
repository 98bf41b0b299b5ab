"""Profiled GP log-likelihood in (sigma, eta).

Drop-in for ``ProfileLikelihood`` of the reference
(gaussian_proc/_likelihood/_profile_likelihood.py:32-415).

``log_likelihood`` (:38-85) uses the same single-factorization terms as the
direct likelihood: with G = [X z]^T (K + eta I)^-1 [X z],
  lp = -(n-m)/2 log sigma^2 - logdet(K + eta I)/2 - log det G_XX / 2
       - (G_zz - G_Xz^T G_XX^-1 G_Xz) / (2 sigma^2).
The reference materialises Y B^-1 Y^T as an n x n matrix (:73); the value is the
same. The eta-derivatives (:91-192) keep the reference formulas on the operator
duck type; on the dense eigenvalue operator they come instead from the Gram
blocks Gp = [X z]^T (K + eta I)^-p [X z], p = 1..3, of the band path
(MixedCorrelation.der_terms, any number of eta per call) and traceinv of
exponents 1 and 2 from the same factor (selected inversion and its eta-tangent),
with the same algebra written in those blocks (_der_from_terms).
"""

import numpy
from scipy.linalg import solve_triangular
from scipy.optimize import minimize
from functools import partial

from ._root_finding import chandrupatla_method, BatchedFunction, \
    find_interval_with_sign_change_batched

__all__ = ['ProfileLikelihood']


def _use_band(K_mixed):
    return hasattr(K_mixed, 'der_terms') and getattr(K_mixed, 'imate_method', None) == \
        'eigenvalue'


def _der_from_terms(n, m, G1, G2, G3, tr1, tr2=None):
    """der1 (and der2 when tr2 is given) of the profiled likelihood from
    Gp = [X z]^T S^-p [X z], S = K + eta I, and tr(S^-1), tr(S^-2); the terms of
    _profile_likelihood.py:91-192 in those blocks: Mz = S^-1 (z - X a) with
    a = B^-1 X^T S^-1 z, B = X^T S^-1 X."""
    B = G1[:m, :m]
    a = numpy.linalg.solve(B, G1[:m, m])
    zMz = G1[m, m] - G1[:m, m] @ a
    zM2z = G2[m, m] - 2.0 * (a @ G2[:m, m]) + a @ G2[:m, :m] @ a
    A = numpy.linalg.solve(B, G2[:m, :m])            # B^-1 Y^T Y
    trace_M = tr1 - numpy.trace(A)
    sigma02 = zMz / (n - m)
    der1 = -0.5 * (trace_M - zM2z / sigma02)
    if tr2 is None:
        return der1, None
    trace_M2 = tr2 - 2.0 * numpy.trace(numpy.linalg.solve(B, G3[:m, :m])) + numpy.trace(A @ A)
    MzS1Mz = G3[m, m] - 2.0 * (a @ G3[:m, m]) + a @ G3[:m, :m] @ a
    YtMz = G2[:m, m] - G2[:m, :m] @ a
    zM3z = MzS1Mz - YtMz @ numpy.linalg.solve(B, YtMz)
    der2 = (0.5 / sigma02) * ((trace_M2 / (n - m) + (trace_M / (n - m)) ** 2) * zMz -
                              2.0 * zM3z)
    return der1, der2


def _predict_from_terms(c, q, G, Phi_star, sigma, sigma0, noise=False):
    """Posterior mean and variance at n* new points (universal kriging) from the
    prediction terms of MixedCorrelation.predict_terms. With S = K + eta I,
    eta = (sigma0 / sigma)^2, R = [X z] and k*_j the correlations of new point j
    with the training points:
      c[j]  = R^T S^-1 k*_j            (n* x (m + 1))
      q[j]  = k*_j^T S^-1 k*_j         (n*)
      G     = R^T S^-1 R               ((m + 1) x (m + 1))
    and Phi_star (n* x m) the basis rows of the new points. Then, with B = G_XX,
      beta  = B^-1 G_Xz
      mean  = Phi_star beta + c_z - c_X beta        (= phi beta + k*^T S^-1 (z - X beta))
      var   = sigma^2 (1 - q + r^T B^-1 r),  r = phi - c_X   (the latent function;
              ``noise`` adds sigma0^2)
    m = 0 (no basis) leaves mean = c_z and var = sigma^2 (1 - q). -> (mean, var)."""
    c = numpy.asarray(c, dtype=float)
    q = numpy.asarray(q, dtype=float)
    G = numpy.asarray(G, dtype=float)
    m = G.shape[0] - 1
    if m < 0 or G.shape != (m + 1, m + 1) or c.ndim != 2 or c.shape[1] != m + 1 or \
            q.shape != (c.shape[0],):
        raise ValueError('c must be n* x (m + 1), q n* and G (m + 1) x (m + 1)')
    Phi = numpy.asarray(Phi_star, dtype=float).reshape(c.shape[0], -1)
    if Phi.shape[1] != m:
        raise ValueError('Phi_star must be n* x %d' % m)
    if not sigma > 0.0:
        raise ValueError('sigma must be positive')
    var = 1.0 - q
    if m == 0:
        mean = c[:, 0].copy()
    else:
        B = G[:m, :m]
        beta = numpy.linalg.solve(B, G[:m, m])
        mean = Phi @ beta + (c[:, m] - c[:, :m] @ beta)
        r = Phi - c[:, :m]
        var = var + numpy.sum(r * numpy.linalg.solve(B, r.T).T, axis=1)
    var = sigma ** 2 * var
    if noise:
        var = var + sigma0 ** 2
    return mean, var


def _loo_from_terms(dinv, sol, G, z, sigma, sigma0, noise=True):
    """Leave-one-out predictions of the n training values (universal kriging, beta
    re-estimated without point i, sigma and sigma0 kept) from the terms of
    MixedCorrelation.loo_terms. With S = K + eta I, eta = (sigma0 / sigma)^2 and
    R = [X z]:
      dinv[i] = (S^-1)_ii              (n)
      sol     = S^-1 R                 (n x (m + 1))
      G       = R^T S^-1 R             ((m + 1) x (m + 1))
    Then, with B = G_XX, u_i the first m entries of row i of sol and
    P = S^-1 - S^-1 X B^-1 X^T S^-1 (Dubrule 1983),
      P_ii   = dinv_i - u_i^T B^-1 u_i
      (Pz)_i = sol_iz - u_i^T B^-1 G_Xz
      mean_i = z_i - (Pz)_i / P_ii
      var_i  = sigma^2 / P_ii          (the noisy observation; ``noise=False``
                                        subtracts sigma0^2: the latent function)
    m = 0 (no basis) leaves P = S^-1. -> (mean, var)."""
    dinv = numpy.asarray(dinv, dtype=float)
    sol = numpy.asarray(sol, dtype=float)
    G = numpy.asarray(G, dtype=float)
    z = numpy.asarray(z, dtype=float)
    m = G.shape[0] - 1
    n = dinv.shape[0]
    if m < 0 or G.shape != (m + 1, m + 1) or dinv.ndim != 1 or sol.shape != (n, m + 1) or \
            z.shape != (n,):
        raise ValueError('dinv and z must be n, sol n x (m + 1) and G (m + 1) x (m + 1)')
    if not sigma > 0.0:
        raise ValueError('sigma must be positive')
    if m == 0:
        pii, pz = dinv, sol[:, 0]
    else:
        B = G[:m, :m]
        u = sol[:, :m]
        Biu = numpy.linalg.solve(B, u.T).T
        pii = dinv - numpy.sum(u * Biu, axis=1)
        pz = sol[:, m] - Biu @ G[:m, m]
    mean = z - pz / pii
    var = sigma ** 2 / pii
    if not noise:
        var = var - sigma0 ** 2
    return mean, var


def _scale_grad_coef(G):
    """The two symmetric coefficient matrices MixedCorrelation.scale_grad_terms hands to
    the device, from G = R^T A^-1 R, R = [X z]: C_X = [[G_XX^-1, 0], [0, 0]] and c c^T with
    c = [-a; 1], a = G_XX^-1 G_Xz (so that Sol c = P z). m = 0 leaves C_X = 0 and c = [1].
    -> array (2, m + 1, m + 1)."""
    G = numpy.asarray(G, dtype=float)
    m = G.shape[0] - 1
    if m < 0 or G.shape != (m + 1, m + 1):
        raise ValueError('G must be (m + 1) x (m + 1)')
    coef = numpy.zeros((2, m + 1, m + 1))
    c = numpy.ones(m + 1)
    if m > 0:
        Bi = numpy.linalg.inv(G[:m, :m])
        coef[0, :m, :m] = 0.5 * (Bi + Bi.T)
        c[:m] = -numpy.linalg.solve(G[:m, :m], G[:m, m])
    coef[1] = numpy.outer(c, c)
    return coef


def _scale_grad_from_terms(n, m, t, qX, qc, G, sigma=None):
    """Gradient of the log-likelihood in the correlation scale rho (d entries) from the
    terms of MixedCorrelation.scale_grad_terms. With A = K + eta I, dK_k = dK / d rho_k,
    P = A^-1 - A^-1 X G_XX^-1 X^T A^-1 and w = P z:
      t[k] = tr(A^-1 dK_k),  qX[k] = tr(A^-1 X G_XX^-1 X^T A^-1 dK_k),  qc[k] = w^T dK_k w,
      tr(P dK_k) = t[k] - qX[k],   z^T P z = c^T G c,  c = [-G_XX^-1 G_Xz; 1].
    ``sigma`` given: the direct likelihood at (sigma, sigma0 = sqrt(eta) sigma),
      dl / d rho_k  = -tr(P dK_k) / 2 + w^T dK_k w / (2 sigma^2);
    ``sigma`` None: the likelihood profiled over sigma (sigma^2 = z^T P z / (n - m)),
      dlp / d rho_k = -tr(P dK_k) / 2 + (n - m) w^T dK_k w / (2 z^T P z).
    -> array (d)."""
    t = numpy.asarray(t, dtype=float)
    qX = numpy.asarray(qX, dtype=float)
    qc = numpy.asarray(qc, dtype=float)
    G = numpy.asarray(G, dtype=float)
    if G.shape != (m + 1, m + 1) or t.ndim != 1 or qX.shape != t.shape or qc.shape != t.shape:
        raise ValueError('t, qX and qc must be d and G (m + 1) x (m + 1)')
    if sigma is None:
        zPz = G[m, m] - (G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m]) if m > 0 else 0.0)
        s = 0.5 * (n - m) / zPz
    else:
        if not abs(sigma) > 0.0:
            raise ValueError('sigma must be non-zero')
        s = 0.5 / sigma ** 2
    return -0.5 * (t - qX) + s * qc


def _eta_grad_from_terms(n, m, trinv, sol, G):
    """d lp / d eta of the likelihood profiled over sigma, from the leave-one-out terms
    (_scale_grad_from_terms with dA = I): -tr(P) / 2 + (n - m) w^T w / (2 z^T P z) with
    tr(P) = tr(A^-1) - tr(G_XX^-1 U^T U), U = sol[:, :m], w = sol c. -> float."""
    sol = numpy.asarray(sol, dtype=float)
    G = numpy.asarray(G, dtype=float)
    c = numpy.ones(m + 1)
    trP = float(trinv)
    if m > 0:
        c[:m] = -numpy.linalg.solve(G[:m, :m], G[:m, m])
        U = sol[:, :m]
        trP -= float(numpy.trace(numpy.linalg.solve(G[:m, :m], U.T @ U)))
    w = sol @ c
    return -0.5 * trP + 0.5 * (n - m) * float(w @ w) / float(c @ G @ c)


def _fisher_from_terms(n, m, sigma, sigma0, terms):
    """The expected information of the restricted likelihood in
    theta = (sigma, sigma0, rho_1 .. rho_d) from the terms of
    MixedCorrelation.fisher_terms: I_ab = tr(P_S S_a P_S S_b) / 2 with
    S = sigma^2 K + sigma0^2 I = sigma^2 A, S_a = dS / d theta_a and P_S = P / sigma^2 its
    REML projector, P = A^-1 - A^-1 X B^-1 X^T A^-1, B = X^T A^-1 X = G_XX. With
    eta = (sigma0 / sigma)^2, N_0 = I, N_k = dK / d rho_k, and from the X part of U, V
    (the expected information does not depend on z)
      p_ab  = tr(P N_a P N_b) = T_ab - 2 tr(B^-1 V_ab) + tr(B^-1 U_a B^-1 U_b)
      tau_a = tr(P N_a)       = (trinv | t_a) - tr(B^-1 U_a),
    the derivatives S_sigma = 2 sigma (A - eta I), S_sigma0 = 2 sigma0 I,
    S_rho_k = sigma^2 N_k and P A P = P, tr(P A) = n - m give
      I[sigma, sigma]   = 2 ((n - m) - 2 eta tau_0 + eta^2 p_00) / sigma^2
      I[sigma, sigma0]  = 2 sigma0 (tau_0 - eta p_00) / sigma^3
      I[sigma0, sigma0] = 2 sigma0^2 p_00 / sigma^4
      I[sigma, rho_k]   = (tau_k - eta p_0k) / sigma
      I[sigma0, rho_k]  = sigma0 p_0k / sigma^2
      I[rho_k, rho_l]   = p_kl / 2.
    -> array (d + 2, d + 2), symmetrised."""
    T = numpy.asarray(terms['T'], dtype=float)
    U = numpy.asarray(terms['U'], dtype=float)
    V = numpy.asarray(terms['V'], dtype=float)
    t = numpy.asarray(terms['t'], dtype=float)
    G = numpy.asarray(terms['G'], dtype=float)
    d1 = T.shape[0]
    if T.shape != (d1, d1) or d1 < 1 or t.shape != (d1 - 1,) or G.shape != (m + 1, m + 1) \
            or U.shape != (d1, m + 1, m + 1) or V.shape != (d1, d1, m + 1, m + 1):
        raise ValueError('T must be (d + 1) x (d + 1), t d, G (m + 1) x (m + 1), U (d + 1) and '
                         'V (d + 1) x (d + 1) blocks of G\'s shape')
    sigma, sigma0 = float(sigma), float(sigma0)
    if not abs(sigma) > 0.0:
        raise ValueError('sigma must be non-zero')
    eta = (sigma0 / sigma) ** 2
    tau = numpy.concatenate([[float(terms['trinv'])], t])
    p = T.copy()
    if m > 0:
        Bi = numpy.linalg.inv(G[:m, :m])
        Bi = 0.5 * (Bi + Bi.T)
        BU = numpy.array([Bi @ U[a, :m, :m] for a in range(d1)])
        for a in range(d1):
            tau[a] -= numpy.trace(BU[a])
            for b in range(d1):
                p[a, b] += -2.0 * numpy.sum(Bi * V[a, b, :m, :m]) + numpy.sum(BU[a] * BU[b].T)
    info = numpy.empty((d1 + 1, d1 + 1))
    info[0, 0] = 2.0 * ((n - m) - 2.0 * eta * tau[0] + eta ** 2 * p[0, 0]) / sigma ** 2
    info[0, 1] = info[1, 0] = 2.0 * sigma0 * (tau[0] - eta * p[0, 0]) / sigma ** 3
    info[1, 1] = 2.0 * sigma0 ** 2 * p[0, 0] / sigma ** 4
    info[0, 2:] = info[2:, 0] = (tau[1:] - eta * p[0, 1:]) / sigma
    info[1, 2:] = info[2:, 1] = sigma0 * p[0, 1:] / sigma ** 2
    info[2:, 2:] = 0.5 * p[1:, 1:]
    return 0.5 * (info + info.T)


def _cross_validation_scores(z, mean, var):
    """The summary scores of GaussianProcess.cross_validate from the leave-one-out
    mean and (noisy) variance. -> dict."""
    z = numpy.asarray(z, dtype=float)
    residual = z - mean
    return {
        'residual': residual,
        'standardized': residual / numpy.sqrt(var),
        'rmse': float(numpy.sqrt(numpy.mean(residual ** 2))),
        'mean_squared_standardized': float(numpy.mean(residual ** 2 / var)),
        'log_pseudo_likelihood': float(numpy.sum(-0.5 * numpy.log(2.0 * numpy.pi * var) -
                                                 residual ** 2 / (2.0 * var))),
    }


def _predict_cov_from_terms(c, G, C0, Phi_star, sigma, sigma0, noise=False):
    """Joint posterior covariance of n* new points (universal kriging) from the
    terms of MixedCorrelation.predict_cov_terms: c and G as in _predict_from_terms
    and C0 = K** - K* S^-1 K*^T (n* x n*, symmetric). With B = G_XX and the rows
    r_j = phi*_j - c_X,j,
      cov = sigma^2 (C0 + r B^-1 r^T)          (the latent function; ``noise`` adds
                                                sigma0^2 on the diagonal only)
    whose diagonal is _predict_from_terms' variance. The rank-m term is symmetrised,
    so cov is exactly symmetric when C0 is. m = 0 leaves cov = sigma^2 C0. -> cov."""
    c = numpy.asarray(c, dtype=float)
    G = numpy.asarray(G, dtype=float)
    C0 = numpy.asarray(C0, dtype=float)
    m = G.shape[0] - 1
    if m < 0 or G.shape != (m + 1, m + 1) or c.ndim != 2 or c.shape[1] != m + 1 or \
            C0.shape != (c.shape[0], c.shape[0]):
        raise ValueError('c must be n* x (m + 1), G (m + 1) x (m + 1) and C0 n* x n*')
    Phi = numpy.asarray(Phi_star, dtype=float).reshape(c.shape[0], -1)
    if Phi.shape[1] != m:
        raise ValueError('Phi_star must be n* x %d' % m)
    if not sigma > 0.0:
        raise ValueError('sigma must be positive')
    cov = C0.copy()
    if m > 0:
        r = Phi - c[:, :m]
        W = r @ numpy.linalg.solve(G[:m, :m], r.T)
        cov += 0.5 * (W + W.T)
    cov *= sigma ** 2
    if noise:
        cov[numpy.diag_indices_from(cov)] += sigma0 ** 2
    return cov


def _sample_lowrank_from_terms(c, G, Phi_star):
    """The rank-m trend term of the joint posterior covariance as a factor: U (n* x m)
    with U U^T = r B^-1 r^T, r = Phi_star - c_X and B = G_XX, the same r and block
    _predict_cov_from_terms uses, so that C0 + U U^T is its covariance in units of
    sigma^2 (noise off). With B = L_B L_B^T, U = r L_B^-T: one Cholesky of the m x m
    block and one triangular solve. m = 0 gives an (n*, 0) U. B not positive definite
    raises numpy.linalg.LinAlgError. -> U."""
    c = numpy.asarray(c, dtype=float)
    G = numpy.asarray(G, dtype=float)
    m = G.shape[0] - 1
    if m < 0 or G.shape != (m + 1, m + 1) or c.ndim != 2 or c.shape[1] != m + 1:
        raise ValueError('c must be n* x (m + 1) and G (m + 1) x (m + 1)')
    Phi = numpy.asarray(Phi_star, dtype=float).reshape(c.shape[0], -1)
    if Phi.shape[1] != m:
        raise ValueError('Phi_star must be n* x %d' % m)
    if m == 0:
        return numpy.empty((c.shape[0], 0))
    r = Phi - c[:, :m]
    LB = numpy.linalg.cholesky(G[:m, :m])
    return numpy.ascontiguousarray(solve_triangular(LB, r.T, lower=True).T)


class ProfileLikelihood(object):

    @staticmethod
    def log_likelihood(z, X, K_mixed, sign_switch, hyperparam):
        sigma, eta = hyperparam[0], hyperparam[1]
        n, m = X.shape
        if hasattr(K_mixed, 'loglik_terms'):
            ld, G = K_mixed.loglik_terms([eta], X, z)
            ld, G = ld[0], G[0]
            Gxx, gxz, gzz = G[:m, :m], G[:m, m], G[m, m]
            logdet_B = numpy.log(numpy.linalg.det(Gxx))
            zMz = gzz - gxz @ numpy.linalg.solve(Gxx, gxz)
        else:
            ld = K_mixed.logdet(eta)
            Y = K_mixed.solve(eta, X)
            w = K_mixed.solve(eta, z)
            B = X.T @ Y
            logdet_B = numpy.log(numpy.linalg.det(B))
            zMz = numpy.dot(z, w - Y @ (numpy.linalg.inv(B) @ (Y.T @ z)))
        lp = -0.5 * (n - m) * numpy.log(sigma ** 2) - 0.5 * ld - 0.5 * logdet_B \
            - (0.5 / (sigma ** 2)) * zMz
        return -lp if sign_switch else lp

    @staticmethod
    def _mz(z, X, K_mixed, eta):
        Y = K_mixed.solve(eta, X)
        w = K_mixed.solve(eta, z)
        Binv = numpy.linalg.inv(X.T @ Y)
        return Y, Binv, w - Y @ (Binv @ (Y.T @ z))

    @staticmethod
    def log_likelihood_der1_eta(z, X, K_mixed, log_eta):           # :91-132
        eta = 0.0 if numpy.isneginf(log_eta) else 10.0 ** log_eta
        n, m = X.shape
        if _use_band(K_mixed):
            return float(ProfileLikelihood.log_likelihood_der1_eta_batch(z, X, K_mixed,
                                                                         [log_eta])[0])
        Y, Binv, Mz = ProfileLikelihood._mz(z, X, K_mixed, eta)
        trace_M = K_mixed.traceinv(eta) - numpy.trace(Binv @ (Y.T @ Y))
        zMz = numpy.dot(z, Mz)
        zM2z = numpy.dot(Mz, Mz)
        sigma02 = zMz / (n - m)
        return -0.5 * (trace_M - zM2z / sigma02)

    @staticmethod
    def log_likelihood_der1_eta_batch(z, X, K_mixed, log_etas):
        """der1 at many log10(eta) in one device call (dense eigenvalue
        operator; otherwise one log_likelihood_der1_eta per point)."""
        log_etas = numpy.atleast_1d(numpy.asarray(log_etas, dtype=float))
        if not _use_band(K_mixed):
            return numpy.array([ProfileLikelihood.log_likelihood_der1_eta(z, X, K_mixed, le)
                                for le in log_etas])
        n, m = X.shape
        etas = numpy.where(numpy.isneginf(log_etas), 0.0, 10.0 ** log_etas)
        _, G1, G2, G3, tr1 = K_mixed.der_terms(etas, X, z, traceinv=True)
        return numpy.array([_der_from_terms(n, m, G1[i], G2[i], G3[i], tr1[i])[0]
                            for i in range(etas.size)])

    @staticmethod
    def log_likelihood_der1_scale(z, X, K_mixed, eta, **kernel_params):
        """Gradient of the likelihood profiled over sigma in the correlation scale rho
        (one entry per point dimension) at ``eta``, analytic: one factorization and one
        fused device pass (MixedCorrelation.scale_grad_terms, _scale_grad_from_terms),
        not 2 d re-assemblies and factorizations. ``kernel_params``: points,
        correlation_scale and nu for an ndarray K. -> array (d)."""
        X = numpy.asarray(X, dtype=float)
        n, m = X.shape
        T = K_mixed.scale_grad_terms(eta, X, z, **kernel_params)
        return _scale_grad_from_terms(n, m, T['t'], T['qX'], T['qc'], T['G'])

    @staticmethod
    def log_likelihood_der2_eta(z, X, K_mixed, eta):               # :138-192
        n, m = X.shape
        if _use_band(K_mixed):
            _, G1, G2, G3, tr1, tr2 = K_mixed.der_terms([eta], X, z, traceinv=2)
            return float(_der_from_terms(n, m, G1[0], G2[0], G3[0], tr1[0], tr2[0])[1])
        Y, Binv, Mz = ProfileLikelihood._mz(z, X, K_mixed, eta)
        V = K_mixed.solve(eta, Y)
        A = Binv @ (Y.T @ Y)
        trace_M = K_mixed.traceinv(eta) - numpy.trace(A)
        trace_M2 = K_mixed.traceinv(eta, exponent=2) - \
            2.0 * numpy.trace(Binv @ (Y.T @ V)) + numpy.trace(A @ A)
        MMz = K_mixed.solve(eta, Mz) - Y @ (Binv @ (Y.T @ Mz))
        zMz = numpy.dot(z, Mz)
        zM3z = numpy.dot(Mz, MMz)
        sigma02 = zMz / (n - m)
        return (0.5 / sigma02) * ((trace_M2 / (n - m) + (trace_M / (n - m)) ** 2) * zMz -
                                  2.0 * zM3z)

    @staticmethod
    def maximize_log_likelihood_with_sigma_eta(z, X, K_mixed, tol=1e-6,
                                               hyperparam_guess=[0.1, 0.1],
                                               method='Nelder-Mead'):   # :198-238
        print('Maximize log likelihood with sigma eta ...')
        f = partial(ProfileLikelihood.log_likelihood, z, X, K_mixed, True)
        res = minimize(f, hyperparam_guess, method='Nelder-Mead', tol=tol)
        print('Iter: %d, Eval: %d, success: %s' % (res.nit, res.nfev, res.success))
        sigma, eta = res.x[0], res.x[1]
        return {'sigma': sigma, 'sigma0': numpy.sqrt(eta) * sigma, 'eta': eta,
                'max_lp': -res.fun}

    @staticmethod
    def find_log_likelihood_der1_zeros(z, X, K_mixed, interval_eta, tol=1e-6,
                                       max_iterations=100, num_bracket_trials=3,
                                       group=False, speculative=None):  # :244-415
        """Root of d lp / d eta in log10(eta) (reference :244-415: bracket search,
        then Chandrupatla, then the optimal sigma). The der1 evaluations are
        batched: the bracket search requests every point it may need next in one
        call (_root_finding.find_interval_with_sign_change_batched), sharded over
        the ranks of a torch.distributed ``group`` when the caller passes one
        (sweep.der1_sweep: one all-gather per batch; every rank must hold the
        same K, X, z, so sharding is opt-in: the default False keeps the search
        on the local device). Chandrupatla's iterations are speculative: each
        device call also evaluates up to ``speculative`` points the next
        iterations may need (_root_finding._chandrupatla_candidates; default 64
        on the band operator, where a batch of eta costs one banded Cholesky's
        latency, else 0). Decisions and results are those of the sequential
        reference driver."""
        n, m = X.shape

        def optimal_sigma(eta):
            if hasattr(K_mixed, 'loglik_terms') and eta > 0:
                _, G = K_mixed.loglik_terms([eta], X, z)
                G = G[0]
                zMz = G[m, m] - G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m])
                return numpy.sqrt(zMz / (n - m))
            Y, Binv, Mz = ProfileLikelihood._mz(z, X, K_mixed, eta)
            return numpy.sqrt(numpy.dot(z, Mz) / (n - m))

        def optimal_sigma0():
            Binv = numpy.linalg.inv(X.T @ X)
            v = X @ (Binv @ (X.T @ z))
            return numpy.sqrt(numpy.dot(z, z - v) / (n - m))

        from ..sweep import der1_sweep
        if speculative is None:
            speculative = 64 if _use_band(K_mixed) else 0
        fb = BatchedFunction(lambda le: der1_sweep(K_mixed, X, z, le, group=group),
                             spec_budget=speculative)
        print('Find root of log likelihood derivative ...')
        bracket = [numpy.log10(interval_eta[0]), numpy.log10(interval_eta[1])]
        found, bracket, values = find_interval_with_sign_change_batched(
            fb, bracket, num_bracket_trials, tol=tol)
        if found:
            res = chandrupatla_method(fb, bracket, values, verbose=False, eps_m=tol,
                                      eps_a=tol, maxiter=max_iterations)
            print('Iter: %d' % (res['iterations']))
            eta = 10 ** res['root']
            sigma = optimal_sigma(eta)
            sigma0 = numpy.sqrt(eta) * sigma
            success = True
        else:
            d2 = ProfileLikelihood.log_likelihood_der2_eta(z, X, K_mixed, 0.0)
            left, right = values[0], values[1]
            print('dL/deta   at eta = %0.2e:\t %0.2f' % (bracket[0], left))
            print('dL/deta   at eta = %0.2e:\t %0.16f' % (bracket[1], right))
            print('d2L/deta2 at eta = 0.0:\t %0.2f' % d2)
            eta = None
            if left > 0 and right > 0:
                eta = 0.0 if d2 > 0 else numpy.inf
            elif left < 0 and right < 0:
                eta = 0.0 if d2 < 0 else numpy.inf
            if eta == 0:
                sigma0 = 0
                sigma = optimal_sigma(eta)
            elif eta == numpy.inf:
                sigma = 0
                sigma0 = optimal_sigma0()
            else:
                raise ValueError('eta must be zero or inf at this point.')
            success = True
        ProfileLikelihood.last_der1_calls = (fb.calls, fb.points, dict(fb.memo))
        # the largest eta batch of one device call (<= 64: the band operator's
        # cyclic-reduction path, gpmi_band_der_terms)
        ProfileLikelihood.last_der1_max_batch = fb.max_points
        return {'sigma': sigma, 'sigma0': sigma0, 'eta': eta, 'success': success}
