"""numpy statements of the expected information, shared by test_fisher_algebra (CPU) and
test_gpu_fisher: the second-order terms the device returns, the information by the direct
formula with the explicit REML projector, and the expected score whose derivative it is.
theta = (sigma, sigma0, rho_1 .. rho_d); Sigma = sigma^2 K(rho) + sigma0^2 I.
"""
import numpy

import _scale_grad_ref as sref


def terms(K, dK, X, z, eta):
    """-> dict(T, U, V, t, trinv, sol, G) as MixedCorrelation.fisher_terms returns: with
    A = K + eta I, N = [I, dK_1 .. dK_d], S = A^-1 [X z], Y_a = N_a S:
    T[a, b] = tr(A^-1 N_a A^-1 N_b), U[a] = S^T Y_a, V[a, b] = Y_a^T A^-1 Y_b."""
    n = K.shape[0]
    Ai = numpy.linalg.inv(K + eta * numpy.eye(n))
    Ai = 0.5 * (Ai + Ai.T)
    R = numpy.column_stack([X, z])
    S = Ai @ R
    N = [numpy.eye(n)] + list(dK)
    M = [Ai @ Na for Na in N]
    Y = [Na @ S for Na in N]
    d1 = len(N)
    T = numpy.array([[numpy.sum(M[a] * M[b].T) for b in range(d1)] for a in range(d1)])
    U = numpy.array([S.T @ Y[a] for a in range(d1)])
    V = numpy.array([[Y[a].T @ Ai @ Y[b] for b in range(d1)] for a in range(d1)])
    return {'T': T, 'U': U, 'V': V, 't': numpy.array([numpy.trace(Ma) for Ma in M[1:]]),
            'trinv': float(numpy.trace(Ai)), 'sol': S, 'G': R.T @ S}


def _sigma(pts, nu, theta):
    sigma, sigma0, rho = theta[0], theta[1], theta[2:]
    n = pts.shape[0]
    return sigma ** 2 * sref.correlation(pts, rho, nu) + sigma0 ** 2 * numpy.eye(n)


def _dsigma(pts, nu, theta):
    sigma, sigma0, rho = theta[0], theta[1], theta[2:]
    n = pts.shape[0]
    return [2.0 * sigma * sref.correlation(pts, rho, nu), 2.0 * sigma0 * numpy.eye(n)] + \
        [sigma ** 2 * D for D in sref.dcorrelation(pts, rho, nu)]


def projector(Sig, X):
    """P = Sig^-1 - Sig^-1 X (X^T Sig^-1 X)^-1 X^T Sig^-1 (Sig^-1 for no basis)."""
    Si = numpy.linalg.inv(Sig)
    Si = 0.5 * (Si + Si.T)
    if X.shape[1] == 0:
        return Si
    SX = Si @ X
    return Si - SX @ numpy.linalg.solve(X.T @ SX, SX.T)


def information(pts, nu, X, theta):
    """I_ab = tr(P Sig_a P Sig_b) / 2 by the formula, every matrix formed."""
    theta = numpy.asarray(theta, dtype=float)
    P = projector(_sigma(pts, nu, theta), X)
    PD = [P @ D for D in _dsigma(pts, nu, theta)]
    k = len(PD)
    return numpy.array([[0.5 * numpy.sum(PD[a] * PD[b].T) for b in range(k)] for a in range(k)])


def expected_score(pts, nu, X, theta, theta0):
    """E_theta0[score_a(theta)] = -tr(P Sig_a) / 2 + tr(P Sig_a P Sig(theta0)) / 2, P and
    Sig_a at theta (z ~ N(X beta, Sig(theta0)), and P X = 0)."""
    theta = numpy.asarray(theta, dtype=float)
    P = projector(_sigma(pts, nu, theta), X)
    S0 = _sigma(pts, nu, numpy.asarray(theta0, dtype=float))
    PS0 = P @ S0
    out = []
    for D in _dsigma(pts, nu, theta):
        PD = P @ D
        out.append(-0.5 * numpy.trace(PD) + 0.5 * numpy.sum(PD * PS0.T))
    return numpy.array(out)


def information_by_differences(pts, nu, X, theta0, step=1e-5):
    """I[a, b] = -d E_theta0[score_a(theta)] / d theta_b at theta0, central differences of
    step ``step`` theta_b."""
    theta0 = numpy.asarray(theta0, dtype=float)
    k = theta0.size
    out = numpy.empty((k, k))
    for b in range(k):
        h = step * theta0[b]
        tp, tm = theta0.copy(), theta0.copy()
        tp[b] += h
        tm[b] -= h
        out[:, b] = -(expected_score(pts, nu, X, tp, theta0)
                      - expected_score(pts, nu, X, tm, theta0)) / (tp[b] - tm[b])
    return out
