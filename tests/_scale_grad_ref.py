"""numpy statements of the correlation-scale gradient, shared by test_scale_grad_algebra
(CPU) and test_gpu_scale_grad: the Matérn correlation and its derivative in the scale, the
terms the device returns, and the two log-likelihoods the gradient belongs to.
"""
import numpy


def _u(pts, rho):
    """u[k, i, j] = (p_i - p_j)_k / rho_k, and x = |u|."""
    u = (pts[:, None, :] - pts[None, :, :]) / numpy.asarray(rho, dtype=float)[None, None, :]
    u = numpy.moveaxis(u, 2, 0)
    return u, numpy.sqrt(numpy.sum(u * u, axis=0))


def correlation(pts, rho, nu):
    _, x = _u(pts, rho)
    if nu == 0.5:
        return numpy.exp(-x)
    if nu == 1.5:
        return (1.0 + numpy.sqrt(3.0) * x) * numpy.exp(-numpy.sqrt(3.0) * x)
    if nu == 2.5:
        return (1.0 + numpy.sqrt(5.0) * x + 5.0 / 3.0 * x * x) * numpy.exp(-numpy.sqrt(5.0) * x)
    assert nu >= 100
    return numpy.exp(-0.5 * x * x)


def dcorrelation(pts, rho, nu):
    """dK[k] = dK / d rho_k = h(x) u_k^2 / rho_k, h = -M'(x) / x; zero where x = 0."""
    u, x = _u(pts, rho)
    if nu == 0.5:
        with numpy.errstate(divide='ignore', invalid='ignore'):
            h = numpy.where(x > 0.0, numpy.exp(-x) / x, 0.0)
    elif nu == 1.5:
        h = 3.0 * numpy.exp(-numpy.sqrt(3.0) * x)
    elif nu == 2.5:
        h = 5.0 / 3.0 * (1.0 + numpy.sqrt(5.0) * x) * numpy.exp(-numpy.sqrt(5.0) * x)
    else:
        assert nu >= 100
        h = numpy.exp(-0.5 * x * x)
    return h[None] * u * u / numpy.asarray(rho, dtype=float)[:, None, None]


def terms(K, dK, X, z, eta):
    """-> dict(t, qX, qc, trinv, sol, G) as MixedCorrelation.scale_grad_terms returns."""
    n, m = X.shape
    Ai = numpy.linalg.inv(K + eta * numpy.eye(n))
    Ai = 0.5 * (Ai + Ai.T)
    R = numpy.column_stack([X, z])
    sol = Ai @ R
    G = R.T @ sol
    c = numpy.ones(m + 1)
    CX = numpy.zeros((m + 1, m + 1))
    if m:
        CX[:m, :m] = numpy.linalg.inv(G[:m, :m])
        c[:m] = -numpy.linalg.solve(G[:m, :m], G[:m, m])
    w = sol @ c
    EX = sol @ CX @ sol.T
    return {'t': numpy.array([numpy.sum(Ai * D) for D in dK]),
            'qX': numpy.array([numpy.sum(EX * D) for D in dK]),
            'qc': numpy.array([w @ D @ w for D in dK]),
            'trinv': float(numpy.trace(Ai)), 'sol': sol, 'G': G}


def _parts(K, X, z, eta):
    n, m = X.shape
    A = K + eta * numpy.eye(n)
    ld = numpy.linalg.slogdet(A)[1]
    R = numpy.column_stack([X, z])
    G = R.T @ numpy.linalg.solve(A, R)
    zPz = G[m, m] - (G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m]) if m else 0.0)
    ldB = numpy.linalg.slogdet(G[:m, :m])[1] if m else 0.0
    return n, m, ld, ldB, zPz


def direct_lp(K, X, z, sigma, sigma0):
    """The restricted log-likelihood at (sigma, sigma0) (DirectLikelihood.log_likelihood)."""
    n, m, ld, ldB, zPz = _parts(K, X, z, (sigma0 / sigma) ** 2)
    s2 = sigma ** 2
    return -0.5 * (n - m) * numpy.log(2 * numpy.pi) - 0.5 * (n * numpy.log(s2) + ld) \
        - 0.5 * (ldB - m * numpy.log(s2)) - 0.5 * zPz / s2


def profiled_lp(K, X, z, eta):
    """... profiled over sigma: sigma^2 = z^T P z / (n - m), constants dropped."""
    n, m, ld, ldB, zPz = _parts(K, X, z, eta)
    return -0.5 * (n - m) * numpy.log(zPz / (n - m)) - 0.5 * ld - 0.5 * ldB


def central_differences(f, rho, step=1e-5):
    """d f / d rho_k by central differences of step ``step`` rho_k."""
    rho = numpy.asarray(rho, dtype=float)
    g = numpy.empty(rho.size)
    for k in range(rho.size):
        h = step * rho[k]
        rp, rm = rho.copy(), rho.copy()
        rp[k] += h
        rm[k] -= h
        g[k] = (f(rp) - f(rm)) / (rp[k] - rm[k])
    return g
