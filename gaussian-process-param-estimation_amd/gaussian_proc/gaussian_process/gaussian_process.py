"""Gaussian process user class (drop-in for
gaussian_proc/gaussian_process/gaussian_process.py:21-71), with the prediction
the reference leaves as a commented-out stub, joint posterior draws at new points,
and leave-one-out cross-validation of the fitted model."""

import numpy

from .._likelihood import Likelihood
from .._likelihood._profile_likelihood import _predict_from_terms, _predict_cov_from_terms, \
    _loo_from_terms, _cross_validation_scores

__all__ = ['GaussianProcess']


class GaussianProcess(object):
    """Gaussian process for regression with basis X (n x m) and correlation K
    (n x n ndarray, or a DeviceCorrelation from
    ``generate_correlation(..., device_resident=True)``)."""

    def __init__(self, X, K, likelihood_method='direct', device=None):
        self.X = X
        self.K = K
        self.likelihood = Likelihood(X, K, likelihood_method=likelihood_method,
                                     device=device)
        self.z = None
        self.results = None

    def train(self, z, plot=False):
        """Find the hyperparameters; prints the results dict (reference :154-162)
        and keeps it, with z, for ``predict``."""
        results = self.likelihood.maximize_log_likelihood(z, plot=plot)
        print(results)
        self.z = numpy.asarray(z, dtype=float).copy()
        self.results = results

    def scale_gradient(self, z=None, hyperparam=None, **kernel_params):
        """Gradient of the (direct, restricted) log-likelihood at
        ``hyperparam = (sigma, sigma0)`` in the correlation scale of K, one entry per
        point dimension, analytic (DirectLikelihood.log_likelihood_der1_scale). ``z``
        and ``hyperparam`` default to those of the last ``train`` or ``train_scale``;
        an ndarray K needs ``points``, ``correlation_scale`` and ``nu`` as keywords.
        -> array (d)."""
        from .._likelihood._direct_likelihood import DirectLikelihood
        if z is None:
            z = self.z
        if hyperparam is None and self.results is not None:
            hyperparam = (self.results['sigma'], self.results['sigma0'])
        if z is None or hyperparam is None:
            raise ValueError('scale_gradient needs z and hyperparam=(sigma, sigma0), or an '
                             'earlier train(z)')
        bad = sorted(set(kernel_params) - {'points', 'correlation_scale', 'nu'})
        if bad:
            raise TypeError('scale_gradient: unexpected keyword argument %s'
                            % ', '.join(map(repr, bad)))
        X = numpy.asarray(self.X, dtype=float)
        z = numpy.asarray(z, dtype=float)
        if z.shape != (X.shape[0],):
            raise ValueError('z must have %d entries' % X.shape[0])
        return DirectLikelihood.log_likelihood_der1_scale(z, X, self.likelihood.K_mixed,
                                                          hyperparam, **kernel_params)

    def fisher_information(self, z=None, hyperparam=None, **kernel_params):
        """The expected information of the (direct, restricted) likelihood at
        ``hyperparam = (sigma, sigma0)`` in theta = (sigma, sigma0, rho_1 .. rho_d), rho
        the correlation scale of K (DirectLikelihood.fisher_information): how well the
        data determine the fitted numbers, and the matrix of a Fisher-scoring step. ``z``
        and ``hyperparam`` default to those of the last ``train`` or ``train_scale``; an
        ndarray K needs ``points``, ``correlation_scale`` and ``nu`` as keywords.
        -> array (d + 2, d + 2), symmetric."""
        from .._likelihood._direct_likelihood import DirectLikelihood
        if z is None:
            z = self.z
        if hyperparam is None and self.results is not None:
            hyperparam = (self.results['sigma'], self.results['sigma0'])
        if z is None or hyperparam is None:
            raise ValueError('fisher_information needs z and hyperparam=(sigma, sigma0), or an '
                             'earlier train(z)')
        bad = sorted(set(kernel_params) - {'points', 'correlation_scale', 'nu'})
        if bad:
            raise TypeError('fisher_information: unexpected keyword argument %s'
                            % ', '.join(map(repr, bad)))
        X = numpy.asarray(self.X, dtype=float)
        z = numpy.asarray(z, dtype=float)
        if z.shape != (X.shape[0],):
            raise ValueError('z must have %d entries' % X.shape[0])
        return DirectLikelihood.fisher_information(z, X, self.likelihood.K_mixed, hyperparam,
                                                   **kernel_params)

    def hyperparam_covariance(self, z=None, hyperparam=None, **kernel_params):
        """The asymptotic covariance of the estimates of (sigma, sigma0, rho_1 .. rho_d):
        the inverse of ``fisher_information`` (same arguments). An information that is
        singular to working precision raises numpy.linalg.LinAlgError naming the cause:
        sigma0 = 0, where the likelihood is even in sigma0 and its row of the
        information is zero, or parameters the data do not separate.
        -> array (d + 2, d + 2), symmetric."""
        info = self.fisher_information(z=z, hyperparam=hyperparam, **kernel_params)
        names = ['sigma', 'sigma0'] + ['correlation_scale[%d]' % k
                                       for k in range(info.shape[0] - 2)]
        diag = numpy.diag(info)
        if not numpy.all(numpy.isfinite(info)):
            raise numpy.linalg.LinAlgError('the information is not finite')
        if numpy.any(diag <= 0.0):
            k = int(numpy.argmin(diag))
            why = ' (sigma0 = 0: the likelihood is even in sigma0, so its first derivative ' \
                  'carries no information there)' if k == 1 else ''
            raise numpy.linalg.LinAlgError('the information is singular: the data hold no '
                                           'information on %s%s' % (names[k], why))
        # in correlation form, so that the parameters' units do not decide the verdict
        s = 1.0 / numpy.sqrt(diag)
        w, Q = numpy.linalg.eigh(info * numpy.outer(s, s))
        if w[0] <= info.shape[0] * numpy.finfo(float).eps * w[-1]:
            worst = names[int(numpy.argmax(numpy.abs(Q[:, 0])))]
            raise numpy.linalg.LinAlgError('the information is singular to working precision: '
                                           'the data do not separate %s from the other '
                                           'parameters' % worst)
        cov = (Q / w) @ Q.T * numpy.outer(s, s)
        return 0.5 * (cov + cov.T)

    def standard_errors(self, z=None, hyperparam=None, **kernel_params):
        """The asymptotic standard errors of the estimates, the square roots of the
        diagonal of ``hyperparam_covariance`` (same arguments)
        -> dict(sigma, sigma0, correlation_scale (d))."""
        se = numpy.sqrt(numpy.diag(self.hyperparam_covariance(z=z, hyperparam=hyperparam,
                                                              **kernel_params)))
        return {'sigma': float(se[0]), 'sigma0': float(se[1]), 'correlation_scale': se[2:]}

    def train_scale(self, z, correlation_scale0=None, eta0=1.0, bounds=None, maxiter=100,
                    tol=1e-6):
        """Fit the correlation scale rho (one entry per point dimension) together with
        eta = (sigma0 / sigma)^2 by maximizing the likelihood profiled over sigma, on a
        device-resident K (a DeviceCorrelation; TypeError otherwise). L-BFGS-B over
        theta = (ln eta, ln rho_1 .. ln rho_d) with the analytic gradient (chain rule
        eta d/d eta, rho_k d/d rho_k): per evaluation K is re-assembled in place at rho
        (DeviceCorrelation.set_correlation_scale) and factorized once, on a 'cholesky'
        MixedCorrelation that drops what it cached from the old K. The start is
        ``correlation_scale0`` (default: K's scale) and ``eta0``; ``bounds`` =
        ((eta_lo, eta_hi), (rho_lo, rho_hi) per dimension) defaults to eta in
        [1e-6, 1e3] and rho_k in [1e-2, 10] times the range of the points in dimension
        k; ``tol`` is the projected-gradient tolerance (1e-3 ``tol`` the relative decrease
        of the likelihood that also ends the search). Leaves K at the fitted scale,
        rebuilds ``self.likelihood`` on it and keeps z and the results dict (sigma,
        sigma0, eta, correlation_scale, max_lp, iterations, evaluations, success), printed
        as ``train`` prints its own: ``predict``, ``sample`` and ``leave_one_out`` then
        work unchanged."""
        import scipy.optimize
        from ..generate_correlation.generate_correlation import DeviceCorrelation, \
            _broadcast_scale
        from .._mixed_correlation import MixedCorrelation
        from .._likelihood._profile_likelihood import _scale_grad_from_terms, \
            _eta_grad_from_terms
        K = self.K
        if not isinstance(K, DeviceCorrelation):
            raise TypeError('train_scale needs a device-resident K (generate_correlation(..., '
                            'device_resident=True)), whose scale it can re-assemble')
        X = numpy.asarray(self.X, dtype=float)
        n, m = X.shape
        z = numpy.asarray(z, dtype=float)
        if z.shape != (n,):
            raise ValueError('z must have %d entries' % n)
        d = K.points.shape[1]
        rho0 = K.correlation_scale if correlation_scale0 is None else \
            _broadcast_scale(K.points, correlation_scale0)
        rho0 = numpy.array(rho0, dtype=float)
        if not (numpy.all(rho0 > 0.0) and eta0 > 0.0):
            raise ValueError('correlation_scale0 and eta0 must be positive')
        if bounds is None:
            span = numpy.ptp(K.points, axis=0)
            span = numpy.where(span > 0.0, span, 1.0)
            bounds = [(1e-6, 1e3)] + [(1e-2 * s, 10.0 * s) for s in span]
        bounds = [(float(lo), float(hi)) for lo, hi in bounds]
        if len(bounds) != d + 1 or not all(0.0 < lo < hi for lo, hi in bounds):
            raise ValueError('bounds must be %d pairs 0 < lo < hi (eta, then one per dimension)'
                             % (d + 1))
        log_bounds = [(numpy.log(lo), numpy.log(hi)) for lo, hi in bounds]
        mc = MixedCorrelation(K, imate_method='cholesky')
        count = [0]

        def terms(theta):
            eta, rho = float(numpy.exp(theta[0])), numpy.exp(theta[1:])
            K.set_correlation_scale(rho)
            ld, G = mc.loglik_terms([eta], X, z)
            ld, G = float(ld[0]), G[0]
            zPz = G[m, m] - (G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m]) if m else 0.0)
            logdet_B = numpy.linalg.slogdet(G[:m, :m])[1] if m else 0.0
            s2 = zPz / (n - m)
            lp = -0.5 * (n - m) * numpy.log(s2) - 0.5 * ld - 0.5 * logdet_B - 0.5 * (n - m)
            return eta, rho, lp, s2

        def fun(theta):
            count[0] += 1
            eta, rho, lp, _ = terms(theta)
            T = mc.scale_grad_terms(eta, X, z)
            g_rho = _scale_grad_from_terms(n, m, T['t'], T['qX'], T['qc'], T['G'])
            g_eta = _eta_grad_from_terms(n, m, T['trinv'], T['sol'], T['G'])
            return -lp, -numpy.concatenate([[eta * g_eta], rho * g_rho])

        theta0 = numpy.concatenate([[numpy.log(eta0)], numpy.log(rho0)])
        theta0 = numpy.clip(theta0, [b[0] for b in log_bounds], [b[1] for b in log_bounds])
        res = scipy.optimize.minimize(fun, theta0, jac=True, method='L-BFGS-B',
                                      bounds=log_bounds,
                                      options={'maxiter': int(maxiter), 'gtol': float(tol),
                                               'ftol': 1e-3 * float(tol)})
        eta, rho, lp, s2 = terms(res.x)
        # K is left as a new DeviceCorrelation at the fitted scale would be, without the
        # factor of the last evaluation: what follows (predict, ...) then computes, bit
        # for bit, what it computes on a GaussianProcess built at that scale
        K.set_correlation_scale(rho)
        sigma = float(numpy.sqrt(s2))
        self.likelihood = Likelihood(self.X, K, likelihood_method=self.likelihood.likelihood_method,
                                     device=K.device)
        results = {'sigma': sigma, 'sigma0': float(numpy.sqrt(eta)) * sigma, 'eta': eta,
                   'correlation_scale': numpy.array(rho), 'max_lp': float(lp),
                   'iterations': int(res.nit), 'evaluations': int(count[0]),
                   'success': bool(res.success)}
        print(results)
        self.z = z.copy()
        self.results = results

    def predict(self, test_points, X_star, z=None, hyperparam=None, noise=False,
                return_var=True, return_cov=False, **kernel_params):
        """Posterior mean (and variance) at ``test_points`` (n* x d) with basis rows
        ``X_star`` (n* x m): universal kriging with the fitted or given
        ``hyperparam = (sigma, sigma0)``,
          mean = phi* beta + k*^T S^-1 (z - X beta),
          var  = sigma^2 (1 - k*^T S^-1 k* + r^T (X^T S^-1 X)^-1 r),
                 r = phi* - X^T S^-1 k*,  S = K + (sigma0 / sigma)^2 I,
        the variance of the latent function (``noise=True`` adds sigma0^2). ``z`` and
        ``hyperparam`` default to those of the last ``train``. The cross-correlation
        k* is assembled on the device from the kernel parameters of a
        DeviceCorrelation K; an ndarray K needs ``points``, ``correlation_scale``
        and ``nu`` (or ``cross``, the n* x n matrix itself) as keywords.
        ``return_cov=True`` returns the joint posterior covariance (n* x n*, exactly
        symmetric) in place of the variance,
          cov = sigma^2 (K** - K* S^-1 K*^T + r (X^T S^-1 X)^-1 r^T),
        ``noise=True`` adding sigma0^2 on its diagonal only; ``return_var`` is then
        ignored, and ``cross`` needs ``cross_star``, the n* x n* correlations of the
        new points with each other.
        -> mean, (mean, var) with ``return_var``, or (mean, cov) with ``return_cov``."""
        if z is None:
            z = self.z
        if hyperparam is None and self.results is not None:
            hyperparam = (self.results['sigma'], self.results['sigma0'])
        if z is None or hyperparam is None:
            raise ValueError('predict needs z and hyperparam=(sigma, sigma0), or an earlier '
                             'train(z)')
        bad = sorted(set(kernel_params) - {'points', 'correlation_scale', 'nu', 'cross',
                                           'cross_star'})
        if bad:
            raise TypeError('predict: unexpected keyword argument %s' % ', '.join(map(repr, bad)))
        sigma, sigma0 = float(hyperparam[0]), float(hyperparam[1])
        if not sigma > 0.0:
            raise ValueError('sigma must be positive')
        X = numpy.asarray(self.X, dtype=float)
        n, m = X.shape
        z = numpy.asarray(z, dtype=float)
        if z.shape != (n,):
            raise ValueError('z must have %d entries' % n)
        test_points = numpy.asarray(test_points, dtype=float)
        if test_points.ndim != 2 or test_points.shape[0] < 1:
            raise ValueError('test_points must be a 2D array (n*, dimension) with n* >= 1')
        X_star = numpy.asarray(X_star, dtype=float)
        if X_star.shape != (test_points.shape[0], m):
            raise ValueError('X_star must be %d x %d' % (test_points.shape[0], m))
        eta = (sigma0 / sigma) ** 2
        if return_cov:
            c, q, G, C0 = self.likelihood.K_mixed.predict_cov_terms(
                eta, X, z, test_points=test_points, **kernel_params)
            mean, _ = _predict_from_terms(c, q, G, X_star, sigma, sigma0, noise=noise)
            return mean, _predict_cov_from_terms(c, G, C0, X_star, sigma, sigma0, noise=noise)
        kernel_params.pop('cross_star', None)   # (only the covariance reads it)
        # (on a sparse K q costs a CG per block of new points: not asked for the mean alone)
        c, q, G = self.likelihood.K_mixed.predict_terms(eta, X, z, test_points=test_points,
                                                        return_q=bool(return_var),
                                                        **kernel_params)
        if q is None:
            q = numpy.zeros(c.shape[0])   # (the mean does not read q)
        mean, var = _predict_from_terms(c, q, G, X_star, sigma, sigma0, noise=noise)
        return (mean, var) if return_var else mean

    def sample(self, test_points, X_star, size=1, seed=0, z=None, hyperparam=None, noise=False,
               jitter=0.0, return_mean=False, xi=None, **kernel_params):
        """``size`` joint draws of the posterior at ``test_points`` (n* x d) with basis
        rows ``X_star`` (n* x m) -> (size, n*):
          draw = mean + sigma (L xi),   xi ~ N(0, I),
          L L^T = C0 + U U^T + (eta [noise] + jitter) I,   eta = (sigma0 / sigma)^2,
        C0 + U U^T the joint covariance of ``predict(return_cov=True)`` in units of
        sigma^2 (C0 = K** - K* S^-1 K*^T, U U^T = r (X^T S^-1 X)^-1 r^T) and mean its mean:
        the draws have exactly the covariance ``predict`` reports, ``noise=True``
        adding sigma0^2 on its diagonal. The covariance stays on the device, where it
        is factored and multiplied with the normals (MixedCorrelation.
        posterior_sample_terms). ``jitter`` (>= 0, in correlation units, default 0: none
        is invented) is added to the diagonal before the factorization; a covariance
        that is not numerically positive definite, such as that of duplicated test
        points with ``noise=False``, raises numpy.linalg.LinAlgError, and ``jitter=`` or
        ``noise=True`` are the remedies. The normals come from the device generator:
        draw j is a function of (``seed``, j) alone (gaussian_proc._normal.
        standard_normals states it); or ``xi`` (n* x size) supplies them.
        ``z``, ``hyperparam`` and the kernel keywords are those of ``predict``.
        -> draws, or (draws, mean) with ``return_mean``."""
        if z is None:
            z = self.z
        if hyperparam is None and self.results is not None:
            hyperparam = (self.results['sigma'], self.results['sigma0'])
        if z is None or hyperparam is None:
            raise ValueError('sample needs z and hyperparam=(sigma, sigma0), or an earlier '
                             'train(z)')
        bad = sorted(set(kernel_params) - {'points', 'correlation_scale', 'nu', 'cross',
                                           'cross_star'})
        if bad:
            raise TypeError('sample: unexpected keyword argument %s' % ', '.join(map(repr, bad)))
        sigma, sigma0 = float(hyperparam[0]), float(hyperparam[1])
        if not sigma > 0.0:
            raise ValueError('sigma must be positive')
        size = int(size)
        if size < 1:
            raise ValueError('size must be at least 1')
        jitter = float(jitter)
        if not jitter >= 0.0:
            raise ValueError('jitter must be non-negative')
        X = numpy.asarray(self.X, dtype=float)
        n, m = X.shape
        z = numpy.asarray(z, dtype=float)
        if z.shape != (n,):
            raise ValueError('z must have %d entries' % n)
        test_points = numpy.asarray(test_points, dtype=float)
        if test_points.ndim != 2 or test_points.shape[0] < 1:
            raise ValueError('test_points must be a 2D array (n*, dimension) with n* >= 1')
        nstar = test_points.shape[0]
        X_star = numpy.asarray(X_star, dtype=float)
        if X_star.shape != (nstar, m):
            raise ValueError('X_star must be %d x %d' % (nstar, m))
        if xi is not None:
            xi = numpy.asarray(xi, dtype=float)
            if xi.shape != (nstar, size):
                raise ValueError('xi must be %d x %d' % (nstar, size))
        eta = (sigma0 / sigma) ** 2
        c, G, draws = self.likelihood.K_mixed.posterior_sample_terms(
            eta, X, z, size=size, test_points=test_points, X_star=X_star,
            extra_eta=(eta if noise else 0.0) + jitter, seed=seed, first=0, xi=xi,
            **kernel_params)
        q = numpy.zeros(nstar)   # (the mean does not read q)
        mean, _ = _predict_from_terms(c, q, G, X_star, sigma, sigma0, noise=noise)
        draws *= sigma
        draws += mean[None, :]
        return (draws, mean) if return_mean else draws

    def _loo_args(self, z, hyperparam, who):
        """z and (sigma, sigma0), defaulting to the last train, checked. -> (X, z, sigma,
        sigma0)."""
        if z is None:
            z = self.z
        if hyperparam is None and self.results is not None:
            hyperparam = (self.results['sigma'], self.results['sigma0'])
        if z is None or hyperparam is None:
            raise ValueError('%s needs z and hyperparam=(sigma, sigma0), or an earlier '
                             'train(z)' % who)
        sigma, sigma0 = float(hyperparam[0]), float(hyperparam[1])
        if not sigma > 0.0:
            raise ValueError('sigma must be positive')
        X = numpy.asarray(self.X, dtype=float)
        n, m = X.shape
        if n <= m:
            raise ValueError('leave-one-out needs more points than basis functions '
                             '(n = %d, m = %d)' % (n, m))
        z = numpy.asarray(z, dtype=float)
        if z.shape != (n,):
            raise ValueError('z must have %d entries' % n)
        return X, z, sigma, sigma0

    def leave_one_out(self, z=None, hyperparam=None, noise=True, return_var=True):
        """Leave-one-out cross-validation in closed form: for every training point i
        the prediction of z_i, and its variance, from the other n - 1 points, with
        ``hyperparam = (sigma, sigma0)`` kept and beta re-estimated without point i
        (what ``predict`` on the reduced data set would return at point i). With
        S = K + (sigma0 / sigma)^2 I and P = S^-1 - S^-1 X (X^T S^-1 X)^-1 X^T S^-1,
          mean_i = z_i - (P z)_i / P_ii,   var_i = sigma^2 / P_ii,
        the variance of the noisy observation z_i (``noise=False`` subtracts sigma0^2:
        the latent function). One factorization and one pass over its triangular
        inverse on the device (MixedCorrelation.loo_terms), not n refits. ``z`` and
        ``hyperparam`` default to those of the last ``train``.
        -> mean, or (mean, var) with ``return_var``."""
        X, z, sigma, sigma0 = self._loo_args(z, hyperparam, 'leave_one_out')
        dinv, sol, G = self.likelihood.K_mixed.loo_terms((sigma0 / sigma) ** 2, X, z)
        mean, var = _loo_from_terms(dinv, sol, G, z, sigma, sigma0, noise=noise)
        return (mean, var) if return_var else mean

    def cross_validate(self, z=None, hyperparam=None):
        """Leave-one-out scores of the fitted model -> dict with 'residual'
        (z - mean), 'standardized' (residual / sqrt(var), the noisy variance), 'rmse',
        'mean_squared_standardized' (about 1 for a well-calibrated model) and
        'log_pseudo_likelihood' = sum_i -log(2 pi var_i) / 2 - residual_i^2 / (2 var_i).
        Arguments as ``leave_one_out``."""
        X, z, sigma, sigma0 = self._loo_args(z, hyperparam, 'cross_validate')
        mean, var = self.leave_one_out(z=z, hyperparam=(sigma, sigma0), noise=True)
        return _cross_validation_scores(z, mean, var)
