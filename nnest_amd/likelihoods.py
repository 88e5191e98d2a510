"""Analytic test likelihoods with the reference's host protocol (nnest/likelihoods.py:7-22):
`like(x[N,D] or x[D]) -> logl`, `.x_dim`, `.num_evaluations`.  The host evaluation is vectorised numpy in
the dtype of the input (it is what the reference's Python row loop computes, used for the initial live
points, nested.py:228).  `hip_like_id` tells the sampler that the same function exists inside the fused
HIP kernels (include/nnest_hip.h NNEST_LIKE_*), which is where the MCMC evaluations happen."""
import numpy as np
import scipy.special

from . import _lib
from ._lib import LIKE_IDS


class Likelihood(object):
    num_derived = 0
    hip_like_id = None
    hip_like_params = ()

    def __init__(self, x_dim):
        self.x_dim = x_dim
        self.num_evaluations = 0

    def __call__(self, x):
        if isinstance(x, list):
            x = np.array(x)
        if x.ndim > 1:
            self.num_evaluations += x.shape[0]
            return self.loglike_rows(x)
        self.num_evaluations += 1
        return self.loglike_rows(x[None, :])[0]

    def loglike(self, x):
        return self.loglike_rows(np.asarray(x)[None, :])[0]

    def loglike_rows(self, x):
        raise NotImplementedError


class Rosenbrock(Likelihood):
    """likelihoods.py:48-59"""
    hip_like_id = LIKE_IDS['rosenbrock']

    def loglike_rows(self, x):
        # the reference adds the terms with Python's `sum`, i.e. left to right in the dtype of x (likelihoods.py:51); cumsum
        # is numpy's left-to-right accumulation (np.sum would add pairwise: other bits in float32 from 8 terms on)
        terms = 100.0 * (x[:, 1:] - x[:, :-1] ** 2.0) ** 2.0 + (1 - x[:, :-1]) ** 2.0
        return -np.cumsum(terms, axis=1)[:, -1]

    @property
    def max_loglike(self):
        return self(np.ones((self.x_dim,)))


class Himmelblau(Likelihood):
    """likelihoods.py:62-74 for x_dim = 2.  For even x_dim > 2 (BASELINE config 4 names x_dim=32, which the
    reference cannot run: it asserts x_dim == 2) the build-defined generalisation is the sum of the 2-D
    function over consecutive pairs (x[2i], x[2i+1]); it reduces to the reference at x_dim = 2."""
    hip_like_id = LIKE_IDS['himmelblau']

    def __init__(self, x_dim=2):
        assert x_dim >= 2 and x_dim % 2 == 0
        super(Himmelblau, self).__init__(x_dim)

    def loglike_rows(self, x):
        a, b = x[:, 0::2], x[:, 1::2]
        return np.sum(-(a ** 2 + b - 11.) ** 2 - (a + b ** 2 - 7.) ** 2, axis=1)

    @property
    def max_loglike(self):
        return self(np.array([3.0, 2.0] * (self.x_dim // 2)))


class GaussianMix(Likelihood):
    """likelihoods.py:165-193 with the defaults the fused kernel implements: sep=4, sigma=1, weights
    (0.4, 0.3, 0.2, 0.1)."""
    hip_like_id = LIKE_IDS['gaussmix']

    def __init__(self, x_dim, sep=4, weights=(0.4, 0.3, 0.2, 0.1), sigma=1):
        assert len(weights) in [2, 3, 4] and np.isclose(sum(weights), 1)
        super(GaussianMix, self).__init__(x_dim)
        self.sep, self.weights, self.sigma = sep, tuple(weights), sigma
        if not (sep == 4 and sigma == 1 and tuple(weights) == (0.4, 0.3, 0.2, 0.1)):
            self.hip_like_id = None  # only the defaults are in the kernel; other settings run on the host protocol
        pos = [(0, sep), (0, -sep), (sep, 0), (-sep, 0)]
        self.positions = [np.asarray(p) for p in pos[:len(weights)]]

    def loglike_rows(self, x):
        # operation for operation what the reference does per row (likelihoods.py:153-162, :182-189): shift the first two
        # coordinates, square, np.sum over the row in the dtype of x, then float64 constants and scipy's logsumexp
        x = np.asarray(x)
        ls = []
        for w, p in zip(self.weights, self.positions):
            d = np.array(x, copy=True)
            d[:, :2] -= p
            logl = -(np.sum(d ** 2, axis=1) / (2 * self.sigma ** 2))
            logl = logl - np.log(2 * np.pi * (self.sigma ** 2)) * self.x_dim / 2.0
            ls.append(logl + np.log(w))
        return scipy.special.logsumexp(np.stack(ls, axis=0), axis=0)

    @property
    def max_loglike(self):
        v = np.zeros(self.x_dim)
        v[:2] = self.positions[int(np.argmax(self.weights))]
        return self(v)


class Gaussian(Likelihood):
    """likelihoods.py:77-94: N(0, Sigma), Sigma = I + corr (11^T - I).  Evaluated in closed form (Sherman-Morrison
    for the equicorrelated covariance) instead of scipy's Cholesky; same float64 arithmetic domain."""
    hip_like_id = LIKE_IDS['gaussian']

    def __init__(self, x_dim, corr, lim=5):
        super(Gaussian, self).__init__(x_dim)
        self.corr, self.lim = corr, lim
        self.hip_like_params = (corr,)

    def loglike_rows(self, x):
        x = np.asarray(x, dtype=np.float64)
        D, c = self.x_dim, self.corr
        s1, s2 = np.sum(x, axis=1), np.sum(x * x, axis=1)
        quad = (s2 - c * s1 * s1 / (1.0 + (D - 1.0) * c)) / (1.0 - c)
        logdet = (D - 1.0) * np.log(1.0 - c) + np.log(1.0 + (D - 1.0) * c)
        return -0.5 * quad - 0.5 * logdet - 0.5 * D * np.log(2 * np.pi)

    @property
    def max_loglike(self):
        return self(np.zeros(self.x_dim))


class Eggbox(Likelihood):
    """likelihoods.py:97-110 (x_dim = 2)"""
    hip_like_id = LIKE_IDS['eggbox']

    def __init__(self, x_dim=2):
        assert x_dim == 2
        super(Eggbox, self).__init__(x_dim)

    def loglike_rows(self, x):
        chi = np.cos(x[:, 0] / 2.) * np.cos(x[:, 1] / 2.)
        return (2. + chi) ** 5

    @property
    def max_loglike(self):
        return self(np.zeros(2))


class GaussianShell(Likelihood):
    """likelihoods.py:113-132 (the fused kernel takes a scalar centre)"""
    hip_like_id = LIKE_IDS['shell']

    def __init__(self, x_dim, sigma=0.1, rshell=2, center=0):
        super(GaussianShell, self).__init__(x_dim)
        self.sigma, self.rshell = sigma, rshell
        if hasattr(center, '__len__'):
            self.center = np.asarray(center, dtype=np.float64)
            if np.ptp(self.center) != 0:
                self.hip_like_id = None
            c0 = float(self.center[0])
        else:
            self.center = np.full(x_dim, float(center))
            c0 = float(center)
        self.hip_like_params = (sigma, rshell, c0)

    def loglike_rows(self, x):
        rad = np.sqrt(np.sum((self.center - np.asarray(x, dtype=np.float64)) ** 2, axis=1))
        return -((rad - self.rshell) ** 2) / (2 * self.sigma ** 2)

    @property
    def max_loglike(self):
        return 0.0


class DoubleGaussianShell(Likelihood):
    """likelihoods.py:135-150"""
    hip_like_id = LIKE_IDS['double_shell']

    def __init__(self, x_dim, sigmas=(0.1, 0.1), rshells=(2, 2), centers=(-4, 4), weights=(1.0, 1.0)):
        super(DoubleGaussianShell, self).__init__(x_dim)
        self.shell1 = GaussianShell(x_dim, sigma=sigmas[0], rshell=rshells[0], center=centers[0])
        self.shell2 = GaussianShell(x_dim, sigma=sigmas[1], rshell=rshells[1], center=centers[1])
        self.weights = tuple(weights)
        # (a sub-shell with a vector centre of unequal entries is not the kernel's: it cleared its own id, and so does the pair;
        # the centres go to the kernel as the scalars the sub-shells made of them)
        if self.weights != (1.0, 1.0) or self.shell1.hip_like_id is None or self.shell2.hip_like_id is None:
            self.hip_like_id = None
        self.hip_like_params = self.shell1.hip_like_params + self.shell2.hip_like_params

    def loglike_rows(self, x):
        return np.logaddexp(np.log(self.weights[0]) + self.shell1.loglike_rows(x),
                            np.log(self.weights[1]) + self.shell2.loglike_rows(x))


class GaussianData(Likelihood):
    """A multivariate Gaussian whose mean and covariance come from the user's data (build-defined: the reference has none):
        logL(theta) = logl_max - 1/2 (theta - mean)^T P (theta - mean),
    P the precision matrix -- `precision`, or the inverse of `cov`; exactly one of the two is given.  A linear model with Gaussian
    noise (`from_linear_model`), a Fisher or Laplace approximation, a compressed data vector.  ValueError for a wrong shape, a
    non-finite entry, a matrix that is not symmetric positive definite, x_dim outside 1 .. 128.
    The host evaluation is float64 from P.  `hip_like_id` stays None -- no NNEST_LIKE_* id stands for this likelihood, and every
    route that keys on one treats the object as a Python callable --; `hip_like_data` carries what the fused Metropolis kernels of
    this likelihood take (include/nnest_hip.h nnest_gdata_t): mu float32 [D]; R float32 [D, D], upper triangular, the float32
    rounding of L^T with P = L L^T in float64; logl0 = logl_max."""
    MAX_DIM = 128

    def __init__(self, mean, cov=None, precision=None, logl_max=0.0):
        if (cov is None) == (precision is None):
            raise ValueError('GaussianData: exactly one of cov and precision')
        mean = np.array(mean, dtype=np.float64)
        if mean.ndim != 1 or not 1 <= mean.shape[0] <= self.MAX_DIM:
            raise ValueError('GaussianData: mean must be shaped [x_dim] with x_dim in 1 .. %d, got %s' % (self.MAX_DIM, mean.shape))
        D = mean.shape[0]
        what = 'cov' if precision is None else 'precision'
        M = np.array(cov if precision is None else precision, dtype=np.float64)
        if M.shape != (D, D):
            raise ValueError('GaussianData: %s must be shaped [%d, %d], got %s' % (what, D, D, M.shape))
        logl_max = float(logl_max)
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(M)) and np.isfinite(logl_max)):
            raise ValueError('GaussianData: mean, %s and logl_max must be finite' % what)
        # symmetric to float64 rounding: a few ulp of the entries' scale (a product such as A^T N^-1 A rounds its two triangles apart)
        if np.max(np.abs(M - M.T)) > 64 * np.finfo(np.float64).eps * np.max(np.abs(M)):
            raise ValueError('GaussianData: %s is not symmetric' % what)
        M = 0.5 * (M + M.T)
        try:
            np.linalg.cholesky(M)
            P = M if precision is not None else np.linalg.inv(M)
            P = 0.5 * (P + P.T)
            L = np.linalg.cholesky(P)
        except np.linalg.LinAlgError:
            raise ValueError('GaussianData: %s is not positive definite' % what)
        super(GaussianData, self).__init__(D)
        self.mean, self.precision, self.logl_max = mean, P, logl_max
        R = np.triu(L.T).astype(np.float32)   # (triu: exact zeros below the diagonal)
        self.hip_like_data = dict(mu=mean.astype(np.float32), R=R, logl0=logl_max)

    @classmethod
    def from_linear_model(cls, A, y, noise_cov):
        """the likelihood of theta in y = A theta + noise, noise ~ N(0, N): A [n, x_dim], y [n], noise_cov a scalar variance, a vector
        of n variances or an [n, n] covariance.  P = A^T N^-1 A, mean = P^-1 A^T N^-1 y, and logl_max the residual term, so that
        loglike(theta) = -1/2 (A theta - y)^T N^-1 (A theta - y) to float64 rounding.  ValueError when P is singular (the data do
        not determine theta)."""
        A = np.array(A, dtype=np.float64)
        y = np.array(y, dtype=np.float64)
        if A.ndim != 2 or y.shape != (A.shape[0],):
            raise ValueError('from_linear_model: A must be shaped [n, x_dim] and y [n], got %s and %s' % (A.shape, y.shape))
        n = A.shape[0]
        N = np.array(noise_cov, dtype=np.float64)
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(y)) and np.all(np.isfinite(N))):
            raise ValueError('from_linear_model: A, y and noise_cov must be finite')
        try:
            if N.ndim == 0 or N.shape == (n,):
                if not np.all(N > 0):
                    raise ValueError('from_linear_model: the noise variances must be positive')
                NiA, Niy = A / (N if N.ndim == 0 else N[:, None]), y / N
            elif N.shape == (n, n):
                c = np.linalg.cholesky(0.5 * (N + N.T))
                solve = lambda b: np.linalg.solve(c.T, np.linalg.solve(c, b))
                NiA, Niy = solve(A), solve(y)
            else:
                raise ValueError('from_linear_model: noise_cov must be a scalar, [n] or [n, n], got %s' % (N.shape,))
            P = A.T @ NiA
            P = 0.5 * (P + P.T)
            b = A.T @ Niy
            np.linalg.cholesky(P)
            if np.linalg.cond(P) > 1.0 / (64 * np.finfo(np.float64).eps):
                raise np.linalg.LinAlgError('singular')
            mean = np.linalg.solve(P, b)
        except np.linalg.LinAlgError:
            raise ValueError('from_linear_model: A^T N^-1 A is singular: the data do not determine theta (or noise_cov is not positive definite)')
        res = A @ mean - y
        return cls(mean, precision=P, logl_max=-0.5 * float(res @ (NiA @ mean - Niy)))   # (N^-1 (A mean - y))

    def loglike_rows(self, x):
        d = np.asarray(x, dtype=np.float64) - self.mean
        return self.logl_max - 0.5 * np.einsum('ni,ij,nj->n', d, self.precision, d)

    @property
    def max_loglike(self):
        return self.logl_max


class GLMData(Likelihood):
    """A generalised linear model of the user's data (build-defined: the reference has none): with the linear predictor
    eta_i = offset_i + sum_c A[i, c] theta_c over the n rows of the design matrix A [n, x_dim],
        family 'logistic': y_i in {0, 1},            logL = logl_const + sum_i -softplus((1 - 2 y_i) eta_i)
        family 'poisson':  y_i in {0, 1, 2, ...},    logL = logl_const + sum_i (y_i eta_i - exp(eta_i) - lgamma(y_i + 1))
    -- Bayesian logistic regression and Poisson regression with the log link, normalised.  ValueError for a wrong shape, a
    non-finite entry, a y the family does not take, x_dim outside 1 .. 128, n outside 1 .. 65536, an unknown family.
    The host evaluation is float64 from the float64 data (-1e100 where it is not finite, the kernels' rule).  `hip_like_id` stays
    None -- no NNEST_LIKE_* id stands for this likelihood, and every route that keys on one treats the object as a Python callable
    --; `hip_like_glm` carries what the fused Metropolis kernels of this likelihood take (include/nnest_hip.h nnest_glm_t): float32
    at [x_dim, ld] = A^T with ld = n rounded up to a multiple of 64, zero padded, y [ld], o [ld]; logl0 (Poisson: logl_const -
    sum_i lgamma(y_i + 1)); n; family."""
    MAX_DIM = 128
    MAX_ROWS = 65536
    FAMILIES = ('logistic', 'poisson')

    def __init__(self, A, y, family='logistic', offset=None, logl_const=0.0):
        if family not in self.FAMILIES:
            raise ValueError('GLMData: family=%r (one of %s)' % (family, ', '.join(self.FAMILIES)))
        A = np.array(A, dtype=np.float64)
        y = np.array(y, dtype=np.float64)
        if A.ndim != 2 or not 1 <= A.shape[1] <= self.MAX_DIM or not 1 <= A.shape[0] <= self.MAX_ROWS:
            raise ValueError('GLMData: A must be shaped [n, x_dim] with n in 1 .. %d and x_dim in 1 .. %d, got %s'
                             % (self.MAX_ROWS, self.MAX_DIM, A.shape))
        n, D = A.shape
        if y.shape != (n,):
            raise ValueError('GLMData: y must be shaped [%d], got %s' % (n, y.shape))
        o = np.zeros(n) if offset is None else np.array(offset, dtype=np.float64)
        if o.shape != (n,):
            raise ValueError('GLMData: offset must be shaped [%d], got %s' % (n, o.shape))
        logl_const = float(logl_const)
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(y)) and np.all(np.isfinite(o)) and np.isfinite(logl_const)):
            raise ValueError('GLMData: A, y, offset and logl_const must be finite')
        if family == 'logistic' and not np.all((y == 0) | (y == 1)):
            raise ValueError('GLMData: family logistic takes y in {0, 1}')
        if family == 'poisson' and not (np.all(y >= 0) and np.all(y == np.round(y)) and np.all(y < 2 ** 24)):
            raise ValueError('GLMData: family poisson takes y in {0, 1, 2, ...} (counts below 2^24: exact in float32)')
        super(GLMData, self).__init__(D)
        self.A, self.y, self.offset, self.family, self.logl_const = A, y, o, family, logl_const
        self.logl0 = logl_const - (float(np.sum(scipy.special.gammaln(y + 1.0))) if family == 'poisson' else 0.0)
        at, yy, oo = self.layout(A, y, o)
        self.hip_like_glm = dict(at=at, y=yy, o=oo, logl0=self.logl0, n=n, family=family)

    @staticmethod
    def layout(A, y, offset=None):
        """the float32 arrays of nnest_glm_t: A [n, D], y [n], offset [n] or None -> (at [D, ld] = A^T, y [ld], o [ld]), ld = n
        rounded up to a multiple of 64, zero padded"""
        A = np.asarray(A, np.float64)
        n, D = A.shape
        ld = (n + 63) // 64 * 64
        at = np.zeros((D, ld), np.float32)
        at[:, :n] = A.T
        yy = np.zeros(ld, np.float32)
        yy[:n] = np.asarray(y, np.float64)
        oo = np.zeros(ld, np.float32)
        if offset is not None:
            oo[:n] = np.asarray(offset, np.float64)
        return at, yy, oo

    def loglike_rows(self, x):
        with np.errstate(over='ignore', invalid='ignore'):
            eta = self.offset + np.asarray(x, dtype=np.float64) @ self.A.T
            if self.family == 'logistic':
                s = (1.0 - 2.0 * self.y) * eta
                terms = -(np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))))
            else:
                terms = self.y * eta - np.exp(eta)
            logl = self.logl0 + np.sum(terms, axis=1)
        return np.where(np.isfinite(logl), logl, -1e100)

    # ---- pointwise predictive statistics (build-defined: the reference has none; include/nnest_hip.h nnest_glm_pointwise) ----
    POINTWISE_CHUNK = 1 << 20        # draws per launch of the fused route
    POINTWISE_HOST_BYTES = 1 << 26   # the host route's [chunk, n] float64 block

    def _draws(self, samples, what):
        x = np.asarray(samples)
        if x.ndim == 3:
            x = x.reshape(-1, x.shape[-1])
        if x.ndim != 2 or x.shape[1] != self.x_dim:
            raise ValueError('%s: samples must be shaped [S, %d] or [N, steps, %d], got %s' % (what, self.x_dim, self.x_dim, np.shape(samples)))
        return x

    @staticmethod
    def _route(route, what):
        if route not in (None, 'host', 'fused'):
            raise ValueError("%s: route=%r: None, 'host' or 'fused'" % (what, route))
        if route is None:
            import torch
            route = 'fused' if torch.cuda.is_available() else 'host'
        return route

    @staticmethod
    def _moments(v, live):
        """(cnt, mean, M2) [n] of the live entries of v [S, n], float64, two passes"""
        cnt = live.sum(axis=0).astype(np.float64)
        safe = np.where(cnt > 0, cnt, 1.0)
        mean = np.where(live, v, 0.0).sum(axis=0) / safe
        M2 = np.where(live, (np.where(live, v, 0.0) - mean) ** 2, 0.0).sum(axis=0)
        return cnt, np.where(cnt > 0, mean, 0.0), np.where(cnt > 0, M2, 0.0)

    @classmethod
    def _pointwise_block(cls, l):
        """the eight statistics of nnest_glm_pointwise [n, 8] of a block of terms l [S, n]"""
        live = np.isfinite(l)
        out = _lib.empty_glm_pointwise(l.shape[1])
        with np.errstate(invalid='ignore', over='ignore'):
            for k, v in ((0, l), (2, -l)):
                m = np.max(np.where(live, v, -np.inf), axis=0, initial=-np.inf)
                e = np.where(live, np.exp(np.where(live, v, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
                out[:, k], out[:, k + 1] = m, e.sum(axis=0)
                if k == 2:
                    out[:, 4] = (e * e).sum(axis=0)
        out[:, 5], out[:, 6], out[:, 7] = cls._moments(l, live)
        return out

    def _row_terms(self, x, rows=slice(None)):
        """l [S, n] float64 from the float64 data (of the data rows `rows`), without the Poisson lgamma (NaN where eta is not
        finite: the kernels' rule)"""
        y = self.y[rows]
        with np.errstate(over='ignore', invalid='ignore'):
            eta = self.offset[rows] + np.asarray(x, dtype=np.float64) @ self.A[rows].T
            if self.family == 'logistic':
                s = (1.0 - 2.0 * y) * eta
                l = -(np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))))
            else:
                l = y * eta - np.exp(eta)
        return np.where(np.isfinite(eta), l, np.nan)

    def pointwise_stats(self, samples, route=None, chunk=None):
        """the per-row statistics [n, 8] float64 (include/nnest_hip.h nnest_glm_pointwise: {a, P, b, Q, Q2, cnt, mean, M2}) of the
        draws `samples`, and the route taken; `pointwise` has the arguments"""
        x = self._draws(samples, 'GLMData.pointwise')
        route = self._route(route, 'GLMData.pointwise')
        n, S = self.A.shape[0], x.shape[0]
        stats = _lib.empty_glm_pointwise(n)
        if route == 'fused':
            import torch
            from . import flow
            chunk = max(1, min(int(self.POINTWISE_CHUNK if chunk is None else chunk), 1 << 30))
            dev = torch.device('cuda', torch.cuda.current_device())
            spec = {k: (torch.as_tensor(v).to(dev) if k in ('at', 'y', 'o') else v) for k, v in self.hip_like_glm.items()}
            for first in range(0, S, chunk):
                part = flow.glm_pointwise(spec, np.ascontiguousarray(x[first:first + chunk], dtype=np.float32), device=dev)
                stats = _lib.merge_glm_pointwise(stats, part.cpu().numpy())
        else:
            chunk = max(1, int(self.POINTWISE_HOST_BYTES // (8 * n) if chunk is None else chunk))
            for first in range(0, S, chunk):
                stats = _lib.merge_glm_pointwise(stats, self._pointwise_block(self._row_terms(x[first:first + chunk])))
        return stats, route

    def pointwise(self, samples, route=None, chunk=None, psis=False):
        """How well the model predicts each observation, from posterior draws (build-defined: the reference has none).  samples:
        [S, x_dim] or [N, steps, x_dim] (flattened) rows theta, as `sampler.samples` holds them, unweighted.  With l_is = log p(y_i |
        theta_s) and the sums over the LIVE draws of a row (l_is finite; a draw with a non-finite coordinate is dead for every row),
        returns a dict of float64 arrays of length n:
            lppd        log mean_s exp(l_is)                      the log pointwise predictive density
            p_waic      var_s l_is (n - 1 in the divisor)         WAIC's effective number of parameters; NaN below 2 live draws
            elpd_waic   lppd - p_waic
            elpd_isloo  -log mean_s exp(-l_is)                    leave-one-out by plain importance sampling (weights 1 / p(y_i | theta_s))
            isloo_ess   (sum_s w_is)^2 / sum_s w_is^2             the effective sample size of those weights
            mean_logl   mean_s l_is
            n_live      the live draws
        The Poisson -lgamma(y_i + 1) is added on the host to lppd, elpd_isloo and mean_logl: these are log p(y_i | .), normalised.
        PLAIN importance-sampled leave-one-out is UNRELIABLE for a row whose isloo_ess is small: its weights have a heavy tail there
        and elpd_isloo is then too high.  psis=True adds PARETO-SMOOTHED leave-one-out (PSIS-LOO; include/nnest_hip.h nnest_glm_psis
        and nnest_amd/psis.py have the definition, to the operation):
            elpd_psis   the leave-one-out density with the row's M largest weights replaced by the quantiles of a generalised
                        Pareto distribution fitted to them (Zhang & Stephens' fit, as loo::gpdfit), truncated at the largest raw one
            pareto_k    the fitted shape khat, the diagnostic: above min(1 - 1 / log10(S), 0.7) the row's estimate is unreliable
                        whatever the number of draws; +inf where the tail was too small for a fit (fewer than 5 values: elpd_psis is
                        then elpd_isloo), NaN where the fit failed
            psis_ess    the effective sample size of the smoothed weights
            psis_tail   M, the weights that were smoothed
            p_loo       lppd - elpd_psis
        All draws are resident at once there: at most 2^20 draws, and a bounded work buffer -- a ValueError above either: thin the run.
        With psis=False the dict is the one above, key for key.
        route: 'fused' -- the product on the matrix cores, the float64 term and the reduction over the draws inside one kernel
        (include/nnest_hip.h nnest_glm_pointwise), float32 data and draws, in launches of `chunk` draws merged by
        _lib.merge_glm_pointwise; 'host' -- the same statistics in chunked float64 numpy from the float64 data, no GPU needed; None
        -- 'fused' where a device is available.  The route taken is left in `pointwise_route`."""
        if not psis:
            stats, route = self.pointwise_stats(samples, route, chunk)
            self.pointwise_route = route
            return self.pointwise_from_stats(stats)
        from . import psis as _psis
        x = self._draws(samples, 'GLMData.pointwise')
        route = self._route(route, 'GLMData.pointwise')
        n, S = self.A.shape[0], x.shape[0]
        if S > _psis.MAX_DRAWS:
            raise ValueError('GLMData.pointwise: psis=True takes at most %d draws at once, got %d: thin the run' % (_psis.MAX_DRAWS, S))
        if route == 'fused':
            import torch
            from . import flow
            if _lib.load().nnest_glm_psis_work_bytes(S, n) < 0:
                raise ValueError('GLMData.pointwise: psis=True with %d draws of %d rows needs too large a work buffer: thin the run' % (S, n))
            dev = torch.device('cuda', torch.cuda.current_device())
            spec = {k: (torch.as_tensor(v).to(dev) if k in ('at', 'y', 'o') else v) for k, v in self.hip_like_glm.items()}
            stats, rows = flow.glm_psis(spec, np.ascontiguousarray(x, dtype=np.float32), device=dev)
            stats, rows = stats.cpu().numpy(), rows.cpu().numpy()
        else:
            stats, _ = self.pointwise_stats(x, 'host', chunk)
            rows = np.empty((n, _psis.SLOTS))
            step = max(1, int(self.POINTWISE_HOST_BYTES // (8 * max(S, 1))))
            for first in range(0, n, step):   # (blocks of data rows: the [S, rows] block of terms is what is held)
                rows[first:first + step] = _psis.psis_rows(self._row_terms(x, slice(first, first + step)))
        self.pointwise_route = route
        out = self.pointwise_from_stats(stats)
        norm = -scipy.special.gammaln(self.y + 1.0) if self.family == 'poisson' else np.zeros_like(self.y)
        out['elpd_psis'] = rows[:, _psis.ELPD] + norm
        out['pareto_k'] = rows[:, _psis.KHAT].copy()
        out['psis_ess'] = rows[:, _psis.ESS].copy()
        out['psis_tail'] = rows[:, _psis.M].copy()
        out['p_loo'] = out['lppd'] - out['elpd_psis']
        return out

    def log_lik(self, samples, route=None):
        """The pointwise log-likelihood matrix [S, n] float64, l_is = log p(y_i | theta_s), normalised (the Poisson -lgamma(y_i + 1)
        is added on the host), NaN for a dead pair: what other tools take for their own leave-one-out.  samples and route as
        `pointwise` takes them; 'fused' is nnest_glm_terms (float32 data and draws, the terms `pointwise` reduces, at most 2^30
        entries), 'host' float64 numpy.  The route taken is left in `log_lik_route`."""
        x = self._draws(samples, 'GLMData.log_lik')
        route = self._route(route, 'GLMData.log_lik')
        if route == 'fused':
            import torch
            from . import flow
            if x.shape[0] * self.A.shape[0] > 1 << 30:
                raise ValueError('GLMData.log_lik: %d draws of %d rows are more than 2^30 entries: thin the run' % (x.shape[0], self.A.shape[0]))
            dev = torch.device('cuda', torch.cuda.current_device())
            spec = {k: (torch.as_tensor(v).to(dev) if k in ('at', 'y', 'o') else v) for k, v in self.hip_like_glm.items()}
            l = flow.glm_terms(spec, np.ascontiguousarray(x, dtype=np.float32), device=dev).cpu().numpy()
        else:
            l = self._row_terms(x)
        self.log_lik_route = route
        if self.family == 'poisson':
            l = l - scipy.special.gammaln(self.y + 1.0)
        return l

    def pointwise_from_stats(self, stats):
        """`pointwise`'s dict from the statistics [n, 8]"""
        a, P, b, Q, Q2, cnt, mean, M2 = np.asarray(stats, np.float64).T
        norm = -scipy.special.gammaln(self.y + 1.0) if self.family == 'poisson' else np.zeros_like(self.y)
        with np.errstate(divide='ignore', invalid='ignore'):
            lppd = np.where(cnt > 0, a + np.log(P) - np.log(cnt) + norm, np.nan)   # (no live draw: nothing to average)
            p_waic = np.where(cnt >= 2, M2 / np.where(cnt >= 2, cnt - 1.0, 1.0), np.nan)
            isloo = np.where(cnt > 0, -(b + np.log(Q) - np.log(cnt)) + norm, np.nan)
            ess = np.where(Q2 > 0, Q * Q / np.where(Q2 > 0, Q2, 1.0), 0.0)
        return dict(lppd=lppd, p_waic=p_waic, elpd_waic=lppd - p_waic, elpd_isloo=isloo, isloo_ess=ess,
                    mean_logl=np.where(cnt > 0, mean + norm, np.nan), n_live=cnt)

    def predict(self, samples, A_new, offset_new=None, route=None):
        """The posterior predictive mean at new design rows: A_new [n_new, x_dim], offset_new [n_new] or None; samples and route as
        `pointwise` takes them.  Returns a dict of float64 arrays of length n_new: mean and sd (n - 1 in the divisor; NaN below 2
        live draws) over the live draws of mu = 1 / (1 + exp(-eta)) (logistic) or exp(eta) (poisson), eta = offset_new + A_new theta,
        and n_live (eta and mu finite).  ValueError for shapes the constructor would refuse."""
        x = self._draws(samples, 'GLMData.predict')
        route = self._route(route, 'GLMData.predict')
        A = np.array(A_new, dtype=np.float64)
        if A.ndim != 2 or A.shape[1] != self.x_dim or not 1 <= A.shape[0] <= self.MAX_ROWS:
            raise ValueError('GLMData.predict: A_new must be shaped [n_new, %d] with n_new in 1 .. %d, got %s' % (self.x_dim, self.MAX_ROWS, A.shape))
        n = A.shape[0]
        o = np.zeros(n) if offset_new is None else np.array(offset_new, dtype=np.float64)
        if o.shape != (n,):
            raise ValueError('GLMData.predict: offset_new must be shaped [%d], got %s' % (n, o.shape))
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(o))):
            raise ValueError('GLMData.predict: A_new and offset_new must be finite')
        stats = _lib.empty_glm_pointwise(n, 3)
        if route == 'fused':
            import torch
            from . import flow
            dev = torch.device('cuda', torch.cuda.current_device())
            at, yy, oo = self.layout(A, np.zeros(n), o)
            spec = dict(at=torch.as_tensor(at).to(dev), y=torch.as_tensor(yy).to(dev), o=torch.as_tensor(oo).to(dev), logl0=0.0, n=n,
                        family=self.family)
            for first in range(0, x.shape[0], self.POINTWISE_CHUNK):
                part = flow.glm_predict(spec, np.ascontiguousarray(x[first:first + self.POINTWISE_CHUNK], dtype=np.float32), device=dev)
                stats = _lib.merge_glm_pointwise(stats, part.cpu().numpy())
        else:
            chunk = max(1, self.POINTWISE_HOST_BYTES // (8 * n))
            for first in range(0, x.shape[0], chunk):
                with np.errstate(over='ignore', invalid='ignore'):
                    eta = o + np.asarray(x[first:first + chunk], dtype=np.float64) @ A.T
                    mu = 1.0 / (1.0 + np.exp(-eta)) if self.family == 'logistic' else np.exp(eta)
                block = np.stack(self._moments(mu, np.isfinite(eta) & np.isfinite(mu)), axis=1)
                stats = _lib.merge_glm_pointwise(stats, block)
        cnt, mean, M2 = stats.T
        with np.errstate(invalid='ignore'):
            sd = np.where(cnt >= 2, np.sqrt(M2 / np.where(cnt >= 2, cnt - 1.0, 1.0)), np.nan)
        self.predict_route = route
        return dict(mean=np.where(cnt > 0, mean, np.nan), sd=sd, n_live=cnt)

    # ---- the posterior mode and the Laplace approximation (build-defined: the reference has none; include/nnest_hip.h nnest_glm_curv) ----
    def laplace(self, prior=None, theta0=None, tol=1e-12, max_iter=100, route=None):
        """The posterior mode, the curvature there and the Laplace approximation built on them, by damped Newton (build-defined:
        the reference has none).  prior: None or a priors.GaussianPrior (ValueError for anything else: a box has no curvature, and
        truncation is not modelled).  Returns a laplace.LaplaceFit: mode, precision (the negative Hessian H of the log posterior at
        the mode), cov, chol, logl, logprior, logdet, logz (the Laplace evidence logl + logprior + (D / 2) log 2 pi - logdet / 2;
        None without a prior), decrement, iterations, halvings, converged, route, and `sample` / `as_gaussian` -- what
        MCMCSampler.run takes as training_samples= and init_samples=, and the approximation as a GaussianData.
        The iteration: start at theta0, else at the prior's mean, else at 0; evaluate log L, its gradient g and H at theta (with
        the prior's terms) and the Newton step delta = H^-1 g; stop with converged=True when the Newton decrement lambda^2 = g^T
        delta AT THE CURRENT theta is <= tol, returning that theta; otherwise try alpha = 1, 1/2, 1/4, ... (at most 40 halvings) and
        accept the first alpha whose log posterior is finite and >= log post(theta) + 1e-4 alpha lambda^2.  After max_iter
        iterations, or a failed line search, the result has converged=False and a warning is issued.
        ValueError where H is not positive definite at an evaluated point: the data do not determine theta (n < x_dim, collinear
        columns), and a GaussianPrior is the remedy.
        FOR SEPARABLE CLASSES WITHOUT A PRIOR NO MODE EXISTS (logistic family: some direction splits the y = 1 rows from the y = 0
        rows): the likelihood keeps rising along that direction, the iterates walk off to infinity, and the decrement falls slowly
        below any tol on the way -- this cannot be told from convergence, so the result then says converged=True at a theta that
        means nothing.  A proper prior is the cure.
        route: 'fused' -- every evaluation is one nnest_glm_curv (the reduction over the data rows on the float64 matrix cores)
        and one nnest_glm_newton_solve on the device, float64 from the float32 data, the host reading four doubles per trial;
        'host' -- the same definition in float64 numpy from the same float32 data, no GPU needed; None -- 'fused' where a device is
        available.  The two routes differ by rounding only."""
        from . import laplace as _laplace
        return _laplace.fit(self, prior=prior, theta0=theta0, tol=tol, max_iter=max_iter, route=route)
