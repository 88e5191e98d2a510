"""The posterior mode of a regression likelihood of user data, the curvature there and the Laplace approximation built on them
(build-defined: the reference has none; include/nnest_hip.h nnest_glm_curv, nnest_glm_newton_solve).

`fit` is the damped Newton iteration behind likelihoods.GLMData.laplace; `host_curvature` and `host_solve` restate the two kernels in
float64 numpy from the same float32 descriptors (route 'host': no GPU needed), in the order of their definition, so that the two
routes differ by rounding only.  `LaplaceFit` is what comes back."""
import math
import warnings

import numpy as np
import scipy.linalg

SAFE = -1e100
ARMIJO = 1e-4        # the sufficient-increase constant of the line search
MAX_HALVINGS = 40    # alpha = 1, 1/2, ..., 2^-40
NOT_POSITIVE_DEFINITE = ('GLMData.laplace: the curvature of the log posterior is not positive definite at an evaluated point: the '
                         'data do not determine theta.  A proper prior is the remedy: pass prior=priors.GaussianPrior(...)')


class LaplaceFit(object):
    """The Laplace approximation of a regression posterior: mode [D]; precision [D, D] = H, the negative Hessian of the log posterior
    at the mode; chol = L with H = L L^T; cov = H^-1; logl and logprior there (logprior 0.0 without a prior); logdet = log det H;
    logz = logl + logprior + (D / 2) log 2 pi - logdet / 2, the Laplace evidence -- None without a prior, where no evidence is
    defined; decrement, the Newton decrement g^T H^-1 g at the mode; iterations and halvings of the run; converged; route."""

    def __init__(self, mode, precision, chol, logl, logprior, logdet, decrement, iterations, halvings, converged, route, has_prior):
        self.mode = np.array(mode, dtype=np.float64)
        self.precision = np.array(precision, dtype=np.float64)
        self.chol = np.array(chol, dtype=np.float64)
        D = self.mode.shape[0]
        linv = scipy.linalg.solve_triangular(self.chol, np.eye(D), lower=True)
        self.cov = linv.T @ linv
        self.logl, self.logprior, self.logdet = float(logl), float(logprior), float(logdet)
        self.logz = self.logl + self.logprior + 0.5 * D * math.log(2.0 * math.pi) - 0.5 * self.logdet if has_prior else None
        self.decrement, self.iterations, self.halvings = float(decrement), int(iterations), int(halvings)
        self.converged, self.route = bool(converged), route

    def sample(self, num_samples, seed=None):
        """num_samples draws [num_samples, D] of the approximation, mode + L^-T z with z ~ N(0, I) from a numpy.random.RandomState(seed),
        float64 on the host: what a sampler's training_samples= and init_samples= take"""
        z = np.random.RandomState(seed).standard_normal(size=(int(num_samples), self.mode.shape[0]))
        return self.mode + scipy.linalg.solve_triangular(self.chol.T, z.T, lower=False).T

    def as_gaussian(self):
        """the approximation as a likelihood the fused Gaussian-data kernels run: GaussianData(mode, precision=precision, logl_max=logl)"""
        from .likelihoods import GaussianData
        return GaussianData(self.mode, precision=self.precision, logl_max=self.logl)


def _prior_parts(prior_data):
    """(m, r, logc) in float64 from the float32-rounded values of priors.GaussianPrior.hip_gauss_prior"""
    return (np.asarray(prior_data['m'], np.float32).astype(np.float64), np.asarray(prior_data['r'], np.float32).astype(np.float64),
            float(prior_data['logc']))


def log_prior(prior_data, theta):
    """log pi = logc - 1/2 sum ((theta - m) r)^2 in float64 from the float32-rounded descriptor; 0.0 without a prior"""
    if prior_data is None:
        return 0.0
    m, r, logc = _prior_parts(prior_data)
    u = (np.asarray(theta, np.float64) - m) * r
    return logc - 0.5 * float(np.sum(u * u))


def host_curvature(data, theta):
    """nnest_glm_curv in float64 numpy from the float32 descriptor `data` (likelihoods.GLMData.hip_like_glm): (logL, the gradient
    [D], the negative Hessian [D, D]) at theta [D]; logL = -1e100 where it is not finite"""
    n = int(data['n'])
    A = np.asarray(data['at'], np.float32)[:, :n].astype(np.float64).T
    y = np.asarray(data['y'], np.float32)[:n].astype(np.float64)
    o = np.asarray(data['o'], np.float32)[:n].astype(np.float64)
    theta = np.asarray(theta, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        eta = o + A @ theta
        if data['family'] in ('logistic', 0):
            s = (1.0 - 2.0 * y) * eta
            l = -(np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))))
            t = np.exp(-np.abs(eta))
            big, small = 1.0 / (1.0 + t), t / (1.0 + t)
            mu, w = np.where(eta >= 0.0, big, small), big * small
        else:
            mu = np.exp(eta)
            l, w = y * eta - mu, mu
        l = np.where(np.isfinite(eta), l, np.nan)
        logl = float(data['logl0']) + float(np.sum(l))
        g = A.T @ (y - mu)
        H = (A * w[:, None]).T @ A
    H = np.triu(H) + np.triu(H, 1).T   # (bit-symmetric, as the kernel writes it)
    return (logl if abs(logl) <= np.finfo(np.float64).max else SAFE), g, H


def host_solve(logl, g, H, theta, prior_data):
    """nnest_glm_newton_solve in float64 numpy: (info [4] = {log L + log pi, decrement, log det, status}, step [D], chol [D, D], H
    with the prior's diagonal)"""
    D = len(g)
    logpi = 0.0
    if prior_data is not None:
        m, r, logc = _prior_parts(prior_data)
        d = np.asarray(theta, np.float64) - m
        u = d * r
        g = g - d * (r * r)
        H = H + np.diag(r * r)
        with np.errstate(over='ignore', invalid='ignore'):
            ss = float(np.sum(u * u))
        logpi = logc - 0.5 * ss if abs(ss) <= np.finfo(np.float64).max else -np.inf
    lp = logl + logpi
    zeros = (np.zeros(D), np.zeros((D, D)), H)
    if logl == SAFE or not np.isfinite(logpi):
        return (np.array([lp if np.isfinite(lp) else SAFE, 0.0, 0.0, 2.0]),) + zeros
    try:
        if not np.all(np.isfinite(H)):
            raise np.linalg.LinAlgError('not finite')
        L = np.linalg.cholesky(H)
        # (a pivot that is not above (j + 2) 2^-52 H_jj, the bound on its own rounding error, counts as <= 0: the kernel's rule)
        if not np.all(np.diag(L) ** 2 > (np.arange(D) + 2.0) * 2.0 ** -52 * np.diag(H)):
            raise np.linalg.LinAlgError('singular to rounding')
    except np.linalg.LinAlgError:
        return (np.array([lp, 0.0, 0.0, 1.0]),) + zeros
    step = scipy.linalg.solve_triangular(L.T, scipy.linalg.solve_triangular(L, g, lower=True), lower=False)
    return np.array([lp, float(g @ step), 2.0 * float(np.sum(np.log(np.diag(L)))), 0.0]), step, L, H


def _newton(evaluate, advance, theta, tol, max_iter):
    """the damped Newton iteration on `evaluate(theta) -> (info [4], state)` and `advance(theta, alpha, state) -> theta + alpha step`.
    Returns (theta, info, state, iterations, halvings, converged)"""
    def checked(th):
        info, state = evaluate(th)
        if int(info[3]) == 1:
            raise ValueError(NOT_POSITIVE_DEFINITE)
        return info, state

    info, state = checked(theta)
    if int(info[3]) != 0:
        raise ValueError('GLMData.laplace: the log posterior is not finite at the starting point: pass a theta0 nearer the mode')
    iterations = halvings = 0
    converged = False
    while True:
        lp, dec = float(info[0]), float(info[1])
        if dec <= tol:   # (the decrement AT the current theta: no further step is taken)
            converged = True
            break
        if iterations >= max_iter:
            break
        alpha, accepted = 1.0, None
        for h in range(MAX_HALVINGS + 1):
            trial = advance(theta, alpha, state)
            tinfo, tstate = checked(trial)
            if int(tinfo[3]) == 0 and np.isfinite(tinfo[0]) and float(tinfo[0]) >= lp + ARMIJO * alpha * dec:
                accepted = (trial, tinfo, tstate)
                break
            if h < MAX_HALVINGS:
                alpha *= 0.5
                halvings += 1
        if accepted is None:
            break
        theta, info, state = accepted   # (the accepted trial's results are the next iteration's)
        iterations += 1
    return theta, info, state, iterations, halvings, converged


def fit(like, prior=None, theta0=None, tol=1e-12, max_iter=100, route=None):
    """likelihoods.GLMData.laplace (its docstring has the definition)"""
    from .priors import GaussianPrior
    if prior is not None and not isinstance(prior, GaussianPrior):
        raise ValueError('GLMData.laplace: prior must be None or a priors.GaussianPrior (a box has no curvature, and truncation is not '
                         'modelled), got %s' % type(prior).__name__)
    D = like.x_dim
    if prior is not None and prior.x_dim != D:
        raise ValueError('GLMData.laplace: the prior has x_dim=%d, the likelihood %d' % (prior.x_dim, D))
    route = like._route(route, 'GLMData.laplace')
    pdata = prior.hip_gauss_prior if prior is not None else None
    if theta0 is None:
        theta0 = np.asarray(pdata['m'], np.float32).astype(np.float64) if pdata is not None else np.zeros(D)
    theta0 = np.array(theta0, dtype=np.float64)
    if theta0.shape != (D,):
        raise ValueError('GLMData.laplace: theta0 must be shaped [%d], got %s' % (D, theta0.shape))
    if not np.all(np.isfinite(theta0)):
        raise ValueError('GLMData.laplace: theta0 must be finite')
    tol, max_iter = float(tol), int(max_iter)
    data = like.hip_like_glm
    if route == 'fused':
        import torch
        from . import flow
        dev = torch.device('cuda', torch.cuda.current_device())
        spec = {k: (torch.as_tensor(v).to(dev) if k in ('at', 'y', 'o') else v) for k, v in data.items()}
        pspec = None if pdata is None else {k: (torch.as_tensor(v).to(dev) if k in ('m', 'r') else v) for k, v in pdata.items()}

        def evaluate(th):
            curv = flow.glm_curvature(spec, th, device=dev)
            step, chol, info = flow.glm_newton_solve(curv, th, prior=pspec, device=dev)
            return info.cpu().numpy(), (curv, step, chol)   # (the one synchronisation of a trial)

        theta, info, (curv, step, chol), iterations, halvings, converged = _newton(
            evaluate, lambda th, alpha, st: th + alpha * st[1], torch.from_numpy(theta0).to(dev), tol, max_iter)
        curv, theta, chol = curv.cpu().numpy(), theta.cpu().numpy(), chol.cpu().numpy()
        logl, H = float(curv[0]), curv[1 + D:].reshape(D, D).copy()
        if pdata is not None:
            r = _prior_parts(pdata)[1]
            H[np.diag_indices(D)] = np.diag(H) + r * r
    else:
        def evaluate(th):
            logl, g, H = host_curvature(data, th)
            info, step, chol, Hp = host_solve(logl, g, H, th, pdata)
            return info, (logl, step, chol, Hp)

        theta, info, (logl, step, chol, H), iterations, halvings, converged = _newton(
            evaluate, lambda th, alpha, st: th + alpha * st[1], theta0, tol, max_iter)
    if not converged:
        warnings.warn('GLMData.laplace: not converged after %d Newton iterations (%d halvings): Newton decrement %.3g above tol %.3g'
                      % (iterations, halvings, float(info[1]), tol))
    return LaplaceFit(theta, H, chol, logl, log_prior(pdata, theta), float(info[2]), float(info[1]), iterations, halvings, converged, route,
                      prior is not None)
