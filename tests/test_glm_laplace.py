"""GLMData.laplace on the host route (nnest_amd/laplace.py): the posterior mode, the curvature there and the Laplace
approximation, against closed forms, a grid quadrature and the longdouble restatement of tests/glm_newton_check.py.  No GPU.

Measured on the host route (float64 numpy): at most 6 Newton iterations and no halving on the 144 cases under the prior, at most 5
without one; the restated decrement at the returned mode at most 9.0e-13 (against 2 tol = 2e-12); Laplace log Z -32.8306 (logistic)
and -77.3678 (poisson) against the quadrature's -32.8064 and -77.3745."""
import warnings

import numpy as np
import pytest

from tests import glm_check as gk
from tests import glm_newton_check as nk

DIMS = [1, 5, 32, 33, 64, 65, 100, 128]
ROWS = [1, 15, 16, 17, 63, 64, 65, 70, 200]
TOL = 1e-12


def the_prior(D):
    from nnest_amd.priors import GaussianPrior
    return GaussianPrior(D, np.linspace(-0.2, 0.3, D), np.linspace(1.0, 1.5, D))


def fit_host(like, prior, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('error')   # (a run that does not converge fails here)
        return like.laplace(prior=prior, route='host', **kw)


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_intercept_only_closed_forms(family):
    from nnest_amd.likelihoods import GLMData
    r = np.random.RandomState(11)
    n = 70
    y = r.poisson(3.0, n).astype(np.float64) if family == 'poisson' else (r.uniform(size=n) < 0.3).astype(np.float64)
    like = GLMData(np.ones((n, 1)), y, family=family)
    ybar = y.mean()
    mode, H = (np.log(ybar), y.sum()) if family == 'poisson' else (np.log(ybar / (1.0 - ybar)), n * ybar * (1.0 - ybar))
    # The iteration returns the first theta whose decrement lambda^2 = g^2 / H is <= tol, and |theta - mode| = sqrt(lambda^2 / H) to
    # first order there: from the default start at the default tol that is all the stopping rule promises (a factor 2 to spare)
    fit = fit_host(like, None)
    assert fit.converged and fit.route == 'host' and fit.logz is None and fit.logprior == 0.0
    assert abs(fit.mode[0] - mode) <= 2 * np.sqrt(TOL / H)
    # A mode to 1e-10 relative needs lambda^2 <= (1e-10 |mode|)^2 H -- 1.2e-19 (logistic, H = 15) and 2.5e-18 (poisson, H = 210)
    # here: tol = 1e-20.  A log posterior of size 100 resolves increases of 1e-14 at best, so the line search cannot be relied on
    # to cross the decrements between 1e-14 and 1e-20 in small steps.  The run starts 1e-6 off the closed form, where lambda^2 =
    # 1e-12 H is far above that noise, and ONE full Newton step squares the error: the third derivative of either family's log
    # likelihood is at most the second in size, so the step lands within 5e-13 of the mode, lambda^2 <= 5e-23 there, 200 times
    # under tol.  What is checked is that the Newton step is right to 1e-10.
    fit = fit_host(like, None, theta0=np.array([mode + 1e-6]), tol=1e-20)
    assert fit.converged and 1 <= fit.iterations <= 2
    np.testing.assert_allclose(fit.mode, [mode], rtol=1e-10)
    np.testing.assert_allclose(fit.precision, [[H]], rtol=1e-10)
    np.testing.assert_allclose(fit.cov, [[1.0 / H]], rtol=1e-10)
    np.testing.assert_allclose(fit.logdet, np.log(H), rtol=1e-10)


# ---- 2. the evidence against quadrature ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_evidence_against_quadrature(family):
    from nnest_amd.priors import GaussianPrior
    from tests.test_gpu_mcmc_glm_prior import quadrature
    like = gk.make_like(2, 40, family, 5)
    prior = GaussianPrior(2, 0.0, 2.0)
    fit = fit_host(like, prior)
    ref = quadrature(like, prior, -20.0, 20.0)[0]
    print('%s: Laplace log Z %.4f, quadrature %.4f' % (family, fit.logz, ref))
    assert fit.converged and abs(fit.logz - ref) <= 0.05
    np.testing.assert_allclose(fit.logz, fit.logl + fit.logprior + np.log(2.0 * np.pi) - 0.5 * fit.logdet, rtol=0, atol=1e-12)
    np.testing.assert_allclose(fit.logprior, prior(fit.mode), rtol=0, atol=1e-6)   # (the descriptor's 1 / sigma is float32)


# ---- 3. convergence under a prior ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', DIMS)
def test_converges_under_a_prior(D, family):
    prior = the_prior(D)
    worst_it = worst_dec = 0
    for n in ROWS:
        like = gk.make_like(D, n, family, D + n)
        fit = fit_host(like, prior)
        dec = nk.decrement(like.hip_like_glm, prior.hip_gauss_prior, fit.mode)
        worst_it, worst_dec = max(worst_it, fit.iterations), max(worst_dec, dec)
        assert fit.converged and fit.iterations <= 10, (n, fit.iterations)
        assert dec <= 2 * TOL, (n, dec)
        assert fit.decrement <= TOL and fit.mode.shape == (D,) and fit.precision.shape == (D, D) and fit.chol.shape == (D, D)
        np.testing.assert_allclose(fit.chol @ fit.chol.T, fit.precision, rtol=1e-12, atol=1e-12 * np.abs(fit.precision).max())
    print('D=%d %s: at most %d iterations, restated decrement at most %.3g' % (D, family, worst_it, worst_dec))


# ---- 4. convergence without a prior ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D,n', [(1, 70), (5, 200), (33, 200), (64, 1000), (128, 1000)])
def test_converges_without_a_prior(D, n, family):
    like = gk.make_like(D, n, family, D + n)
    fit = fit_host(like, None)
    assert fit.converged and fit.iterations <= 5 and fit.logz is None
    assert np.linalg.cond(fit.precision) < 10.0
    assert nk.decrement(like.hip_like_glm, None, fit.mode) <= 2 * TOL


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from nnest_amd.priors import UniformPrior
    like = gk.make_like(5, 3, 'logistic', 8)
    with pytest.raises(ValueError, match='GaussianPrior'):
        like.laplace(route='host')   # (n < D: the curvature is singular)
    assert like.laplace(prior=the_prior(5), route='host').converged   # (the remedy)
    like = gk.make_like(5, 40, 'poisson', 9)
    with pytest.raises(ValueError, match='GaussianPrior'):
        like.laplace(prior=UniformPrior(5, -1, 1), route='host')
    with pytest.raises(ValueError, match='theta0'):
        like.laplace(theta0=np.zeros(4), route='host')
    with pytest.raises(ValueError, match='theta0'):
        like.laplace(theta0=np.zeros((1, 5)), route='host')
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='finite'):
            like.laplace(theta0=np.array([0.0, bad, 0.0, 0.0, 0.0]), route='host')
    with pytest.raises(ValueError, match='route'):
        like.laplace(route='device')


def test_the_line_search_and_the_iteration_limit():
    """from a start six units off in every coordinate the weights of a logistic model are small and the full Newton step
    overshoots: the damped iteration halves and still reaches the mode the default start finds; one iteration is not enough from
    there, and says so"""
    like = gk.make_like(5, 200, 'logistic', 3)
    fit = fit_host(like, None, theta0=np.full(5, 6.0))
    ref = fit_host(like, None)
    assert fit.converged and fit.halvings >= 1 and ref.halvings == 0
    lam_min = np.linalg.eigvalsh(ref.precision)[0]
    assert np.linalg.norm(fit.mode - ref.mode) <= 4 * np.sqrt(2 * TOL / lam_min)   # (tests/test_gpu_glm_laplace.py has the bound)
    with pytest.warns(UserWarning, match='not converged'):
        cut = like.laplace(theta0=np.full(5, 6.0), max_iter=1, route='host')
    assert not cut.converged and cut.iterations == 1


# ---- 6. as_gaussian and sample ---------------------------------------------------------------------------------------------------------
def test_as_gaussian_and_sample():
    import nnest_amd
    like = gk.make_like(5, 70, 'logistic', 4)
    fit = fit_host(like, the_prior(5))
    assert isinstance(fit, nnest_amd.LaplaceFit)
    gd = fit.as_gaussian()
    assert gd(fit.mode) == fit.logl
    r = np.random.RandomState(2)
    d = r.normal(size=(16, 5))
    np.testing.assert_allclose(gd(fit.mode + d), fit.logl - 0.5 * np.einsum('ni,ij,nj->n', d, fit.precision, d), rtol=1e-12)
    np.testing.assert_allclose(fit.cov @ fit.precision, np.eye(5), rtol=0, atol=1e-12)
    N = 200000
    x = fit.sample(N, seed=1)
    assert x.shape == (N, 5) and x.dtype == np.float64
    assert np.array_equal(x, fit.sample(N, seed=1)) and not np.array_equal(x, fit.sample(N, seed=2))
    se_mean = np.sqrt(np.diag(fit.cov) / N)
    assert np.all(np.abs(x.mean(0) - fit.mode) <= 5 * se_mean)
    c = (x - fit.mode).T @ (x - fit.mode) / N   # (about the true mean: each entry is a mean of N products)
    se_cov = np.sqrt((np.outer(np.diag(fit.cov), np.diag(fit.cov)) + fit.cov ** 2) / N)
    assert np.all(np.abs(c - fit.cov) <= 5 * se_cov)


def test_laplace_evidence_host(caplog):
    import logging
    from nnest_amd import evaluation
    from nnest_amd.priors import GaussianPrior
    like = gk.make_like(2, 40, 'poisson', 5)
    prior = GaussianPrior(2, 0.0, 2.0)
    with caplog.at_level(logging.INFO, logger='nnest_amd.evaluation'):
        out = evaluation.laplace_evidence(like, prior, route='host')
    fit = fit_host(like, prior)
    assert {'logz', 'logl', 'logdet', 'iterations', 'converged'} <= set(out)
    assert out['logz'] == fit.logz and out['logl'] == fit.logl and out['logdet'] == fit.logdet and out['converged']
    assert any(rec.getMessage().startswith('Laplace: log Z [') and 'Newton steps' in rec.getMessage() for rec in caplog.records)
    with pytest.raises(ValueError, match='prior'):
        evaluation.laplace_evidence(like, None, route='host')
