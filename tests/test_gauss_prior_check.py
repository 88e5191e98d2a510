"""CPU checks of priors.GaussianPrior, of its restatement and bound (tests/gauss_prior_check.py), of DeviceTarget's `prior_gauss`, of
Sampler._device_target's routing on a stub flow, and of the restated walk on the target with the prior against a brute-force float64
Metropolis step in one dimension."""
import logging

import numpy as np
import pytest

from nnest_amd.priors import GaussianPrior, Prior
from tests import gauss_prior_check as pk
from tests import glm_check as gk
from tests import mcmc_adapt_check as ac


# ---- the class ----------------------------------------------------------------------------------------------------------------------
def test_log_density_is_the_closed_form_and_normalised():
    p = GaussianPrior(3, [0.5, -1.0, 2.0], [0.5, 2.0, 1.5])
    assert isinstance(p, Prior) and p.x_dim == 3
    x = np.array([0.1, 0.2, 0.3])
    want = sum(-0.5 * ((x[c] - p.mean[c]) / p.sigma[c]) ** 2 - np.log(p.sigma[c]) - 0.5 * np.log(2 * np.pi) for c in range(3))
    assert abs(p(x) - want) < 1e-13 and isinstance(p(x), float)
    assert abs(p.logc - (-np.sum(np.log([0.5, 2.0, 1.5])) - 1.5 * np.log(2 * np.pi))) < 1e-14
    # the density integrates to 1: trapezoid over +-12 sigma, one dimension (a product of such)
    q = GaussianPrior(1, 0.7, 0.3)
    g = np.linspace(0.7 - 3.6, 0.7 + 3.6, 20001)
    assert abs(np.trapezoid(np.exp(q.log_prob_rows(g[:, None])), g) - 1.0) < 1e-9
    # scalars broadcast
    b = GaussianPrior(4, 0.0, 2.0)
    assert np.array_equal(b.mean, np.zeros(4)) and np.array_equal(b.sigma, np.full(4, 2.0))


def test_rows_equal_the_callable_row_by_row():
    p = GaussianPrior(5, np.linspace(-1, 1, 5), np.linspace(0.5, 2.5, 5))
    x = np.random.RandomState(0).normal(size=(40, 5)) * 3
    rows = p.log_prob_rows(x)
    assert rows.dtype == np.float64 and rows.shape == (40,)
    np.testing.assert_allclose(rows, [p(r) for r in x], rtol=0, atol=1e-13)


def test_sample_moments_and_rng_consumption():
    p = GaussianPrior(2, [1.0, -2.0], [0.5, 3.0])
    np.random.seed(7)
    s = p.sample(200000)
    after = np.random.uniform()
    assert s.shape == (200000, 2)
    # five standard errors of the mean and of the standard deviation
    assert np.all(np.abs(s.mean(0) - p.mean) <= 5 * p.sigma / np.sqrt(len(s)))
    assert np.all(np.abs(s.std(0) - p.sigma) <= 5 * p.sigma / np.sqrt(2 * len(s)))
    # one normal block of (n, D) from numpy's global generator, nothing else
    np.random.seed(7)
    block = np.random.standard_normal(size=(200000, 2))
    assert np.array_equal(s, p.mean + p.sigma * block) and np.random.uniform() == after


@pytest.mark.parametrize('sigma', [0.0, -1.0, np.inf, np.nan, [1.0, 0.0], [1.0, np.nan]])
def test_bad_sigma(sigma):
    with pytest.raises(ValueError, match='sigma'):
        GaussianPrior(2, 0.0, sigma)


def test_bad_shapes_and_means():
    with pytest.raises(ValueError, match='length x_dim=3'):
        GaussianPrior(3, [0.0, 1.0], 1.0)
    with pytest.raises(ValueError, match='length x_dim=3'):
        GaussianPrior(3, 0.0, [1.0, 1.0])
    with pytest.raises(ValueError, match='mean'):
        GaussianPrior(2, [0.0, np.inf], 1.0)


def test_descriptor():
    p = GaussianPrior(3, [0.5, -1.0, 2.0], [0.3, 2.0, 1.5])
    d = p.hip_gauss_prior
    assert d['m'].dtype == np.float32 and d['r'].dtype == np.float32 and isinstance(d['logc'], float)
    assert np.array_equal(d['m'], np.float32([0.5, -1.0, 2.0])) and np.array_equal(d['r'], (1.0 / np.array([0.3, 2.0, 1.5])).astype(np.float32))
    assert d['logc'] == p.logc


# ---- the restatement and the bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 2, 33, 128])
def test_float32_evaluations_stay_inside_the_bound(D):
    r = np.random.RandomState(D)
    p = GaussianPrior(D, r.uniform(-2, 2, D), r.uniform(0.05, 5.0, D))
    t = (r.normal(size=(400, D)) * r.uniform(0.01, 30.0, size=(400, 1))).astype(np.float32)
    t[0] = p.hip_gauss_prior['m']
    want, B = pk.exact(p, t), pk.bound(p, t)
    assert want[0] == p.logc
    # the restatement is the callable's value on the float32 descriptor: r = float32(1 / sigma) is within 2^-24 of 1 / sigma
    np.testing.assert_allclose(want, p.log_prob_rows(t.astype(np.float64)), rtol=2e-7, atol=1e-6)
    worst = 0.0
    for order in ('forward', 'reversed'):
        got = pk.float32_eval(p, t, order)
        assert np.all(np.abs(got - want) <= B)
        worst = max(worst, float(np.max(np.abs(got - want) / B)))
    assert 0.0 < worst <= 1.0
    # the bound is not idle: most of it is the float32 part, which a float32 evaluation uses a fair share of
    assert D > 2 or worst > 0.01


def test_non_finite_rows_are_refused_never_nan():
    p = GaussianPrior(3, 0.0, 1.0)
    t = np.zeros((5, 3), np.float32)
    t[1, 0], t[2, 2], t[3, 1], t[4] = np.nan, np.inf, -np.inf, 3.0e38
    wide = dict(m=np.zeros(3, np.float32), r=np.zeros(3, np.float32), logc=0.0)   # r = 0: inf * 0 is NaN -- refused too
    for data in (p, wide):
        for got in (pk.exact(data, t), pk.float32_eval(data, t)):
            assert np.isfinite(got[0]) and np.all(got[1:4] == -np.inf) and not np.any(np.isnan(got))
    # (a large finite coordinate is no such row: u = 3e38 is a float32 and u^2 = 9e76 a float64)
    assert np.isfinite(pk.float32_eval(p, t)[4]) and np.isfinite(pk.exact(p, t)[4])
    assert pk.exact(wide, t)[0] == 0.0 and pk.exact(wide, t)[4] == 0.0


def test_sensitivity_bounds_the_change():
    r = np.random.RandomState(3)
    D = 6
    p = GaussianPrior(D, r.uniform(-1, 1, D), r.uniform(0.2, 2.0, D))
    sd = r.uniform(0.5, 1.5, D)
    x = r.normal(size=(50, D))
    tol = 1e-3
    dx = r.uniform(-tol, tol, size=x.shape)
    a, b = p.log_prob_rows(x * sd), p.log_prob_rows((x + dx) * sd)
    s = pk.sensitivity(p, (x * sd).astype(np.float32), sd, np.full(50, tol))
    assert np.all(np.abs(a - b) <= s * (1 + 1e-4) + 1e-9) and np.all(s < 1.0)


# ---- DeviceTarget -----------------------------------------------------------------------------------------------------------------
def test_device_target_carries_the_prior():
    from nnest_amd.device_target import DeviceTarget
    like = gk.make_like(3, 40, 'poisson', 1)
    p = GaussianPrior(3, [0.1, 0.2, 0.3], 2.0)
    t = DeviceTarget(None, (), np.ones(3), np.zeros(3), like_glm=like.hip_like_glm, prior_gauss=p.hip_gauss_prior)
    assert t.prior_gauss['logc'] == p.logc and t.prior_gauss['m'].dtype == np.float32 and t.lo is None
    assert np.array_equal(t.prior_gauss['r'], p.hip_gauss_prior['r']) and t.prior_gauss['m'] is not p.hip_gauss_prior['m']
    with pytest.raises(AttributeError):
        t.prior_gauss = None
    with pytest.raises(ValueError):
        t.prior_gauss['m'][0] = 1.0
    u = t.with_transform(2 * np.ones(3), np.ones(3))
    assert np.array_equal(u.prior_gauss['m'], t.prior_gauss['m']) and u.prior_gauss['logc'] == p.logc and u.t_std[0] == 2.0
    assert u.like_glm['n'] == 40
    # only beside a like_glm, and without a box
    with pytest.raises(ValueError, match='prior_gauss needs a like_glm'):
        DeviceTarget(3, (0.5,), prior_gauss=p.hip_gauss_prior)
    with pytest.raises(ValueError, match='prior_gauss needs a like_glm'):
        DeviceTarget(None, (), like_data=dict(mu=[0.0], R=[[1.0]], logl0=0.0), prior_gauss=p.hip_gauss_prior)
    with pytest.raises(ValueError, match='no box'):
        DeviceTarget(None, (), None, None, -np.ones(3), np.ones(3), like_glm=like.hip_like_glm, prior_gauss=p.hip_gauss_prior)
    # the call forms there were
    assert DeviceTarget(None, (), like_glm=like.hip_like_glm).prior_gauss is None
    assert DeviceTarget(3, (0.5,)).with_transform(np.ones(2), np.zeros(2)).prior_gauss is None


# ---- the routing, on a flow without a device ---------------------------------------------------------------------------------------
class _Flow(object):
    device = 'cpu'
    refusal = None

    def __init__(self, D, syms):
        self.D, self._sym = D, dict((s, None) for s in syms)
        self.asked = []

    def mcmc_glm_refusal(self, D=None):
        self.asked.append(('glm', D))
        return None

    def mcmc_glm_prior_refusal(self, D=None):
        self.asked.append(('glm_prior', D))
        return self.refusal

    def mcmc_gdata_refusal(self, D=None):
        return None


class _Trainer(object):
    def __init__(self, net):
        self.netG = net


def _bare_sampler(like, net, prior):
    from nnest_amd.mcmc import MCMCSampler
    s = MCMCSampler.__new__(MCMCSampler)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = like.x_dim, 0, 0, _Trainer(net)
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = like, prior, None, True, 1.0
    s.logger = logging.getLogger('test_gauss_prior_check')
    s._probe_agrees_glm = lambda data, affine, warn='': True
    s._probe_agrees_gdata = lambda data, affine, warn='': True
    s._probe_agrees = lambda *a, **k: True
    return s


OLD = ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt', 'importance', 'ensemble', 'mcmc_gdata', 'mcmc_gdata_check', 'mcmc_glm',
       'mcmc_glm_check')
NEW = OLD + ('mcmc_glm_prior', 'mcmc_glm_prior_check')
REFUSED = ('this transform, likelihood or prior (an affine transform, a likelihood that agrees with the kernel\'s, and no prior or a '
           'UniformPrior on T(x), or a GaussianPrior with a GLMData)')


def test_device_target_takes_a_gaussian_prior_beside_a_glm():
    like = gk.make_like(3, 40, 'logistic', 2)
    p = GaussianPrior(3, 0.0, 2.0)
    net = _Flow(3, NEW)
    s = _bare_sampler(like, net, p)
    probes = []
    s._probe_agrees_gauss_prior = lambda data, affine, warn='': probes.append(data) or True
    for entry in ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt'):
        target, why = s._device_target(entry=entry)
        assert why is None and target.like_glm['n'] == 40 and target.lo is None and target.hi is None
        assert np.array_equal(target.prior_gauss['r'], np.full(3, 0.5, np.float32)) and target.prior_gauss['logc'] == p.logc
    assert net.asked == [('glm_prior', 3)] * 4 and len(probes) == 4
    # the library's refusal of the flow, in its words
    net.refusal = 'mcmc glm: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only'
    assert s._device_target(entry='mcmc') == (None, 'the flow _Flow: ' + net.refusal)
    net.refusal = None
    # a descriptor that disagrees with the callable
    s._probe_agrees_gauss_prior = lambda data, affine, warn='': False
    assert s._device_target(entry='mcmc') == (None, REFUSED)
    s._probe_agrees_gauss_prior = lambda data, affine, warn='': True
    # not on T(x); a subclass with a rule of its own; a flow that does not bind the entry: a Python prior, as before
    s._transform_prior = False
    assert s._device_target(entry='mcmc') == (None, REFUSED)
    s._transform_prior = True

    class Mine(GaussianPrior):
        def __call__(self, x):
            return 0.0

    s._user_prior = Mine(3, 0.0, 2.0)
    assert s._device_target(entry='mcmc') == (None, REFUSED)
    s._user_prior = p
    s.trainer.netG = _Flow(3, OLD)
    assert s._device_target(entry='mcmc') == (None, REFUSED)
    assert s.trainer.netG.asked == [('glm', 3)]
    # without a prior the likelihood's own check is asked, as before
    s._user_prior = None
    s.trainer.netG = net2 = _Flow(3, NEW)
    target, why = s._device_target(entry='mcmc')
    assert why is None and target.prior_gauss is None and net2.asked == [('glm', 3)]


def test_device_target_refuses_a_gaussian_prior_with_any_other_likelihood():
    from nnest_amd.likelihoods import GaussianData
    p = GaussianPrior(3, 0.0, 2.0)
    r = np.random.RandomState(0)
    gd = GaussianData(r.normal(size=3), np.eye(3))
    s = _bare_sampler(gd, _Flow(3, NEW), p)
    s._probe_agrees_gauss_prior = lambda *a, **k: pytest.fail('no probe of the prior beside another likelihood')
    for entry in ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt'):
        assert s._device_target(entry=entry) == (None, REFUSED)

    class ById(object):
        x_dim, hip_like_id, hip_like_params = 3, 3, (0.5,)

        def __call__(self, x):
            return np.zeros(len(x))

    net = _Flow(3, NEW)
    net.mcmc_mixed_refusal = net.mcmc_adapt_refusal = lambda like_id: None
    s = _bare_sampler(ById(), net, p)
    for entry in ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt'):
        assert s._device_target(entry=entry) == (None, REFUSED)
    assert net.asked == []
    # the evidence's sentence is extended in the same way
    net.importance_refusal = lambda like_id: None
    why = s._device_target(entry='importance', unit_box_on_x=True)[1]
    assert why.endswith('a UniformPrior on T(x) or the unit box on x, or a GaussianPrior with a GLMData)')


def test_mcmc_steps_takes_prior_gauss_only_with_like_glm():
    from nnest_amd.flow import _HipFlow
    p = GaussianPrior(3, 0.0, 2.0)
    net = _HipFlow.__new__(_HipFlow)
    net._sym = {}
    with pytest.raises(ValueError, match='prior_gauss goes only with a like_glm'):
        net.mcmc_steps(3, None, 2, 0.1, prior_gauss=p.hip_gauss_prior)
    with pytest.raises(ValueError, match='prior_gauss goes only with a like_glm'):
        net.mcmc_steps(None, None, 2, 0.1, like_data=dict(mu=[0.0], R=[[1.0]], logl0=0.0), prior_gauss=p.hip_gauss_prior)
    with pytest.raises(NotImplementedError, match='under a normal prior'):
        net.mcmc_steps(None, None, 2, 0.1, like_glm=gk.make_like(3, 40, 'logistic', 2).hip_like_glm, prior_gauss=p.hip_gauss_prior)


def test_host_route_takes_the_prior_through_the_protocol():
    """a GaussianPrior is a prior with `sample` and `log_prob_rows`: Sampler's host side calls it as it calls every prior"""
    from nnest_amd.sampler import Sampler
    p = GaussianPrior(2, [0.5, -0.5], [1.0, 2.0])
    s = Sampler.__new__(Sampler)
    s._user_prior, s._transform_prior, s.transform = p, True, (lambda x: 2.0 * x)
    x = np.random.RandomState(1).normal(size=(7, 2))
    np.testing.assert_allclose(s._checked_prior(x), [p(2.0 * r) for r in x], rtol=0, atol=1e-13)
    assert callable(getattr(p, 'sample')) and p.sample(3).shape == (3, 2)


# ---- the restated walk against a brute-force Metropolis step, one dimension ---------------------------------------------------------
class _Identity(object):
    """the identity flow: x = z, log|det| = 0"""

    def inverse(self, q):
        q = np.asarray(q, np.float32)
        return q, np.zeros(len(q))


@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('beta', [1.0, 0.5])
def test_restated_walk_is_a_metropolis_step_on_the_posterior(family, beta):
    like = gk.make_like(1, 40, family, 9)
    p = GaussianPrior(1, 0.3, 0.8)
    rs = pk.RestatedPrior(_Identity(), like.hip_like_glm, p, np.ones(1), np.zeros(1), beta=beta)
    r = np.random.RandomState(2)
    N, k = 500, 3
    z = r.normal(size=(N, 1)).astype(np.float32)

    def logpost(th):   # float64 from the definitions, nothing shared with the restatement
        th = np.asarray(th, np.float64)
        return beta * like.loglike_rows(th) + np.array([p(row) for row in th])

    lp = rs.lp(z)
    np.testing.assert_allclose(lp, logpost(z), rtol=1e-6, atol=1e-5)
    moved_l = moved_g = 0
    for t in range(6):
        eps, u = r.normal(size=(N, 1)).astype(np.float32), r.uniform(size=N).astype(np.float32)
        step = np.full((N, 1), 0.7, np.float32)
        rec = {}
        z_new, lp_new = pk.mixed_step(t, k, z, lp, eps, u, step, rs, record=rec)
        glob = ac.kind(t, k)
        q = eps.astype(np.float64) if glob else z.astype(np.float64) + 0.7 * eps.astype(np.float64)
        ratio = logpost(q) - logpost(z)
        if glob:   # the independence step from N(0, 1): the ratio of importance weights
            ratio = ratio + 0.5 * q[:, 0] ** 2 - 0.5 * z[:, 0].astype(np.float64) ** 2
        margin = ratio - np.log(u.astype(np.float64))
        clear = np.abs(margin) > 1e-4   # (float32 proposals and float32 eta against float64: decisions away from the threshold)
        assert clear.mean() > 0.99
        assert np.array_equal(rec['accept'][clear], (margin > 0)[clear])
        np.testing.assert_allclose(rec['margin'][clear], margin[clear], rtol=0, atol=1e-4)
        assert np.array_equal(z_new[rec['accept']], rec['q'][rec['accept']]) and np.array_equal(z_new[~rec['accept']], z[~rec['accept']])
        moved_g += int(rec['accept'].sum()) if glob else 0
        moved_l += 0 if glob else int(rec['accept'].sum())
        z, lp = z_new, lp_new
    assert 0 < moved_g < 2 * N and 0 < moved_l < 4 * N
