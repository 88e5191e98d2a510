"""CPU checks of the Gaussian likelihood from user data (nnest_amd.likelihoods.GaussianData; include/nnest_hip.h nnest_gdata_t): the
host evaluation against scipy and against the residual formula of a linear model, the refusals, the descriptor the kernels take, the
a-priori bound of tests/gdata_check.py against three legal summation orders, DeviceTarget's new field, and `_device_target` on a flow
without the entry, which answers as it always did."""
import logging

import numpy as np
import pytest

from tests import gdata_check as gc


def _like(D, seed, logl_max=-3.25):
    from nnest_amd.likelihoods import GaussianData
    mu, P = gc.make_target(D, seed)
    return GaussianData(mu, precision=P, logl_max=logl_max), mu, P


@pytest.mark.parametrize('D', [1, 3, 17])
def test_against_scipy_up_to_its_constant(D):
    import scipy.stats
    from nnest_amd.likelihoods import GaussianData
    mu, P = gc.make_target(D, D)
    cov = np.linalg.inv(P)
    cov = 0.5 * (cov + cov.T)
    x = np.random.RandomState(1).normal(size=(64, D))
    want = scipy.stats.multivariate_normal.logpdf(x, mean=mu, cov=cov).reshape(-1)
    const = -0.5 * D * np.log(2 * np.pi) + 0.5 * np.linalg.slogdet(P)[1]
    for like in (GaussianData(mu, cov=cov), GaussianData(mu, precision=P)):
        np.testing.assert_allclose(like(x), want - const, rtol=1e-10, atol=1e-10)
        assert like.num_evaluations == 64 and like.max_loglike == 0.0 and like.x_dim == D
        assert like(mu) == 0.0 and like.num_evaluations == 65
    shifted = GaussianData(mu, precision=P, logl_max=-3.25)
    np.testing.assert_allclose(shifted(x), want - const - 3.25, rtol=1e-10, atol=1e-10)
    assert shifted.max_loglike == -3.25 and np.all(shifted(x) <= -3.25)


@pytest.mark.parametrize('noise', ['scalar', 'vector', 'matrix'])
def test_linear_model_is_the_residual_formula(noise):
    from nnest_amd.likelihoods import GaussianData
    r = np.random.RandomState(5)
    n, D = 40, 4
    A, y = r.normal(size=(n, D)), r.normal(size=n)
    if noise == 'scalar':
        N, Nm = 0.7, 0.7 * np.eye(n)
    elif noise == 'vector':
        N = r.uniform(0.5, 2.0, n)
        Nm = np.diag(N)
    else:
        B = r.normal(size=(n, n))
        N = Nm = B @ B.T / n + np.eye(n)
    like = GaussianData.from_linear_model(A, y, N)
    theta = r.normal(size=(32, D))
    res = theta @ A.T - y
    want = -0.5 * np.einsum('ni,ij,nj->n', res, np.linalg.inv(Nm), res)
    np.testing.assert_allclose(like(theta), want, rtol=1e-11, atol=1e-11)
    assert like.max_loglike >= want.max() and like(like.mean) == like.max_loglike   # (the least-squares residual is the maximum)
    assert like.hip_like_id is None and like.hip_like_data['logl0'] == like.max_loglike


def test_refusals():
    from nnest_amd.likelihoods import GaussianData
    mu, P = gc.make_target(3, 0)
    bad = [dict(mean=mu),                                               # neither
           dict(mean=mu, cov=P, precision=P),                           # both
           dict(mean=mu[:2], precision=P),                              # shapes
           dict(mean=mu.reshape(1, 3), precision=P),
           dict(mean=mu, precision=P[:2]),
           dict(mean=[], precision=np.zeros((0, 0))),                   # x_dim outside 1 .. 128
           dict(mean=np.zeros(129), precision=np.eye(129)),
           dict(mean=mu, precision=P + np.triu(np.full((3, 3), 1e-6), 1)),   # not symmetric
           dict(mean=mu, precision=-P),                                 # not positive definite
           dict(mean=mu, cov=np.ones((3, 3))),                          # singular
           dict(mean=mu * np.nan, precision=P),                         # not finite
           dict(mean=mu, precision=P * np.inf),
           dict(mean=mu, precision=P, logl_max=np.inf)]
    for kw in bad:
        with pytest.raises(ValueError, match='GaussianData'):
            GaussianData(**kw)
    GaussianData(np.zeros(128), precision=np.eye(128))
    r = np.random.RandomState(2)
    A = r.normal(size=(10, 3))
    A[:, 2] = A[:, 0] + A[:, 1]                                          # the data do not determine theta
    with pytest.raises(ValueError, match='singular'):
        GaussianData.from_linear_model(A, r.normal(size=10), 1.0)
    with pytest.raises(ValueError, match='from_linear_model'):
        GaussianData.from_linear_model(r.normal(size=(10, 3)), r.normal(size=9), 1.0)
    with pytest.raises(ValueError, match='from_linear_model'):
        GaussianData.from_linear_model(r.normal(size=(10, 3)), r.normal(size=10), np.ones(7))
    with pytest.raises(ValueError, match='positive'):
        GaussianData.from_linear_model(r.normal(size=(10, 3)), r.normal(size=10), -1.0)


@pytest.mark.parametrize('D', [1, 2, 33, 128])
def test_descriptor(D):
    like, mu, P = _like(D, D)
    assert like.hip_like_id is None and tuple(like.hip_like_params) == ()
    data = like.hip_like_data
    R = data['R']
    assert data['mu'].dtype == np.float32 and data['mu'].shape == (D,) and np.array_equal(data['mu'], mu.astype(np.float32))
    assert R.dtype == np.float32 and R.shape == (D, D) and R.flags['C_CONTIGUOUS']
    assert np.all(R[np.tril_indices(D, -1)] == 0.0) and np.all(np.diag(R) > 0)
    assert isinstance(data['logl0'], float) and data['logl0'] == -3.25
    # R^T R = P to float32 rounding: each entry is a sum of at most D products of float32-rounded factors
    R64 = R.astype(np.float64)
    slack = 2.0 ** -23 * (np.abs(R64).T @ np.abs(R64))
    assert np.all(np.abs(R64.T @ R64 - P) <= slack)
    assert np.array_equal(R, np.linalg.cholesky(P).T.astype(np.float32))


@pytest.mark.parametrize('D', [1, 2, 5, 33, 64, 128])
def test_bound_holds_for_three_orders_and_is_not_vacuous(D):
    like, mu, P = _like(D, 100 + D)
    data = like.hip_like_data
    r = np.random.RandomState(D)
    t = (mu + r.normal(size=(200, D)) * r.uniform(0.1, 3.0, size=(200, 1))).astype(np.float32)
    want, _, q = gc.exact(data, t)
    B = gc.bound(data, t)
    # not vacuous: a small fraction of the value it bounds
    assert np.all(B <= 1e-4 * (1.0 + q)) and np.all(B > 0)
    worst = 0.0
    for order in ('forward', 'reversed', 'pairwise'):
        got = gc.float32_eval(data, t, order)
        assert np.all(got <= data['logl0'])
        assert np.all(np.abs(got - want) <= B), (order, float(np.max(np.abs(got - want) / B)))
        worst = max(worst, float(np.max(np.abs(got - want) / B)))
    assert D == 1 or worst > 1e-3    # (the orders do differ from float64: the bound is of the error's own scale)
    # the host evaluation is that float64 value up to the rounding of mu and R to float32
    np.testing.assert_allclose(like(t.astype(np.float64)), want, rtol=1e-5, atol=1e-4)
    # a row equal to mu is logl0 exactly; a NaN or an infinity follows the safe rule
    odd = np.stack([data['mu'], data['mu'], data['mu']])
    odd[1, D - 1] = np.nan
    odd[2, 0] = np.inf
    for fn in (lambda v: gc.exact(data, v)[0], lambda v: gc.float32_eval(data, v, 'forward')):
        got = fn(odd)
        assert got[0] == data['logl0'] and got[1] == gc.SAFE and got[2] == gc.SAFE


def test_device_target_carries_the_data():
    from nnest_amd.device_target import DeviceTarget
    like, mu, P = _like(3, 1)
    t = DeviceTarget(None, (), np.ones(3), np.zeros(3), like_data=like.hip_like_data)
    assert t.like_id is None and t.like_data['logl0'] == -3.25 and np.array_equal(t.like_data['R'], like.hip_like_data['R'])
    with pytest.raises(AttributeError):
        t.like_data = None
    with pytest.raises(ValueError):
        t.like_data['mu'][0] = 1.0
    u = t.with_transform(2 * np.ones(3), np.ones(3))
    assert u.like_id is None and np.array_equal(u.like_data['mu'], t.like_data['mu']) and u.t_std[0] == 2.0
    for bad in (dict(like_id=None), dict(like_id=3, like_data=like.hip_like_data)):
        with pytest.raises(ValueError):
            DeviceTarget(**bad)
    plain = DeviceTarget(3, (0.5,))
    assert plain.like_data is None and plain.with_transform(np.ones(2), np.zeros(2)).like_data is None


class _Flow(object):
    """a flow as `_device_target` sees it, without a device"""
    device = 'cpu'

    def __init__(self, D, syms):
        self.D, self._sym = D, dict((s, None) for s in syms)
        self.asked = []

    def mcmc_gdata_refusal(self, D=None):
        self.asked.append(D)
        return self.refusal

    refusal = None


class _Trainer(object):
    def __init__(self, net):
        self.netG = net


def _bare_sampler(like, net):
    from nnest_amd.mcmc import MCMCSampler
    s = MCMCSampler.__new__(MCMCSampler)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = like.x_dim, 0, 0, _Trainer(net)
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = like, None, None, True, 1.0
    s.logger = logging.getLogger('test_gdata_check')
    return s


TODAY = 'a likelihood the kernels do not know (a Python callable)'
OLD = ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt', 'importance', 'ensemble')


def test_device_target_without_the_entry_answers_as_before():
    like, _, _ = _like(3, 2)
    s = _bare_sampler(like, _Flow(3, OLD))
    for entry in (None, 'mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt', 'importance'):
        assert s._device_target(entry=entry) == (None, TODAY), entry
    assert s.trainer.netG.asked == []
    # with the entry bound, the routes that are not Metropolis runs still answer as before, and nothing is asked or probed
    net = _Flow(3, OLD + ('mcmc_gdata', 'mcmc_gdata_check'))
    s = _bare_sampler(like, net)
    s._probe_agrees_gdata = lambda *a, **k: pytest.fail('no probe on a refused route')
    for entry in (None, 'importance'):
        assert s._device_target(entry=entry) == (None, TODAY), entry
    assert net.asked == []


def test_device_target_with_the_entry():
    like, _, _ = _like(3, 2)
    net = _Flow(3, OLD + ('mcmc_gdata', 'mcmc_gdata_check'))
    s = _bare_sampler(like, net)
    probes = []
    s._probe_agrees_gdata = lambda data, affine, warn='': probes.append(data) or True
    s._probe_agrees = lambda *a, **k: pytest.fail('the probe by id is not this likelihood\'s')
    for entry in ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt'):
        target, why = s._device_target(entry=entry)
        assert why is None and target.like_id is None and target.like_params == ()
        assert np.array_equal(target.like_data['R'], like.hip_like_data['R']) and target.like_data['logl0'] == -3.25
        assert target.lo is None and np.array_equal(target.t_std, np.ones(3, np.float32))
    assert net.asked == [3] * 4 and len(probes) == 4
    # the library's refusal, in its words; a disagreeing probe, in the words of every refused target
    net.refusal = 'mcmc gdata: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only'
    assert s._device_target(entry='mcmc') == (None, 'the flow _Flow: ' + net.refusal)
    net.refusal = None
    s._probe_agrees_gdata = lambda data, affine, warn='': False
    target, why = s._device_target(entry='mcmc')
    assert target is None and why.startswith('this transform, likelihood or prior')
    # derived or slow parameters are refused first, as for every likelihood
    s.num_slow = 1
    assert s._device_target(entry='mcmc')[1] == 'the fast/slow proposal (num_slow=1)'


def test_mcmc_steps_refuses_an_id_beside_the_data():
    from nnest_amd.flow import _HipFlow
    like, _, _ = _like(3, 2)
    net = _HipFlow.__new__(_HipFlow)
    net._sym = {}
    with pytest.raises(ValueError, match='like_data goes with like_id=None'):
        net.mcmc_steps(3, None, 2, 0.1, like_data=like.hip_like_data)
    with pytest.raises(NotImplementedError, match='Gaussian likelihood from user data'):
        net.mcmc_steps(None, None, 2, 0.1, like_data=like.hip_like_data)
    with pytest.raises(NotImplementedError, match='Gaussian likelihood from user data'):
        net.mcmc_gdata_refusal()
