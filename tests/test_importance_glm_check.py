"""CPU checks of the importance-sampled evidence of a regression (include/nnest_hip.h nnest_importance_glm_evidence,
nnest_spline_importance_glm_evidence and their _check entries; HipNVP / HipSpline.importance_evidence with like_glm and prior_gauss,
importance_glm_refusal; Sampler._device_target(entry='importance') on a likelihoods.GLMData): the declarations, exports and
bindings; the argument errors that need no device; the routing with stub flows; and the numpy restatement
(tests/importance_glm_check.py) against the truth -- the float64 grid quadrature of L pi."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

from tests import glm_check as gk
from tests import importance_glm_check as igc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = 1   # NNEST_E_ARG
NEW = ('nnest_importance_glm_check', 'nnest_spline_importance_glm_check', 'nnest_importance_glm_evidence',
       'nnest_spline_importance_glm_evidence')


# ---- the library and the bindings ---------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from nnest_amd import _lib
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read(), flags=re.S)
    syms = set(re.findall(r'\b(nnest_[a-z0-9_]+)\s*\(', text))
    for s in NEW:
        assert s in syms, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    # the importance entries' arguments, the two descriptors in the place of `like`
    assert _lib.SIGNATURES['nnest_importance_glm_evidence'] == _lib.SIGNATURES['nnest_spline_importance_glm_evidence']
    assert len(_lib.SIGNATURES['nnest_importance_glm_evidence']) == len(_lib.SIGNATURES['nnest_importance_evidence']) + 1
    assert _lib.SIGNATURES['nnest_importance_glm_check'] == _lib.SIGNATURES['nnest_mcmc_glm_check'] == _lib.SIGNATURES['nnest_spline_importance_glm_check']
    assert lib.nnest_hip_version() == 15
    # the flows bind them
    for fname, names in (('flow.py', ('nnest_importance_glm_evidence', 'nnest_importance_glm_check')),
                         ('spline.py', ('nnest_spline_importance_glm_evidence', 'nnest_spline_importance_glm_check'))):
        src = open(os.path.join(ROOT, 'nnest_amd', fname)).read()
        assert "importance_glm='%s'" % names[0] in src and "importance_glm_check='%s'" % names[1] in src
    # the new units are built beside the existing ones, the spline unit with its siblings' flag
    mk = open(os.path.join(ROOT, 'nnest_amd', 'csrc', 'Makefile')).read()
    assert 'nnest_importance_glm.hip' in mk and 'nnest_spline_importance_glm.hip' in mk and 'nnest_importance.hip' in mk
    assert re.search(r'nnest_spline_importance_glm\.o: nnest_spline_importance_glm\.hip\n\t.*-mllvm -disable-machine-licm', mk)
    assert not re.search(r'nnest_importance_glm\.o: nnest_importance_glm\.hip\n', mk)   # (the pattern rule's flags, as nnest_importance.o)


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    for name in ('nnest_importance_glm_evidence', 'nnest_spline_importance_glm_evidence'):
        rc = getattr(lib, name)(None, None, None, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None)
        assert rc == E_ARG, name
        assert lib.nnest_hip_last_error()
        # a descriptor that is there, and sums, but no handle
        a = np.zeros((2, 64), np.float32)
        sums = np.full(4, 128.0)
        spec = _lib.GlmSpec(a.ctypes.data, a.ctypes.data, a.ctypes.data, 0.0, 40, 64, 2, 0)
        rc = getattr(lib, name)(None, ctypes.byref(spec), None, None, None, None, None, None, None, None, None, None, sums.ctypes.data, 0, 0, 0,
                                None)
        assert rc == E_ARG and b'NULL handle' in lib.nnest_hip_last_error(), name
        assert np.all(sums == 128.0)
    for name in ('nnest_importance_glm_check', 'nnest_spline_importance_glm_check'):
        assert getattr(lib, name)(None, 3) == E_ARG, name


def test_importance_evidence_refuses_what_does_not_go_together():
    from nnest_amd.flow import _HipFlow
    from nnest_amd.priors import GaussianPrior
    like = gk.make_like(3, 40, 'logistic', 2)
    prior = GaussianPrior(3, 0.0, 2.0).hip_gauss_prior
    net = _HipFlow.__new__(_HipFlow)
    net._sym = {}
    with pytest.raises(ValueError, match='like_glm goes with like_id=None'):
        net.importance_evidence(3, 8, like_glm=like.hip_like_glm)
    with pytest.raises(ValueError, match='prior_gauss goes only with a like_glm'):
        net.importance_evidence(3, 8, prior_gauss=prior)
    with pytest.raises(ValueError, match='prior_gauss goes without lo / hi'):
        net.importance_evidence(None, 8, like_glm=like.hip_like_glm, prior_gauss=prior, lo=-np.ones(3), hi=np.ones(3))
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        net.importance_evidence(None, 8, like_glm=like.hip_like_glm)
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        net.importance_evidence(None, 8, like_glm=like.hip_like_glm, prior_gauss=prior)
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        net.importance_glm_refusal()
    with pytest.raises(NotImplementedError, match='no fused importance-sampling kernel for _HipFlow$'):
        net.importance_evidence(3, 8)


# ---- the routing ----------------------------------------------------------------------------------------------------------------------
class _Flow(object):
    """a flow as `_device_target` sees it, without a device"""
    device = 'cpu'
    refusal = None

    def __init__(self, D, syms):
        self.D, self._sym = D, dict((s, None) for s in syms)
        self.asked = []

    def importance_glm_refusal(self, D=None):
        self.asked.append(D)
        return self.refusal

    def importance_refusal(self, like_id):
        pytest.fail('the check by id is not this likelihood\'s')

    def mcmc_glm_refusal(self, D=None):
        pytest.fail('the walk\'s check is not the evidence\'s')

    mcmc_glm_prior_refusal = mcmc_gdata_refusal = mcmc_glm_refusal


class _Trainer(object):
    def __init__(self, net):
        self.netG = net


def _bare_sampler(like, net, prior=None, cls_name='MCMCSampler'):
    import nnest_amd
    cls = getattr(nnest_amd, cls_name)
    s = cls.__new__(cls)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = like.x_dim, 0, 0, _Trainer(net)
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = like, prior, None, True, 1.0
    s.logger = logging.getLogger('test_importance_glm_check')
    return s


def _probes(s):
    seen = dict(glm=[], gauss=[])
    s._probe_agrees_glm = lambda data, affine, warn='': seen['glm'].append(data) or True
    s._probe_agrees_gauss_prior = lambda data, affine, warn='': seen['gauss'].append(data) or True
    s._probe_agrees = lambda *a, **k: pytest.fail('the probe by id is not this likelihood\'s')
    s._probe_agrees_gdata = lambda *a, **k: pytest.fail('the Gaussian descriptor\'s probe is not this likelihood\'s')
    return seen


TODAY = 'a likelihood the kernels do not know (a Python callable)'
OLD = ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt', 'importance', 'ensemble', 'mcmc_gdata', 'mcmc_gdata_check', 'mcmc_glm',
       'mcmc_glm_check', 'mcmc_glm_prior', 'mcmc_glm_prior_check')
BOUND = OLD + ('importance_glm', 'importance_glm_check')


@pytest.mark.parametrize('family', gk.FAMILIES)
def test_device_target_with_a_uniform_prior(family):
    from nnest_amd.priors import UniformPrior
    like = gk.make_like(3, 40, family, 2)
    net = _Flow(3, BOUND)
    s = _bare_sampler(like, net, UniformPrior(3, -4.0, 4.0))
    seen = _probes(s)
    target, why = s._device_target(entry='importance', unit_box_on_x=True)
    assert why is None and target.like_id is None and target.like_params == () and target.like_data is None and target.prior_gauss is None
    assert np.array_equal(target.like_glm['at'], like.hip_like_glm['at']) and target.like_glm['family'] == family
    assert np.all(np.asarray(target.lo) == -4.0) and np.all(np.asarray(target.hi) == 4.0)
    assert net.asked == [3] and len(seen['glm']) == 1 and seen['gauss'] == []


def test_device_target_with_the_unit_box_on_x():
    like = gk.make_like(3, 40, 'logistic', 2)
    net = _Flow(3, BOUND)
    s = _bare_sampler(like, net, prior=None, cls_name='NestedSampler')
    s._unit_box_on_x = lambda: True
    s._user_transform, s._linear_scale = (lambda x: -5.0 * x), -5.0
    s._user_prior, s._transform_prior = (lambda x: np.zeros(len(x))), False
    seen = _probes(s)
    target, why = s._device_target(entry='importance', unit_box_on_x=True)
    assert why is None and target.like_glm is not None and target.prior_gauss is None
    assert np.all(np.asarray(target.lo) == -5.0) and np.all(np.asarray(target.hi) == 5.0) and np.all(np.asarray(target.t_std) == -5.0)
    assert net.asked == [3] and len(seen['glm']) == 1 and seen['gauss'] == []
    # the Metropolis entries do not know that box: without `unit_box_on_x` the likelihood stays a Python callable for the evidence
    assert s._device_target(entry='importance') == (None, TODAY)
    assert net.asked == [3]


def test_device_target_with_a_gaussian_prior():
    from nnest_amd.priors import GaussianPrior
    like = gk.make_like(3, 40, 'poisson', 2)
    prior = GaussianPrior(3, [0.1, -0.2, 0.0], [2.0, 1.0, 0.5])
    net = _Flow(3, BOUND)
    s = _bare_sampler(like, net, prior)
    seen = _probes(s)
    target, why = s._device_target(entry='importance', unit_box_on_x=True)
    assert why is None and target.like_glm is not None and target.lo is None and target.hi is None
    assert np.array_equal(target.prior_gauss['m'], prior.hip_gauss_prior['m']) and target.prior_gauss['logc'] == prior.hip_gauss_prior['logc']
    assert net.asked == [3] and len(seen['glm']) == 1 and len(seen['gauss']) == 1
    # taken on the `importance_glm` symbol, not on `mcmc_glm_prior`
    net2 = _Flow(3, tuple(k for k in BOUND if not k.startswith('mcmc_glm_prior')))
    s2 = _bare_sampler(like, net2, prior)
    _probes(s2)
    target, why = s2._device_target(entry='importance', unit_box_on_x=True)
    assert why is None and target.prior_gauss is not None and net2.asked == [3]

    # a subclass with a rule of its own stays a Python prior: no proper prior the kernels know, today's sentence
    class Mine(GaussianPrior):
        def __call__(self, x):
            return GaussianPrior.__call__(self, x) - 1.0

    s3 = _bare_sampler(like, _Flow(3, BOUND), Mine(3, 0.0, 1.0))
    _probes(s3)
    assert s3._device_target(entry='importance', unit_box_on_x=True) == (None, TODAY)
    assert s3.trainer.netG.asked == []


def test_device_target_answers_as_before_where_it_did():
    from nnest_amd.priors import GaussianPrior, UniformPrior
    like = gk.make_like(3, 40, 'logistic', 2)
    # no prior: the integral of the likelihood over R^D is not an evidence -- today's sentence, nothing asked or probed
    net = _Flow(3, BOUND)
    s = _bare_sampler(like, net)
    s._probe_agrees_glm = lambda *a, **k: pytest.fail('no probe on a refused route')
    assert s._device_target(entry='importance', unit_box_on_x=True) == (None, TODAY)
    assert net.asked == []
    # without the symbol: today's answer under every prior, nothing asked or probed
    for prior in (None, UniformPrior(3, -4.0, 4.0), GaussianPrior(3, 0.0, 2.0)):
        net = _Flow(3, OLD)
        s = _bare_sampler(like, net, prior)
        s._probe_agrees_glm = s._probe_agrees_gauss_prior = lambda *a, **k: pytest.fail('no probe on a refused route')
        assert s._device_target(entry='importance', unit_box_on_x=True) == (None, TODAY)
        assert net.asked == []
    # the library's refusal, in its words; a disagreeing probe, in the words of every refused target
    net = _Flow(3, BOUND)
    s = _bare_sampler(like, net, GaussianPrior(3, 0.0, 2.0))
    _probes(s)
    net.refusal = 'importance: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only'
    assert s._device_target(entry='importance', unit_box_on_x=True) == (None, 'the flow _Flow: ' + net.refusal)
    net.refusal = None
    s._probe_agrees_gauss_prior = lambda data, affine, warn='': False
    target, why = s._device_target(entry='importance', unit_box_on_x=True)
    assert target is None and why.startswith('this transform, likelihood or prior') and why.endswith('or a GaussianPrior with a GLMData)')
    _probes(s)
    s._probe_agrees_glm = lambda data, affine, warn='': False
    target, why = s._device_target(entry='importance', unit_box_on_x=True)
    assert target is None and why.startswith('this transform, likelihood or prior')
    # derived or slow parameters are refused first, as for every likelihood
    s.num_slow = 1
    assert s._device_target(entry='importance')[1] == 'the fast/slow proposal (num_slow=1)'


# ---- the restatement against the truth ----------------------------------------------------------------------------------------------
def oracle_nvp(D, seed):
    """the oracle's RealNVP on HipNVP's default_init(seed): no device is needed for the initialisation"""
    from nnest_amd.flow import HipNVP
    from oracle import oracle as orc
    o = object.__new__(HipNVP)
    o.D, o.H, o.B, o.L, o.scale = D, 16, 3, 1, ''
    o.num_params = 2 * 3 * (16 * D + 16 + (16 * 16 + 16) + D * 16 + D)
    return orc.NVP(D, 16, 3, 1, o.default_init(seed))


# M was chosen here on the CPU: at 2^14 the restated estimate's own standard error is 0.0034 (logistic) and 0.0031 (poisson), far
# under 0.1, with an ESS of 0.84 M and 0.87 M, and it lies 0.3 and 0.4 of them from the quadrature
M_TRUTH, FLOW_SEED, DRAW_SEED = 1 << 14, 4, 11


@pytest.mark.parametrize('family', gk.FAMILIES)
def test_the_restatement_against_the_quadrature(family):
    from nnest_amd.priors import GaussianPrior
    from tests.test_gpu_mcmc_glm_prior import posterior_draws, quadrature
    like = gk.make_like(2, 40, family, 5)
    prior = GaussianPrior(2, 0.0, 2.0)
    exact = quadrature(like, prior, -20.0, 20.0)[0]   # (ten sigma of the prior)
    train = posterior_draws(like, prior, np.random.RandomState(3), 2000)
    sd, mu = train.std(0).astype(np.float32), train.mean(0).astype(np.float32)   # T, as a front end installs it
    rs = igc.restated(oracle_nvp(2, FLOW_SEED), like.hip_like_glm, sd, mu, prior=prior)
    z = igc.importance_draws(DRAW_SEED, 0, M_TRUTH, 2)
    lw = igc.logw(rs, z)
    r = igc.estimate(lw, sd)
    print('%s: restated logz %.4f +- %.4f (quadrature %.4f), ESS %.0f of %d' % (family, r['logz'], r['logzerr'], exact, r['ess'], M_TRUTH))
    assert np.all(igc.is_live(lw))
    assert r['logzerr'] < 0.1
    assert abs(r['logz'] - exact) <= 5.0 * r['logzerr']
    # the pieces: logw + logb is (logL + log|det|) + log pi at the restated x
    x, ld = rs.x_of_z(z)
    # (to rounding: the subtraction of logb and its addition do not cancel to the bit)
    np.testing.assert_allclose(lw + igc.logb(z), (rs.logl(x) + np.asarray(ld, np.float64)) + igc.logprior(rs, x), rtol=1e-14, atol=0)
    # and the box form of the same model: the quadrature over the box, the UniformPrior the unnormalised indicator
    from tests.test_gpu_mcmc_glm import quadrature as box_quadrature
    rb = igc.restated(oracle_nvp(2, FLOW_SEED), like.hip_like_glm, sd, mu, half=4.0)
    lb = igc.logw(rb, z)
    e = igc.estimate(lb, sd)
    assert e['logzerr'] < 0.1 and abs(e['logz'] - box_quadrature(like, -4.0, 4.0)[0]) <= 5.0 * e['logzerr']
    assert not np.any(igc.near_face(igc.restated(oracle_nvp(2, FLOW_SEED), like.hip_like_glm, sd, mu), x, 1e-3))
