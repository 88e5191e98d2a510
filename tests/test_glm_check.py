"""CPU checks of the regression likelihoods of user data (nnest_amd.likelihoods.GLMData; include/nnest_hip.h nnest_glm_t): the host
evaluation, the refusals, the descriptor the kernels take, the a-priori bound of tests/glm_check.py against three legal summation
orders, the masked rows, DeviceTarget's new field, `_device_target` with fake flows, and the library's entries and their argument
errors, which need no device."""
import ctypes
import logging
import math
import os
import re

import numpy as np
import pytest

from tests import glm_check as gk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_loglike_glm', 'nnest_mcmc_glm_steps', 'nnest_spline_mcmc_glm_steps', 'nnest_mcmc_glm_check', 'nnest_spline_mcmc_glm_check')


# ---- the likelihood on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_host_evaluation(family):
    from nnest_amd.likelihoods import GLMData
    A, y, o = gk.make_data(4, 37, family, 3)
    like = GLMData(A, y, family=family, offset=o, logl_const=-1.5)
    x = np.random.RandomState(1).normal(size=(16, 4))
    eta = o + x @ A.T
    if family == 'logistic':
        p = 1.0 / (1.0 + np.exp(-eta))
        want = -1.5 + np.sum(y * np.log(p) + (1 - y) * np.log1p(-p), axis=1)
    else:
        try:
            from scipy.special import gammaln
            lg = gammaln(y + 1.0)
        except ImportError:
            lg = np.array([math.lgamma(v + 1.0) for v in y])
        want = -1.5 + np.sum(y * eta - np.exp(eta) - lg, axis=1)
        assert like.logl0 == -1.5 - float(np.sum(lg))
        assert abs(like.logl0 - (-1.5 - sum(math.lgamma(v + 1.0) for v in y))) <= 1e-12 * abs(like.logl0)
    np.testing.assert_allclose(like(x), want, rtol=1e-12, atol=1e-12)
    assert like.num_evaluations == 16 and like.x_dim == 4 and like.hip_like_id is None and tuple(like.hip_like_params) == ()
    assert like(x[0]) == like(x)[0]
    if family == 'logistic':
        assert np.all(like(50 * x) <= -1.5)
    assert like(np.full(4, np.nan)) == gk.SAFE and like(np.full((1, 4), np.inf))[0] == gk.SAFE
    # no offset is an offset of zeros
    np.testing.assert_array_equal(GLMData(A, y, family=family)(x), GLMData(A, y, family=family, offset=np.zeros(37))(x))


def test_refusals():
    from nnest_amd.likelihoods import GLMData
    r = np.random.RandomState(0)
    A, y = r.normal(size=(10, 3)), (r.uniform(size=10) < 0.5).astype(float)
    bad = [dict(A=A, y=y[:9]),                                          # shapes
           dict(A=A[0], y=y),
           dict(A=A, y=y.reshape(10, 1)),
           dict(A=A, y=y, offset=np.zeros(9)),
           dict(A=np.zeros((0, 3)), y=np.zeros(0)),                      # n outside 1 .. 65536
           dict(A=np.zeros((65537, 1)), y=np.zeros(65537)),
           dict(A=np.zeros((4, 0)), y=np.zeros(4)),                      # x_dim outside 1 .. 128
           dict(A=np.zeros((4, 129)), y=np.zeros(4)),
           dict(A=A * np.nan, y=y),                                      # not finite
           dict(A=A, y=y, offset=np.full(10, np.inf)),
           dict(A=A, y=y, logl_const=np.nan),
           dict(A=A, y=y * np.nan),
           dict(A=A, y=y + 0.5),                                         # logistic: y in {0, 1}
           dict(A=A, y=2 * y),
           dict(A=A, y=y - 1.0, family='poisson'),                       # poisson: counts
           dict(A=A, y=y + 0.5, family='poisson'),
           dict(A=A, y=y, family='probit')]
    for kw in bad:
        with pytest.raises(ValueError, match='GLMData'):
            GLMData(**kw)
    GLMData(np.zeros((1, 128)), np.zeros(1))
    GLMData(np.zeros((65536, 1)), np.zeros(65536), family='poisson')
    GLMData(A, 3 * y, family='poisson')


@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_descriptor(family, n):
    D = 5
    like = gk.make_like(D, n, family, n)
    data = like.hip_like_glm
    ld = (n + 63) // 64 * 64
    assert set(data) == {'at', 'y', 'o', 'logl0', 'n', 'family'} and data['n'] == n and data['family'] == family
    assert data['at'].dtype == np.float32 and data['at'].shape == (D, ld) and data['at'].flags['C_CONTIGUOUS']
    assert data['y'].dtype == np.float32 and data['y'].shape == (ld,) and data['o'].dtype == np.float32 and data['o'].shape == (ld,)
    assert np.array_equal(data['at'][:, :n], like.A.T.astype(np.float32)) and np.all(data['at'][:, n:] == 0)
    assert np.array_equal(data['y'][:n], like.y.astype(np.float32)) and np.all(data['y'][n:] == 0) and np.all(data['o'][n:] == 0)
    assert isinstance(data['logl0'], float) and data['logl0'] == like.logl0
    lg = sum(math.lgamma(v + 1.0) for v in like.y) if family == 'poisson' else 0.0
    assert abs(data['logl0'] - (gk.LOGL0 - lg)) <= 1e-12 * (1.0 + lg) and (family == 'poisson' or data['logl0'] == gk.LOGL0)
    assert not hasattr(like, 'hip_like_data')


# ---- the bound ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D,n', [(1, 1), (2, 63), (5, 64), (33, 65), (64, 200), (128, 40)])
def test_bound_holds_for_three_orders_and_is_not_vacuous(family, D, n):
    like = gk.make_like(D, n, family, 100 + D)
    data = like.hip_like_glm
    r = np.random.RandomState(D)
    t = (r.normal(size=(120, D)) * r.uniform(0.1, 3.0, size=(120, 1))).astype(np.float32)
    want, eta, l = gk.exact(data, t)
    B = gk.bound(data, t)
    size = abs(data['logl0']) + np.sum(np.abs(l), axis=1)
    # not vacuous: a small fraction of the value it bounds (gamma_{D + 2} is 1.6e-5 at x_dim 128, times sum |A| |t| over |l|)
    assert np.all(B > 0) and np.all(B <= 1e-3 * (1.0 + size))
    worst = 0.0
    for order in ('forward', 'reversed', 'pairwise'):
        got = gk.float32_eval(data, t, order)
        if family == 'logistic':
            assert np.all(got <= data['logl0'])
        assert np.all(np.abs(got - want) <= B), (order, float(np.max(np.abs(got - want) / B)))
        worst = max(worst, float(np.max(np.abs(got - want) / B)))
    # the orders do differ from float64; B adds magnitudes over the D products and the n rows where the roundings themselves
    # partly cancel, so the share of it in use falls about as 1 / sqrt(D n)
    assert worst > 1e-4
    # the host evaluation is that float64 value up to the rounding of the data to float32
    np.testing.assert_allclose(like(t.astype(np.float64)), want, rtol=1e-5, atol=1e-4)
    # a NaN or an infinity follows the safe rule, whatever the signs of A and y
    odd = np.zeros((3, D), np.float32)
    odd[1, D - 1] = np.nan
    odd[2, 0] = np.inf
    for fn in (lambda v: gk.exact(data, v)[0], lambda v: gk.float32_eval(data, v, 'forward')):
        got = fn(odd)
        assert np.isfinite(got[0]) and got[0] != gk.SAFE and got[1] == gk.SAFE and got[2] == gk.SAFE
    if family == 'poisson':   # exp overflows in float64: the safe rule
        big = np.full((1, D), 3.0e4, np.float32) * np.sign(data['at'][:, 0])
        assert gk.exact(data, big)[0][0] == gk.SAFE


@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_masked_rows_contribute_nothing(family, n):
    D = 3
    like = gk.make_like(D, n, family, n)
    data = dict(like.hip_like_glm)
    t = np.random.RandomState(n).normal(size=(20, D)).astype(np.float32)
    clean = gk.float32_eval(data, t, 'forward')
    # all-zero rows beyond n would each count softplus(0) = log 2 (logistic) or -1 (poisson) were they not masked
    ld = data['at'].shape[1]
    unmasked = dict(data, n=ld)
    if ld > n:
        per_row = -np.log(2.0) if family == 'logistic' else -1.0
        np.testing.assert_allclose(gk.float32_eval(unmasked, t, 'forward') - clean, (ld - n) * per_row, rtol=1e-9)
    r = np.random.RandomState(7)
    dirty = dict(data, at=data['at'].copy(), y=data['y'].copy(), o=data['o'].copy())
    dirty['at'][:, n:] = r.normal(size=(D, ld - n)) * 1e6
    dirty['y'][n:] = 7.0
    dirty['o'][n:] = np.nan
    got = gk.float32_eval(dirty, t, 'forward')
    assert np.array_equal(got.view(np.uint64), clean.view(np.uint64))
    assert np.array_equal(gk.exact(dirty, t)[0].view(np.uint64), gk.exact(data, t)[0].view(np.uint64))


def test_posterior_mode_is_the_maximum():
    for family in gk.FAMILIES:
        like = gk.make_like(2, 40, family, 5)
        th, top = gk.posterior_mode(like, -3.0, 3.0)
        g = np.stack(np.meshgrid(np.linspace(-3, 3, 121), np.linspace(-3, 3, 121)), -1).reshape(-1, 2)
        assert top >= like.loglike_rows(g).max() - 1e-9


# ---- DeviceTarget and the routing ---------------------------------------------------------------------------------------------------
def test_device_target_carries_the_descriptor():
    from nnest_amd.device_target import DeviceTarget
    like = gk.make_like(3, 40, 'poisson', 1)
    t = DeviceTarget(None, (), np.ones(3), np.zeros(3), like_glm=like.hip_like_glm)
    assert t.like_id is None and t.like_data is None and t.like_glm['logl0'] == like.logl0 and t.like_glm['n'] == 40
    assert np.array_equal(t.like_glm['at'], like.hip_like_glm['at']) and t.like_glm['family'] == 'poisson'
    with pytest.raises(AttributeError):
        t.like_glm = None
    with pytest.raises(ValueError):
        t.like_glm['at'][0, 0] = 1.0
    u = t.with_transform(2 * np.ones(3), np.ones(3))
    assert u.like_id is None and np.array_equal(u.like_glm['y'], t.like_glm['y']) and u.t_std[0] == 2.0
    for bad in (dict(like_id=3, like_glm=like.hip_like_glm), dict(like_id=None, like_glm=like.hip_like_glm, like_data=dict(mu=[0.0], R=[[1.0]], logl0=0.0))):
        with pytest.raises(ValueError):
            DeviceTarget(**bad)
    # the call forms there were
    plain = DeviceTarget(3, (0.5,))
    assert plain.like_glm is None and plain.like_data is None and plain.with_transform(np.ones(2), np.zeros(2)).like_glm is None
    assert DeviceTarget(3, (0.5,), None, None, None, None, None).like_glm is None


class _Flow(object):
    """a flow as `_device_target` sees it, without a device"""
    device = 'cpu'

    def __init__(self, D, syms):
        self.D, self._sym = D, dict((s, None) for s in syms)
        self.asked = []

    def mcmc_glm_refusal(self, D=None):
        self.asked.append(D)
        return self.refusal

    def mcmc_gdata_refusal(self, D=None):
        pytest.fail('the Gaussian descriptor\'s check is not this likelihood\'s')

    refusal = None


class _Trainer(object):
    def __init__(self, net):
        self.netG = net


def _bare_sampler(like, net):
    from nnest_amd.mcmc import MCMCSampler
    s = MCMCSampler.__new__(MCMCSampler)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = like.x_dim, 0, 0, _Trainer(net)
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = like, None, None, True, 1.0
    s.logger = logging.getLogger('test_glm_check')
    return s


TODAY = 'a likelihood the kernels do not know (a Python callable)'
OLD = ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt', 'importance', 'ensemble', 'mcmc_gdata', 'mcmc_gdata_check')


def test_device_target_without_the_entry_answers_as_before():
    like = gk.make_like(3, 40, 'logistic', 2)
    s = _bare_sampler(like, _Flow(3, OLD))
    for entry in (None, 'mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt', 'importance'):
        assert s._device_target(entry=entry) == (None, TODAY), entry
    assert s.trainer.netG.asked == []
    # with the entry bound, the routes that are not Metropolis runs still answer as before, and nothing is asked or probed
    net = _Flow(3, OLD + ('mcmc_glm', 'mcmc_glm_check'))
    s = _bare_sampler(like, net)
    s._probe_agrees_glm = lambda *a, **k: pytest.fail('no probe on a refused route')
    for entry in (None, 'importance'):
        assert s._device_target(entry=entry) == (None, TODAY), entry
    assert net.asked == []


@pytest.mark.parametrize('family', gk.FAMILIES)
def test_device_target_with_the_entry(family):
    like = gk.make_like(3, 40, family, 2)
    net = _Flow(3, OLD + ('mcmc_glm', 'mcmc_glm_check'))
    s = _bare_sampler(like, net)
    probes = []
    s._probe_agrees_glm = lambda data, affine, warn='': probes.append(data) or True
    s._probe_agrees = lambda *a, **k: pytest.fail('the probe by id is not this likelihood\'s')
    s._probe_agrees_gdata = lambda *a, **k: pytest.fail('the Gaussian descriptor\'s probe is not this likelihood\'s')
    for entry in ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt'):
        target, why = s._device_target(entry=entry)
        assert why is None and target.like_id is None and target.like_params == () and target.like_data is None
        assert np.array_equal(target.like_glm['at'], like.hip_like_glm['at']) and target.like_glm['logl0'] == like.logl0
        assert target.like_glm['family'] == family and target.like_glm['n'] == 40
        assert target.lo is None and np.array_equal(target.t_std, np.ones(3, np.float32))
    assert net.asked == [3] * 4 and len(probes) == 4
    # the library's refusal, in its words; a disagreeing probe, in the words of every refused target
    net.refusal = 'mcmc glm: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only'
    assert s._device_target(entry='mcmc') == (None, 'the flow _Flow: ' + net.refusal)
    net.refusal = None
    s._probe_agrees_glm = lambda data, affine, warn='': False
    target, why = s._device_target(entry='mcmc')
    assert target is None and why.startswith('this transform, likelihood or prior')
    # derived or slow parameters are refused first, as for every likelihood
    s.num_slow = 1
    assert s._device_target(entry='mcmc')[1] == 'the fast/slow proposal (num_slow=1)'
    s.num_slow, s.num_derived = 0, 2
    assert s._device_target(entry='mcmc')[1] == 'derived parameters (num_derived=2)'


def test_mcmc_steps_refuses_an_id_or_the_other_descriptor_beside_this_one():
    from nnest_amd.flow import _HipFlow
    like = gk.make_like(3, 40, 'logistic', 2)
    net = _HipFlow.__new__(_HipFlow)
    net._sym = {}
    with pytest.raises(ValueError, match='like_glm goes with like_id=None and like_data=None'):
        net.mcmc_steps(3, None, 2, 0.1, like_glm=like.hip_like_glm)
    with pytest.raises(ValueError, match='like_glm goes with like_id=None and like_data=None'):
        net.mcmc_steps(None, None, 2, 0.1, like_glm=like.hip_like_glm, like_data=dict(mu=[0.0], R=[[1.0]], logl0=0.0))
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        net.mcmc_steps(None, None, 2, 0.1, like_glm=like.hip_like_glm)
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        net.mcmc_glm_refusal()


# ---- the library and the bindings ---------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(nnest_[a-z0-9_]+)\s*\(', text)), text


def test_header_declares_and_library_exports_the_entries():
    from nnest_amd import _lib
    from nnest_amd.flow import HipNVP
    from nnest_amd.spline import HipSpline
    lib = _lib.load()
    syms, text = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert re.search(r'\}\s*nnest_glm_t;', text) and 'NNEST_GLM_LOGISTIC 0' in text and 'NNEST_GLM_POISSON 1' in text
    assert _lib.GLM_FAMILIES == {'logistic': 0, 'poisson': 1}
    assert [f[0] for f in _lib.GlmSpec._fields_] == ['at_dev', 'y_dev', 'o_dev', 'logl0', 'n', 'ld', 'D', 'family']
    # the adaptive entries' arguments, the descriptor in the place of `like`
    assert _lib.SIGNATURES['nnest_mcmc_glm_steps'] == _lib.SIGNATURES['nnest_mcmc_adapt_steps'] == _lib.SIGNATURES['nnest_spline_mcmc_glm_steps']
    assert _lib.SIGNATURES['nnest_loglike_glm'] == _lib.SIGNATURES['nnest_loglike_gdata']
    assert _lib.SIGNATURES['nnest_mcmc_glm_check'] == _lib.SIGNATURES['nnest_mcmc_gdata_check'] == _lib.SIGNATURES['nnest_spline_mcmc_glm_check']
    assert lib.nnest_hip_version() == 15
    # the flows bind them
    for cls, names in ((HipNVP, ('nnest_mcmc_glm_steps', 'nnest_mcmc_glm_check')), (HipSpline, ('nnest_spline_mcmc_glm_steps', 'nnest_spline_mcmc_glm_check'))):
        src = open(os.path.join(ROOT, 'nnest_amd', 'flow.py' if cls is HipNVP else 'spline.py')).read()
        assert "mcmc_glm='%s'" % names[0] in src and "mcmc_glm_check='%s'" % names[1] in src
    # the new units are built beside the existing ones, the spline unit with its siblings' flag
    mk = open(os.path.join(ROOT, 'nnest_amd', 'csrc', 'Makefile')).read()
    assert 'nnest_mcmc_glm.hip' in mk and 'nnest_spline_mcmc_glm.hip' in mk and 'nnest_mcmc_gdata.hip' in mk
    assert re.search(r'nnest_spline_mcmc_glm\.o: nnest_spline_mcmc_glm\.hip\n\t.*-mllvm -disable-machine-licm', mk)


def test_argument_errors_are_reported_not_thrown():
    """every refusal comes before a launch, in the library's words, and leaves the outputs alone: the buffers here are host arrays
    holding a guard pattern (nothing reads or writes them: no device is needed)"""
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    guard = dict((name, np.full(64, 0x5A, np.uint8)) for name in ('z_out', 'x_out', 'lp_out', 'logl_out', 'n_acc', 'n_glob', 'step_out',
                                                                  'hist_step'))
    g = dict((name, ctypes.c_void_p(a.ctypes.data)) for name, a in guard.items())
    p = ctypes.c_void_p(64)   # (inputs; never dereferenced)
    err = lib.nnest_hip_last_error

    def spec(**kw):
        s = _lib.GlmSpec(64, 64, 64, -3.25, 40, 64, 5, 0)
        for key, val in kw.items():
            setattr(s, key, val)
        return s

    bad_specs = [(dict(at_dev=None), b'NULL at_dev, y_dev or o_dev'), (dict(y_dev=None), b'NULL at_dev, y_dev or o_dev'),
                 (dict(o_dev=None), b'NULL at_dev, y_dev or o_dev'), (dict(D=0), b'glm: D=0'), (dict(D=129), b'glm: D=129'),
                 (dict(n=0), b'glm: n=0'), (dict(n=65537, ld=65600), b'glm: n=65537'), (dict(ld=32), b'glm: ld=32'),
                 (dict(ld=100), b'glm: ld=100'), (dict(n=65, ld=64), b'glm: ld=64'), (dict(ld=65600), b'glm: ld=65600'),
                 (dict(family=2), b'glm: family=2'), (dict(family=-1), b'glm: family=-1'),
                 (dict(logl0=float('inf')), b'glm: logl0='), (dict(logl0=float('nan')), b'glm: logl0=')]
    good = spec()
    for fn in (lib.nnest_mcmc_glm_steps, lib.nnest_spline_mcmc_glm_steps):
        def steps(h=None, glm=good, lo=None, hi=None, z_out=g['z_out'], C=8, S=2, step=0.3, beta=1.0, k=2, n_glob=g['n_glob'], step_in=p,
                  step_out=g['step_out'], hist_step=g['hist_step'], A=5, rate=1.0, target=0.234):
            return fn(h, None if glm is None else ctypes.byref(glm), p, p, lo, hi, p, None, None, z_out, g['x_out'], g['lp_out'], g['logl_out'],
                      None, None, None, g['n_acc'], C, S, ctypes.c_float(step), 0, 0, 0, ctypes.c_double(beta), k, n_glob, step_in, step_out,
                      hist_step, ctypes.c_uint32(A), ctypes.c_double(rate), ctypes.c_double(target), None)

        # with nothing else wrong, the handle is what is missing: both families, the ends of the ranges
        assert steps() == E_ARG and b'NULL handle' in err()
        for ok in (dict(family=1), dict(n=1), dict(n=64), dict(n=65536, ld=65536), dict(D=1), dict(D=128), dict(ld=128)):
            assert steps(glm=spec(**ok)) == E_ARG and b'NULL handle' in err(), ok
        assert steps(glm=None) == E_ARG and b'glm is NULL' in err()
        for kw, words in bad_specs:
            assert steps(glm=spec(**kw)) == E_ARG and words in err(), (kw, err())
        # every argument error of the adaptive entries
        for bad in (-0.1, 1.5, float('nan')):
            assert steps(rate=bad) == E_ARG and b'mcmc adapt: adapt_rate=' in err()
        for bad in (0.0, 1.0, float('nan')):
            assert steps(target=bad) == E_ARG and b'mcmc adapt: target_accept=' in err()
        assert steps(k=-1) == E_ARG and b'global_every=-1' in err()
        for bad in (-0.5, float('nan'), float('inf')):
            assert steps(beta=bad) == E_ARG and b"the likelihood's power" in err()
        assert steps(C=0) == E_ARG and b'C=0' in err()
        assert steps(S=-1) == E_ARG and b'steps=-1' in err()
        assert steps(step=float('nan')) == E_ARG and b'step_size' in err()
        assert steps(z_out=None) == E_ARG and b'NULL device buffer' in err()
        assert steps(z_out=None, S=0) == E_ARG and b'NULL handle' in err()   # (steps = 0 writes no z)
        assert steps(lo=p) == E_ARG and b'both or neither' in err()
    for fn in (lib.nnest_mcmc_glm_check, lib.nnest_spline_mcmc_glm_check):
        assert fn(None, 3) == E_ARG and b'NULL handle' in err()
    # the likelihood alone: the descriptor's errors, a D that is not the descriptor's, N < 0; N = 0 launches nothing
    out = g['logl_out']
    assert lib.nnest_loglike_glm(None, p, out, 4, 5, None) == E_ARG and b'glm is NULL' in err()
    for kw, words in bad_specs:
        s = spec(**kw)
        assert lib.nnest_loglike_glm(ctypes.byref(s), p, out, 4, s.D, None) == E_ARG and words in err(), kw
    assert lib.nnest_loglike_glm(ctypes.byref(good), p, out, 4, 4, None) == E_ARG and b"the likelihood's D=5 is not D=4" in err()
    assert lib.nnest_loglike_glm(ctypes.byref(good), p, out, -1, 5, None) == E_ARG and b'N=-1' in err()
    assert lib.nnest_loglike_glm(ctypes.byref(good), None, out, 4, 5, None) == E_ARG and b'NULL device buffer' in err()
    assert lib.nnest_loglike_glm(ctypes.byref(good), None, None, 0, 5, None) == 0
    for name, a in guard.items():
        assert np.all(a == 0x5A), name
    # the refusal of a non-Gaussian base is worded as the siblings word it
    for unit in ('nnest_abi.hip', 'nnest_spline.hip'):
        text = open(os.path.join(ROOT, 'nnest_amd', 'csrc', unit)).read()
        assert '"mcmc glm: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only"' in text


def test_glm_spec_names_its_errors():
    torch = pytest.importorskip('torch')
    from nnest_amd import flow
    like = gk.make_like(3, 40, 'logistic', 2)
    data = like.hip_like_glm
    spec, keep = flow.glm_spec(dict(data, at=torch.as_tensor(data['at']), y=torch.as_tensor(data['y']), o=torch.as_tensor(data['o'])), 'cpu')
    assert (spec.n, spec.ld, spec.D, spec.family, spec.logl0) == (40, 64, 3, 0, like.logl0) and spec.at_dev == keep[0].data_ptr()
    assert flow.glm_spec(dict(data, family='poisson'), 'cpu')[0].family == 1 and flow.glm_spec(dict(data, family=1), 'cpu')[0].family == 1
    with pytest.raises(ValueError, match='like_glm: family'):
        flow.glm_spec(dict(data, family='probit'), 'cpu')
    with pytest.raises(ValueError, match='like_glm: at must be shaped'):
        flow.glm_spec(dict(data, y=data['y'][:40]), 'cpu')
