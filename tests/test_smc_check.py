"""CPU checks of the sequential Monte Carlo sampler (include/nnest_hip.h nnest_smc_reweight, nnest_smc_resample,
nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps; nnest_amd/smc.py; tests/smc_check.py restates the pieces): the restated
reweighting, integer weights, systematic rule and tempered target; the log Z identity of a ladder against scipy's logsumexp; the
properties of the systematic rule; a numpy-only sampler on a target with a closed form, which pins the estimator and the convention of
log Z; the four entry points are declared, exported and bound within ABI 15 and answer their argument checks without a device; the
Python layers route to them: `mcmc_steps(beta=...)` selects the family's tempered entry, SMCSampler chooses its route from what it can
observe, names what the fused route does not take, and runs its host route on stub flows."""
import contextlib
import ctypes
import inspect
import logging
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp

from tests import smc_check as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_mcmc_tempered_steps', 'nnest_spline_mcmc_tempered_steps', 'nnest_smc_reweight', 'nnest_smc_resample')


def heavy_logl(rng, N, dead=0):
    """a Rosenbrock-like heavy-tailed log-likelihood sample, with some dead (-1e100) entries"""
    x = rng.uniform(-5, 5, size=(N, 2))
    logl = -(100.0 * (x[:, 1] - x[:, 0] ** 2) ** 2 + (1.0 - x[:, 0]) ** 2)
    if dead:
        logl[rng.choice(N, size=min(dead, N - 1), replace=False)] = -1e100
    return logl


# ---- the restatements ------------------------------------------------------------------------------------------------------
def test_reweight_rule():
    rng = np.random.RandomState(0)
    for N, frac in ((64, 0.5), (1000, 0.5), (1000, 0.9), (4099, 0.5)):
        logl = heavy_logl(rng, N, dead=N // 50)
        (b, inc, ess, mx), m = sc.reweight(logl, 0.0, frac)
        assert 0.0 < b < 1.0 and mx == logl.max()
        assert abs(ess - frac * N) <= 1e-6 * N   # (the bracket is 2^-64 wide: the ESS sits on its target)
        assert ess == pytest.approx(sc.ess_of(sc.weights(logl, 0.0, b)), rel=1e-15)
        assert inc == pytest.approx(logsumexp(b * logl) - np.log(N), rel=1e-12)
        assert m.dtype == np.int64 and m.max() == 2 ** 31 and m.min() >= 0 and np.all(m[logl == -1e100] == 0)
        np.testing.assert_array_equal(m, np.floor(np.exp(b * (logl - mx)) * 2.0 ** 31))
        # the next stage starts from b
        b2 = sc.next_beta(logl, b, frac)
        assert b < b2 <= 1.0
    # an easy population goes to 1 at once; the hardest one still advances
    flat = rng.normal(size=500) * 0.01
    assert sc.next_beta(flat, 0.0, 0.5) == 1.0 and sc.next_beta(flat, 0.7, 0.9) == 1.0
    spiky = np.array([0.0] + [-1e300] * 99)
    assert sc.next_beta(spiky, 0.0, 0.5) > 0.0
    assert sc.next_beta(spiky, 0.5, 0.5) == np.nextafter(0.5, 1.0)   # (ESS = 1 anywhere above 0.5: hi ends one ulp above beta -- it advances)
    assert sc.next_beta(np.full(10, -1e100), 0.0, 0.5) == 1.0   # (everything dead: equal weights)


def test_logz_identity_of_a_ladder_without_resampling():
    """the stage increments of a full ladder add up to log mean exp(logL) over the first population's draws (the weights carried,
    no resampling): the estimator is consistent whatever the ladder"""
    rng = np.random.RandomState(1)
    for N in (3, 64, 1000):
        logl = heavy_logl(rng, N, dead=N // 20)
        want = logsumexp(logl) - np.log(N)
        first = sc.next_beta(logl, 0.0, 0.5)
        for ladder in ([1.0], [first, 1.0], [first, 0.5 * (first + 1.0), 1.0], list(np.linspace(0.0, 1.0, 12)[1:])):
            total, beta = 0.0, 0.0
            for b in ladder:
                carried = sc.weights(logl, 0.0, beta)   # exp(beta (logL - max)): what the population weighs at beta
                total += sc.increment(logl, beta, b, carried=carried)
                beta = b
            assert total == pytest.approx(want, abs=1e-10, rel=1e-10), (N, ladder)
        assert sc.increment(logl, 0.0, first) == pytest.approx(logsumexp(first * logl) - np.log(N), abs=1e-10)


def test_systematic_rule():
    rng = np.random.RandomState(2)
    for N in (1, 3, 64, 1000, 4099):
        logl = heavy_logl(rng, N, dead=N // 10)
        m = sc.integer_weights(logl, 0.0, sc.next_beta(logl, 0.0, 0.5))
        T = int(m.sum())
        for u in (0.0, 1.0 - 2.0 ** -24, sc.smc_uniform(7, 3), 0.5):
            anc = sc.systematic(m, u)
            assert anc.shape == (N,) and anc.min() >= 0 and anc.max() < N   # (u = 0 and u = 1 - 2^-24 stay in range)
            assert np.all(np.diff(anc) >= 0)
            counts = np.bincount(anc, minlength=N)
            assert counts.sum() == N
            assert np.all(np.abs(counts - N * m / float(T)) < 1.0 + 1e-9)
            assert np.all(counts[m == 0] == 0)
    # a single live weight: that index, N times, whatever u
    m = np.zeros(50, np.int64)
    m[17] = 5
    for u in (0.0, 0.3, 1.0 - 2.0 ** -24):
        np.testing.assert_array_equal(sc.systematic(m, u), np.full(50, 17))
    # the largest sums the kernel meets (N = 2^20 weights of 2^31) keep every position exact and in range
    m = np.full(sc.MAX_N, 2 ** 31, np.int64)
    for u in (0.0, 1.0 - 2.0 ** -24):
        np.testing.assert_array_equal(sc.systematic(m, u), np.arange(sc.MAX_N))


def test_stream_8_word():
    us = [sc.smc_uniform(11, s) for s in range(200)]
    assert all(0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24) for u in us) and len(set(us)) > 190
    assert abs(np.mean(us) - 0.5) < 4.0 / np.sqrt(12 * 200)
    assert sc.smc_uniform(11, 5) == us[5] and sc.smc_uniform(12, 5) != us[5] and sc.smc_uniform((3 << 40) + 11, 5) != us[5]
    # not the random walk's accept draw of (walker 5, step 0), which differs in the stream alone
    from tests.mcmc_walk_check import mcmc_draws
    assert float(mcmc_draws(11, 5, 1, 0, 1, 1)[1][0, 0]) != us[5]


def test_tempered_target():
    from tests.ensemble_check import latent_target
    rng = np.random.RandomState(3)
    x_of_z = lambda q: (np.asarray(q, np.float64) * 1.5, np.full(len(q), 0.25))
    logl = lambda x: -0.5 * np.sum(x * x, axis=1) - 3.0
    box = lambda x: np.all(np.abs(x) <= 2.0, axis=1)
    q = rng.normal(size=(200, 3)).astype(np.float32)
    one = sc.tempered_target(x_of_z, logl, box, 1.0)(q)
    np.testing.assert_array_equal(one.view(np.uint64), latent_target(x_of_z, logl, box)(q).view(np.uint64))   # 1.0 * logL is exact
    zero = sc.tempered_target(x_of_z, logl, box, 0.0)(q)
    inside = box(x_of_z(q)[0])
    assert inside.any() and (~inside).any()
    assert np.all(zero[inside] == 0.25) and np.all(zero[~inside] == -np.inf)
    third = sc.tempered_target(x_of_z, logl, box, 0.3)(q)
    np.testing.assert_array_equal(third[inside], (0.3 * logl(x_of_z(q)[0]) + 0.25)[inside])
    dead = sc.tempered_target(x_of_z, lambda x: np.full(len(x), -1e100), box, 0.0)(q)   # (the safe value: 0 * -1e100 = -0)
    assert np.all(dead[inside] == 0.25)


def gauss_logl(corr):
    from nnest_amd.likelihoods import Gaussian
    return lambda D: Gaussian(D, corr)


def test_numpy_smc_pins_the_estimator_and_its_convention():
    """Gaussian(4, 0.5) in the +-6 box: the normalised N(0, Sigma) has all but 1e-8 of its mass inside, so log Z with the NORMALISED
    prior is -4 log 12; the mean over 8 seeds within 4 standard errors from those seeds' own scatter"""
    like = gauss_logl(0.5)(4)
    got = []
    for seed in range(8):
        logz, betas, theta = sc.numpy_smc(like, [-6.0] * 4, [6.0] * 4, 512, 10, 0.5, np.random.RandomState(100 + seed))
        assert betas[-1] == 1.0 and np.all(np.diff([0.0] + betas) > 0) and np.all(np.abs(theta) <= 6.0)
        got.append(logz)
    se = np.std(got, ddof=1) / np.sqrt(len(got))
    print('numpy SMC: log Z %.4f +- %.4f over %d seeds (exact %.4f), %d stages' % (np.mean(got), se, len(got), -4 * np.log(12.0), len(betas)))
    assert 0.0 < se < 0.2
    assert abs(np.mean(got) + 4.0 * np.log(12.0)) <= 4.0 * se


# ---- the C boundary ----------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(nnest_[a-z0-9_]+)\s*\(', text))


def test_header_declares_and_library_exports_the_entries():
    from nnest_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    for fam in ('nnest_mcmc', 'nnest_spline_mcmc'):   # the sibling's arguments plus `double beta` before `stream`
        old, new = _lib.SIGNATURES[fam + '_steps'], _lib.SIGNATURES[fam + '_tempered_steps']
        assert new == old[:-1] + [ctypes.c_double] + old[-1:]
    assert lib.nnest_hip_version() == 15


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)
    for fn in (lib.nnest_mcmc_tempered_steps, lib.nnest_spline_mcmc_tempered_steps):
        def steps(h=None, like=L, z_in=p, x_out=p, C=8, S=2, step=0.5, beta=0.5):
            return fn(h, like, p, p, None, None, z_in, None, None, p, x_out, p, p, p, p, p, None, C, S, ctypes.c_float(step), 0, 0, 0,
                      ctypes.c_double(beta), None)

        for beta in (0.0, 0.3, 1.0, 7.5):   # (valid: the refusal is the handle's)
            assert steps(beta=beta) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error(), beta
        for beta in (float('nan'), -1.0, float('inf'), -float('inf'), -1e-300):
            assert steps(beta=beta) == E_ARG and b'beta' in lib.nnest_hip_last_error(), beta
        # the sibling's checks
        assert steps(like=None) == E_ARG and b'NULL' in lib.nnest_hip_last_error()
        assert steps(z_in=None) == E_ARG and b'NULL device buffer' in lib.nnest_hip_last_error()
        assert steps(x_out=None) == E_ARG and b'NULL device buffer' in lib.nnest_hip_last_error()
        assert steps(C=0) == E_ARG and b'C=0' in lib.nnest_hip_last_error()
        assert steps(S=-1) == E_ARG and b'steps=-1' in lib.nnest_hip_last_error()
        assert steps(step=float('nan')) == E_ARG and b'step_size' in lib.nnest_hip_last_error()

    def rw(logl=p, N=8, beta=0.0, frac=0.5, out=p, m=p):
        return lib.nnest_smc_reweight(logl, N, ctypes.c_double(beta), ctypes.c_double(frac), out, m, None)

    for name in ('logl', 'out', 'm'):
        assert rw(**{name: None}) == E_ARG and b'NULL' in lib.nnest_hip_last_error(), name
    for N in (0, -1, (1 << 20) + 1):
        assert rw(N=N) == E_ARG and b'N=' in lib.nnest_hip_last_error(), N
    for frac in (0.0, 1.0, -0.5, 1.5, float('nan')):
        assert rw(frac=frac) == E_ARG and b'ess_fraction' in lib.nnest_hip_last_error(), frac
    for beta in (1.0, -0.1, 2.0, float('nan'), float('inf')):
        assert rw(beta=beta) == E_ARG and b'beta' in lib.nnest_hip_last_error(), beta

    def rs(m=p, N=8, D=3, stage=0, theta_in=p, logl_in=p, anc=p, theta_out=ctypes.c_void_p(128), logl_out=ctypes.c_void_p(192)):
        return lib.nnest_smc_resample(m, N, D, 5, stage, theta_in, logl_in, anc, theta_out, logl_out, None)

    for name in ('m', 'theta_in', 'logl_in', 'anc', 'theta_out', 'logl_out'):
        assert rs(**{name: None}) == E_ARG and b'NULL' in lib.nnest_hip_last_error(), name
    for N in (0, (1 << 20) + 1):
        assert rs(N=N) == E_ARG and b'N=' in lib.nnest_hip_last_error(), N
    assert rs(D=0) == E_ARG and b'D=0' in lib.nnest_hip_last_error()
    assert rs(stage=-1) == E_ARG and b'stage' in lib.nnest_hip_last_error()
    assert rs(theta_out=p) == E_ARG and b'must not be the inputs' in lib.nnest_hip_last_error()
    assert rs(logl_out=p) == E_ARG and b'must not be the inputs' in lib.nnest_hip_last_error()


def test_refused_calls_leave_host_visible_outputs_untouched():
    """a refusal comes before any launch: buffers the host can see (plain host memory here, which no launch could take) keep their
    guard pattern"""
    from nnest_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_double * 4)(*([123.0] * 4))
    m = (ctypes.c_longlong * 8)(*([-7] * 8))
    logl = (ctypes.c_double * 8)(*range(8))
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for beta, frac, N in ((1.0, 0.5, 8), (0.0, 1.0, 8), (0.0, 0.0, 8), (float('nan'), 0.5, 8), (0.0, 0.5, 0)):
        assert lib.nnest_smc_reweight(cast(logl), N, ctypes.c_double(beta), ctypes.c_double(frac), cast(out), cast(m), None) == 1
    assert list(out) == [123.0] * 4 and list(m) == [-7] * 8
    x = (ctypes.c_float * 24)(*([55.0] * 24))
    lk = _lib.like_spec(3, 1.0, (0.5,))
    for fn in (lib.nnest_mcmc_tempered_steps, lib.nnest_spline_mcmc_tempered_steps):
        for beta in (float('nan'), -1.0, float('inf')):
            assert fn(None, ctypes.byref(lk), None, None, None, None, cast(x), None, None, cast(x), cast(x), cast(out), cast(out), None, None,
                      None, None, 4, 2, ctypes.c_float(0.5), 0, 0, 0, ctypes.c_double(beta), None) == 1
    assert list(x) == [55.0] * 24 and list(out) == [123.0] * 4


# ---- the Python layers -------------------------------------------------------------------------------------------------------
def bound(cls, family, **named):
    """an instance of the flow class with its C symbols bound as its constructor binds them, without a handle (no GPU)"""
    from nnest_amd import _lib
    o = object.__new__(cls)
    o._lib = _lib.load()
    o._h = None
    o._bind(family, **named)
    return o


def test_mcmc_steps_binds_the_entry_beta_selects(monkeypatch):
    import torch
    from nnest_amd import _lib, flow
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.flow import _HipFlow, HipNVP
    from nnest_amd.maf import HipMAF
    from nnest_amd.spline import HipSpline
    lib = _lib.load()
    assert "mcmc_tempered='nnest_mcmc_tempered_steps'" in inspect.getsource(HipNVP.__init__)
    assert "mcmc_tempered='nnest_spline_mcmc_tempered_steps'" in inspect.getsource(HipSpline.__init__)
    assert inspect.signature(_HipFlow.mcmc_steps).parameters['beta'].default is None
    assert callable(flow.smc_reweight) and callable(flow.smc_resample)
    monkeypatch.setattr(_lib, 'current_stream', lambda dev: None)   # (no device here: the calls below are refused before a launch)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    for cls, family, old, new in ((HipNVP, 'nnest_nvp', 'nnest_mcmc_steps', 'nnest_mcmc_tempered_steps'),
                                  (HipSpline, 'nnest_spline', 'nnest_spline_mcmc_steps', 'nnest_spline_mcmc_tempered_steps')):
        o = bound(cls, family, mcmc=old, mcmc_tempered=new)
        assert o._sym['mcmc'] is getattr(lib, old) and o._sym['mcmc_tempered'] is getattr(lib, new)
        o.device, o.D = torch.device('cpu'), 3
        # the library itself answers: no handle, so each entry refuses -- under its own name's argument list
        calls = []
        for key in ('mcmc', 'mcmc_tempered'):
            real = o._sym[key]
            o._sym[key] = (lambda real, key: lambda *a: (calls.append((key, len(a), a[-2])), real(*a))[1])(real, key)
        z = torch.zeros(4, 3)
        with pytest.raises(_lib.NnestHipError, match='NULL handle'):
            o.mcmc_steps(3, z, 2, 0.5, like_params=(0.5,))
        with pytest.raises(_lib.NnestHipError, match='NULL handle'):
            o.mcmc_steps(3, z, 2, 0.5, like_params=(0.5,), beta=0.5)
        with pytest.raises(_lib.NnestHipError, match='beta'):
            o.mcmc_steps(3, z, 2, 0.5, like_params=(0.5,), beta=-1.0)
        assert [c[:2] for c in calls] == [('mcmc', 24), ('mcmc_tempered', 25), ('mcmc_tempered', 25)]
        assert calls[1][2].value == 0.5 and calls[2][2].value == -1.0   # (beta sits before the stream)
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        o = bound(cls, family)
        o.device = 'cpu'
        assert 'mcmc_tempered' not in o._sym
        with pytest.raises(NotImplementedError, match='tempered'):
            o.mcmc_steps(3, None, 2, 0.5, beta=0.5)


class _IdentityFlow(object):
    """a flow that is the identity, on the CPU: what the host route asks of netG"""
    device = 'cpu'

    def __init__(self, D, tempered=True):
        self._sym = {'mcmc': object()}
        if tempered:
            self._sym['mcmc_tempered'] = object()
        self.D = D

    def forward(self, x):
        import torch
        x = torch.as_tensor(np.asarray(x, np.float32))
        return x, torch.zeros(len(x))

    inverse = forward


class _StubTrainer(object):
    def __init__(self, net):
        self.netG, self.trained = net, []

    def train(self, samples, jitter=0.0, **kw):
        self.trained.append((np.asarray(samples).copy(), jitter))


def _bare_sampler(D, like, prior, net, agrees=True):
    from nnest_amd.smc import SMCSampler
    s = SMCSampler.__new__(SMCSampler)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = D, 0, 0, _StubTrainer(net)
    s.total_calls = s.total_accepted = s.total_rejected = 0
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = like, prior, None, True, None
    s.transform = lambda x: x
    s.loglike, s.prior = s._checked_loglike, s._checked_prior
    s.sample_prior = getattr(prior, 'sample', None)
    s._probe_agrees = lambda like_id, params, **kw: agrees   # (the one step of _device_target that needs a device)
    s.single_or_primary_process = True
    s.logger = logging.getLogger('test_smc_check')
    s._seed_gen = None
    return s


def test_exported_and_constructed_as_mcmc_sampler():
    import nnest_amd
    from nnest_amd.mcmc import MCMCSampler
    from nnest_amd.sampler import Sampler
    from nnest_amd.smc import SMCSampler
    assert nnest_amd.SMCSampler is SMCSampler and issubclass(SMCSampler, Sampler)
    assert list(inspect.signature(SMCSampler.__init__).parameters) == list(inspect.signature(MCMCSampler.__init__).parameters)
    par = inspect.signature(SMCSampler.run).parameters
    assert [(k, v.default) for k, v in par.items() if k != 'self'] == [
        ('num_particles', 1000), ('mcmc_steps', 25), ('ess_fraction', 0.5), ('step_size', 0.0), ('jitter', 0.01), ('seed', None), ('route', None),
        ('max_stages', 1000)]
    assert "self.sampler = 'smc'" in inspect.getsource(SMCSampler.__init__)
    for name in ('_mcmc_sample', '_mcmc_sample_device', '_install_transform', '_device_target'):   # the base class's, untouched
        assert getattr(SMCSampler, name) is getattr(Sampler, name)


def test_host_route_on_a_stub_flow(caplog):
    """the whole host loop on the CPU: a Python likelihood, the identity for the flow.  Gaussian(3, 0.5) in the +-6 box"""
    from nnest_amd.priors import UniformPrior
    from nnest_amd.smc import SMCSampler, reweight_host, resample_host
    like = gauss_logl(0.5)(3)
    python_like = lambda x: like(x)
    got = []
    for seed in range(4):
        np.random.seed(seed)
        net = _IdentityFlow(3)
        s = _bare_sampler(3, python_like, UniformPrior(3, -6.0, 6.0), net)
        with caplog.at_level(logging.INFO, logger='test_smc_check'):
            assert s.run(num_particles=400, mcmc_steps=8, seed=seed) == s.logz
        assert s.smc_route == 'host'
        K = len(s.betas)
        assert K >= 3 and s.betas[-1] == 1.0 and np.all(np.diff([0.0] + s.betas) > 0)
        assert len(s.ess) == len(s.acceptance) == len(s.logz_steps) == len(s.stage_times) == K == len(s.trainer.trained)
        assert all(0.0 < a < 1.0 for a in s.acceptance) and sum(s.logz_steps) == pytest.approx(s.logz, rel=1e-12)
        assert all(set(t) == {'reweight', 'train', 'move'} for t in s.stage_times)
        assert all(j == 0.01 for _, j in s.trainer.trained)
        for x, _ in s.trainer.trained:   # the flow trains on the DISTINCT rows of the normalised population: no resampled copies
            assert len(np.unique(x, axis=0)) == len(x) and 400 // 4 < len(x) <= 400
            assert np.all(np.abs(x.mean(0)) < 0.3) and np.all(np.abs(x.std(0) - 1.0) < 0.3)
        assert any(len(x) < 400 for x, _ in s.trainer.trained)   # (a resampling at half the ESS does make copies)
        assert s.samples.shape == (400, 3) and s.loglikes.shape == (400,) and s.latent_samples.shape == (400, 3)
        np.testing.assert_allclose(s.loglikes, like(s.samples), rtol=1e-5, atol=1e-5)   # (theta = T(x) from a float32 x)
        assert np.all(np.abs(s.samples) <= 6.0)
        assert s.total_calls == 400 + K * 400 * (1 + 8) and s.total_accepted + s.total_rejected == K * 400 * 8
        got.append(s.logz)
    assert len([r for r in caplog.records if 'smc stage' in r.getMessage()]) >= K
    se = np.std(got, ddof=1) / 2.0
    assert abs(np.mean(got) + 3.0 * np.log(12.0)) <= 4.0 * se and se < 0.3
    # the product's numpy rules are the restatement's
    logl = heavy_logl(np.random.RandomState(5), 777, dead=20)
    (b, inc, ess, mx), m = reweight_host(logl, 0.1, 0.5)
    (b2, inc2, ess2, mx2), m2 = sc.reweight(logl, 0.1, 0.5)
    assert (b, mx) == (b2, mx2) and inc == pytest.approx(inc2, rel=1e-13) and ess == pytest.approx(ess2, rel=1e-13)
    np.testing.assert_array_equal(m, m2)
    np.testing.assert_array_equal(resample_host(m, 0.37), sc.systematic(m, 0.37))
    with pytest.raises(ValueError, match='sum to 0'):
        resample_host(np.zeros(5, np.int64), 0.5)


def test_front_end_chooses_and_names_its_route():
    from nnest_amd.priors import UniformPrior
    from nnest_amd.smc import stage_seed

    class _Like(object):
        hip_like_id = 3

        def __call__(self, x):
            return -0.5 * np.sum(np.asarray(x) ** 2, axis=1)

    prior = UniformPrior(2, -6.0, 6.0)

    def fused_stub(s, record):
        s._smc_start_fused = lambda N, target: ('theta', 'logl', None)

        def stage(state, beta, ess_fraction, S, step_size, jitter, seed, stage, target):
            record.append((beta, ess_fraction, S, step_size, jitter, seed, stage))
            return min(1.0, beta + 0.4), -1.0, 50.0, 0.25, (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2))), dict(reweight=0, train=0, move=0)
        s._smc_stage_fused = stage

    # a likelihood the kernels know, a UniformPrior, a flow with a tempered entry: route=None runs fused
    rec = []
    s = _bare_sampler(2, _Like(), prior, _IdentityFlow(2))
    fused_stub(s, rec)
    s.run(num_particles=100, mcmc_steps=5, seed=9, step_size=0.0, jitter=0.02, ess_fraction=0.7)
    assert s.smc_route == 'fused' and s.betas == [0.4, 0.8, 1.0] and s.logz == -3.0 and s.logz_steps == [-1.0] * 3
    assert [r[6] for r in rec] == [0, 1, 2] and all(r[5] == 9 for r in rec)
    assert all(r[1:5] == (0.7, 5, 2 / 2 ** 0.5, 0.02) for r in rec)   # (step_size <= 0: 2 / sqrt(x_dim))
    assert len({stage_seed(9, k) for k in range(100)}) == 100 and stage_seed(9, 3) == stage_seed(9, 3) != stage_seed(10, 3)
    rec.clear()
    s.run(num_particles=100, route='fused', seed=1)
    assert s.smc_route == 'fused' and len(rec) == 3
    with pytest.raises(RuntimeError, match='max_stages'):
        s.run(num_particles=100, seed=1, max_stages=2)
    # what the fused route does not take is named; route=None falls to the host loop
    python_like = lambda x: -0.5 * np.sum(np.asarray(x) ** 2, axis=1)
    for change, word in ((dict(_user_loglike=python_like), 'Python callable'), (dict(num_derived=1), 'derived'), (dict(num_slow=1), 'fast/slow')):
        s = _bare_sampler(2, _Like(), prior, _IdentityFlow(2))
        for k, v in change.items():
            setattr(s, k, v)
        with pytest.raises(ValueError, match='the fused route does not take .*%s' % word):
            s.run(num_particles=50, route='fused')
        assert s.trainer.trained == []   # (refused before anything is trained)
    s = _bare_sampler(2, _Like(), prior, _IdentityFlow(2, tempered=False))
    with pytest.raises(ValueError, match='_IdentityFlow .*tempered'):
        s.run(num_particles=50, route='fused')
    s.run(num_particles=50, mcmc_steps=2, seed=3)
    assert s.smc_route == 'host' and s.betas[-1] == 1.0
    s = _bare_sampler(2, _Like(), prior, _IdentityFlow(2), agrees=False)
    with pytest.raises(ValueError, match='prior'):
        s.run(num_particles=50, route='fused')
    # route='host' is honoured where the fused route would apply
    s = _bare_sampler(2, _Like(), prior, _IdentityFlow(2))
    fused_stub(s, rec)
    rec.clear()
    s.run(num_particles=50, mcmc_steps=2, seed=3, route='host')
    assert s.smc_route == 'host' and rec == []
    # a prior that cannot be sampled; bad arguments
    for bad_prior in (None, (lambda x: 0.0)):
        s = _bare_sampler(2, _Like(), bad_prior, _IdentityFlow(2))
        with pytest.raises(ValueError, match='Prior does not have sample method'):
            s.run(num_particles=50)
    s = _bare_sampler(2, _Like(), prior, _IdentityFlow(2))
    with pytest.raises(ValueError, match='route'):
        s.run(route='rounds')
    for kw in (dict(ess_fraction=0.0), dict(ess_fraction=1.0), dict(num_particles=1), dict(mcmc_steps=0)):
        with pytest.raises(ValueError):
            s.run(**kw)
