"""CPU checks of the adaptive walk (include/nnest_hip.h nnest_mcmc_adapt_steps; tests/mcmc_adapt_check.py restates it): the rule's
factor, guards, freezing and rounding point; that it finds the target acceptance on N(0, I) and the frozen chains keep the target; the
library exports the entries and their argument checks answer without a device; the bindings and the front ends hand the step on."""
import contextlib
import ctypes
import inspect
import logging
import math
import os
import re

import numpy as np
import pytest

from tests import mcmc_adapt_check as ac
from tests.mcmc_walk_check import numpy_draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_mcmc_adapt_steps', 'nnest_spline_mcmc_adapt_steps', 'nnest_mcmc_adapt_check', 'nnest_spline_mcmc_adapt_check')


def lp_gauss(q):
    q = np.asarray(q, np.float64)
    return -0.5 * np.sum(q * q, axis=1)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def test_factor_is_positive_over_the_allowed_arguments():
    below_one = np.nextafter(1.0, 0.0)
    tiny = np.nextafter(0.0, 1.0)
    for rate in (0.0, tiny, 0.3, 1.0):
        for target in (tiny, 0.234, 0.5, below_one):
            for t in (0, 1, 7, 10 ** 6, 2 ** 32 - 1):
                f = ac.adapt_factor(t, np.array([False, True]), rate, target)
                assert np.all(f > 0.0) and np.all(f <= 2.0), (rate, target, t, f)   # (in (0, 2); rounded, 2 is reached)
                assert f[0] <= 1.0 <= f[1]
    # rate 0 is no adaptation; the gain decays as 1 / sqrt(t + 1)
    assert np.array_equal(ac.adapt_factor(3, np.array([False, True]), 0.0, 0.234), [1.0, 1.0])
    assert ac.adapt_factor(3, np.array([True]), 1.0, 0.234)[0] == 1.0 + 0.5 * (1.0 - 0.234)
    assert ac.adapt_factor(0, np.array([False]), 1.0, 0.234)[0] == 1.0 + (0.0 - 0.234)


def test_clamp_and_the_nan_load():
    s = ac.clamp([np.nan, -1.0, 0.0, 1e-9, 1e-8, 0.5, 1e2, 1e3, np.inf, -np.inf])
    assert np.array_equal(s, [1e-8, 1e-8, 1e-8, 1e-8, 1e-8, 0.5, 1e2, 1e2, 1e2, 1e-8])
    assert ac.STEP_MIN == 1e-8 and ac.STEP_MAX == 1e2
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    assert re.search(r'#define NNEST_ADAPT_STEP_MIN 1e-8\b', text) and re.search(r'#define NNEST_ADAPT_STEP_MAX 1e2\b', text)
    # the update is clamped at both ends
    assert ac.adapt_update(np.array([1e2]), 0, np.array([True]), 1.0, 0.234)[0] == 1e2
    assert ac.adapt_update(np.array([1e-8]), 0, np.array([False]), 1.0, 0.234)[0] == 1e-8


def test_sigma_is_frozen_after_adapt_steps_and_on_global_steps():
    N, D, S, k, step0, A = 12, 3, 14, 3, 4, 11   # (step0 no multiple of k; steps 4 .. 17; global: 5, 8, 11, 14, 17)
    rng = np.random.RandomState(3)
    draws = numpy_draws(rng, N, D, S)
    z0 = rng.standard_normal((N, D)).astype(np.float32)
    sig0 = np.linspace(0.1, 2.0, N)
    out = ac.adapt_run(z0, lp_gauss(z0), draws, sig0, lp_gauss, k, A, step0=step0)
    hs, acc = out[4], out[7]
    prev = sig0
    for i in range(S):
        t = step0 + i
        if ac.kind(t, k) or t >= A:
            assert np.array_equal(hs[:, i], prev), t
        else:   # (a local adapting step moves every walker's step: the factor is never 1 at rate 1)
            assert np.all((hs[:, i] > prev) == acc[:, i]) and np.all(hs[:, i] != prev), t
        prev = hs[:, i]
    assert np.array_equal(hs, ac.adapt_replay(sig0, acc, k, A, 1.0, 0.234, step0=step0))
    # a cut is the same run: sigma is the whole of the state the rule adds
    a = ac.adapt_run(z0, lp_gauss(z0), draws[:5], sig0, lp_gauss, k, A, step0=step0)
    b = ac.adapt_run(a[0], a[1], draws[5:], a[4][:, -1], lp_gauss, k, A, step0=step0 + 5)
    assert np.array_equal(np.concatenate([a[4], b[4]], 1), hs) and np.array_equal(b[0], out[0])
    # adapt_steps = 0 at a common step is the mixed walk
    from tests.mcmc_mixed_check import mixed_run
    m = mixed_run(z0, lp_gauss(z0), draws, 0.7, lp_gauss, k, step0=step0)
    f = ac.adapt_run(z0, lp_gauss(z0), draws, float(np.float32(0.7)), lp_gauss, k, 0, step0=step0)
    assert np.array_equal(m[2], f[2]) and np.array_equal(m[4], f[5]) and np.array_equal(m[5], f[6])
    assert np.all(f[4] == float(np.float32(0.7)))


def test_the_proposal_uses_the_float32_rounding_of_sigma():
    N, D = 16, 5
    rng = np.random.RandomState(5)
    (eps, u), = numpy_draws(rng, N, D, 1)
    z0 = rng.standard_normal((N, D)).astype(np.float32)
    sigma = 0.3 + rng.uniform(size=N) * 1e-3   # (float64 values that float32 does not hold)
    assert np.all(sigma.astype(np.float32).astype(np.float64) != sigma)
    recs = []
    ac.adapt_run(z0, lp_gauss(z0), [(eps, u)], sigma, lp_gauss, 0, 1, records=recs)
    q = recs[0]['q']
    assert q.dtype == np.float32
    assert np.array_equal(q, z0 + (np.float32(1) * sigma.astype(np.float32))[:, None] * eps)
    wide = (z0.astype(np.float64) + sigma[:, None] * eps.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(q, wide)   # (a float64 product rounded once is another proposal)


# ---- it finds the target acceptance, and the frozen chains keep N(0, I) ---------------------------------------------------------
@pytest.mark.parametrize('D', [5, 20])
@pytest.mark.parametrize('start', [0.02, 5.0])
def test_adapts_on_a_gaussian(D, start):
    """2000 walkers on N(0, I) from exact draws, 100 adapting and 100 frozen steps at adapt_rate 1.  The frozen acceptance is within
    0.05 of the target 0.234: the offsets seen were at most 0.014, and the binomial error of 2000 x 100 decisions is 0.001.  The
    sample variance of the ends is within 5 % of 1."""
    N, A, S = 2000, 100, 200
    rng = np.random.RandomState(100 * D + int(start))
    z0 = rng.standard_normal((N, D)).astype(np.float32)
    out = ac.adapt_run(z0, lp_gauss(z0), numpy_draws(rng, N, D, S), start, lp_gauss, 0, A)
    z, hs, acc = out[0], out[4], out[7]
    frozen = acc[:, A:].mean()
    sig = hs[:, -1]
    print('D %d start %g: frozen acceptance %.4f, geometric-mean step %.4f, sd of log step %.3f, variance %.4f' % (
        D, start, frozen, np.exp(np.log(sig).mean()), np.log(sig).std(), z.var()))
    assert np.array_equal(hs[:, A - 1], sig)
    assert abs(frozen - 0.234) <= 0.05
    assert abs(z.astype(np.float64).var() - 1.0) <= 0.05
    assert 0.5 * 2.38 / D ** 0.5 < np.exp(np.log(sig).mean()) < 2.0 * 2.38 / D ** 0.5   # (the optimal scaling's neighbourhood)


# ---- the library and the bindings ---------------------------------------------------------------------------------------------
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
    assert _lib.SIGNATURES['nnest_spline_mcmc_adapt_steps'] == _lib.SIGNATURES['nnest_mcmc_adapt_steps']   # one argument list
    # the mixed entry's arguments up to n_accept_global_dev, then (step_in, step_out, hist_step, adapt_steps, rate, target), the stream
    m = _lib.SIGNATURES['nnest_mcmc_mixed_steps']
    assert _lib.SIGNATURES['nnest_mcmc_adapt_steps'] == m[:-1] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_double, ctypes.c_double] + m[-1:]
    assert _lib.SIGNATURES['nnest_mcmc_adapt_check'] == _lib.SIGNATURES['nnest_mcmc_mixed_check']
    assert lib.nnest_hip_version() == 15
    # the existing units stay what they are: the new code is beside them
    mk = open(os.path.join(ROOT, 'nnest_amd', 'csrc', 'Makefile')).read()
    assert 'nnest_mcmc_adapt.hip' in mk and 'nnest_spline_mcmc_adapt.hip' in mk
    assert re.search(r'nnest_spline_mcmc_adapt\.o: nnest_spline_mcmc_adapt\.hip\n\t.*-mllvm -disable-machine-licm', mk)


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
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)
    for fn in (lib.nnest_mcmc_adapt_steps, lib.nnest_spline_mcmc_adapt_steps):
        def steps(h=None, like=L, lo=None, hi=None, z_out=g['z_out'], C=8, S=2, step=0.3, beta=1.0, k=2, n_glob=g['n_glob'], step_in=p,
                  step_out=g['step_out'], hist_step=g['hist_step'], A=5, rate=1.0, target=0.234):
            return fn(h, like, p, p, lo, hi, p, None, None, z_out, g['x_out'], g['lp_out'], g['logl_out'], None, None, None, g['n_acc'], C, S,
                      ctypes.c_float(step), 0, 0, 0, ctypes.c_double(beta), k, n_glob, step_in, step_out, hist_step, ctypes.c_uint32(A),
                      ctypes.c_double(rate), ctypes.c_double(target), None)

        err = lib.nnest_hip_last_error
        assert steps() == E_ARG and b'NULL handle' in err()
        # the new buffers are optional, adapt_steps = 0 and the ends of the rate's range are valid: the handle is what is missing
        assert steps(step_in=None, step_out=None, hist_step=None) == E_ARG and b'NULL handle' in err()
        assert steps(A=0) == E_ARG and b'NULL handle' in err()
        assert steps(A=2 ** 32 - 1) == E_ARG and b'NULL handle' in err()
        for ok in (0.0, 1.0):
            assert steps(rate=ok) == E_ARG and b'NULL handle' in err()
        for bad in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
            assert steps(rate=bad) == E_ARG and b'mcmc adapt: adapt_rate=' in err() and b'in [0, 1]' in err()
        for bad in (0.0, 1.0, -0.2, 1.2, float('nan'), float('inf')):
            assert steps(target=bad) == E_ARG and b'mcmc adapt: target_accept=' in err() and b'strictly inside (0, 1)' in err()
        for ok in (np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)):
            assert steps(target=float(ok)) == E_ARG and b'NULL handle' in err()
        # the mixed entry's own
        assert steps(k=0) == E_ARG and b'NULL handle' in err()
        assert steps(k=-1) == E_ARG and b'global_every=-1' in err()
        for bad in (-0.5, float('nan'), float('inf')):
            assert steps(beta=bad) == E_ARG and b"the likelihood's power" in err()
        assert steps(like=None) == E_ARG and b'NULL' in err()
        assert steps(C=0) == E_ARG and b'C=0' in err()
        assert steps(S=-1) == E_ARG and b'steps=-1' in err()
        assert steps(step=float('nan')) == E_ARG and b'step_size' in err()
        assert steps(z_out=None) == E_ARG and b'NULL device buffer' in err()
        assert steps(z_out=None, S=0) == E_ARG and b'NULL handle' in err()   # (steps = 0 writes no z)
        assert steps(lo=p) == E_ARG and b'both or neither' in err()
        bad_like = _lib.like_spec(99, 1.0)
        assert steps(like=ctypes.byref(bad_like)) == E_ARG and b'likelihood id' in err()
    for fn in (lib.nnest_mcmc_adapt_check, lib.nnest_spline_mcmc_adapt_check):
        assert fn(None, 3) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()
    for name, a in guard.items():
        assert np.all(a == 0x5A), name
    # the refusal of a non-Gaussian base is worded as the mixed and the importance checks word it
    for unit in ('nnest_abi.hip', 'nnest_spline.hip'):
        text = open(os.path.join(ROOT, 'nnest_amd', 'csrc', unit)).read()
        assert '"mcmc adapt: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only"' in text
        assert '"mcmc mixed: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only"' in text


def bound(cls, family, **named):
    """an instance of the flow class with its C symbols bound as its constructor binds them, without a handle (no GPU)"""
    from nnest_amd import _lib
    o = object.__new__(cls)
    o._lib = _lib.load()
    o._h = None
    o._bind(family, **named)
    return o


def test_mcmc_steps_binds_the_entry_the_new_keywords_select(monkeypatch):
    import torch
    from nnest_amd import _lib
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.flow import _HipFlow, HipNVP
    from nnest_amd.maf import HipMAF
    from nnest_amd.spline import HipSpline
    lib = _lib.load()
    for cls in (HipNVP, HipSpline):
        assert 'mcmc_steps' not in cls.__dict__ and cls.mcmc_steps is _HipFlow.mcmc_steps   # one body
        assert cls.mcmc_adapt_refusal is _HipFlow.mcmc_adapt_refusal
    assert "mcmc_adapt='nnest_mcmc_adapt_steps'" in inspect.getsource(HipNVP.__init__)
    assert "mcmc_adapt_check='nnest_mcmc_adapt_check'" in inspect.getsource(HipNVP.__init__)
    assert "mcmc_adapt='nnest_spline_mcmc_adapt_steps'" in inspect.getsource(HipSpline.__init__)
    assert "mcmc_adapt_check='nnest_spline_mcmc_adapt_check'" in inspect.getsource(HipSpline.__init__)
    par = inspect.signature(_HipFlow.mcmc_steps).parameters
    assert par['step_in'].default is None and par['adapt_steps'].default == 0
    assert par['adapt_rate'].default == 1.0 and par['target_accept'].default == 0.234
    monkeypatch.setattr(_lib, 'current_stream', lambda dev: None)   # (no device here: the calls below are refused before a launch)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    for cls, family, names in ((HipNVP, 'nnest_nvp', dict(mcmc='nnest_mcmc_steps', mcmc_mixed='nnest_mcmc_mixed_steps',
                                                           mcmc_adapt='nnest_mcmc_adapt_steps')),
                               (HipSpline, 'nnest_spline', dict(mcmc='nnest_spline_mcmc_steps', mcmc_mixed='nnest_spline_mcmc_mixed_steps',
                                                                mcmc_adapt='nnest_spline_mcmc_adapt_steps'))):
        o = bound(cls, family, **names)
        assert o._sym['mcmc_adapt'] is getattr(lib, names['mcmc_adapt'])
        o.device, o.D = torch.device('cpu'), 3
        calls = []
        for key in names:
            real = o._sym[key]
            o._sym[key] = (lambda real, key: lambda *a: (calls.append((key, a)), real(*a))[1])(real, key)
        z = torch.zeros(4, 3)
        kw = dict(like_params=(0.5,))
        # the library itself answers: no handle, so each entry refuses -- under its own name's argument list
        with pytest.raises(_lib.NnestHipError, match='NULL handle'):
            o.mcmc_steps(3, z, 2, 0.5, **kw)                                   # as it was
        with pytest.raises(_lib.NnestHipError, match='NULL handle'):
            o.mcmc_steps(3, z, 2, 0.5, global_every=2, **kw)                   # as it was
        with pytest.raises(_lib.NnestHipError, match='NULL handle'):
            o.mcmc_steps(3, z, 2, 0.5, adapt_steps=7, **kw)
        with pytest.raises(_lib.NnestHipError, match='NULL handle'):
            o.mcmc_steps(3, z, 2, 0.5, step_in=torch.full((4,), 0.25, dtype=torch.float64), global_every=3, beta=0.5, **kw)
        with pytest.raises(_lib.NnestHipError, match='adapt_rate'):
            o.mcmc_steps(3, z, 2, 0.5, adapt_steps=7, adapt_rate=2.0, **kw)
        with pytest.raises(_lib.NnestHipError, match='target_accept'):
            o.mcmc_steps(3, z, 2, 0.5, adapt_steps=7, target_accept=1.0, **kw)
        assert [(c[0], len(c[1])) for c in calls] == [('mcmc', 24), ('mcmc_mixed', 27)] + [('mcmc_adapt', 33)] * 4
        a = calls[2][1]   # (beta None -> 1.0, global_every 0, no counter of global steps, no step_in; out and history given)
        assert a[23].value == 1.0 and a[24] == 0 and a[25] is None and a[26] is None and a[27] and a[28]
        assert (a[29].value, a[30].value, a[31].value) == (7, 1.0, 0.234)
        a = calls[3][1]
        assert a[23].value == 0.5 and a[24] == 3 and a[25] and a[26] and (a[29].value, a[30].value, a[31].value) == (0, 1.0, 0.234)
        with pytest.raises(ValueError, match='adapt_steps=-1'):
            o.mcmc_steps(3, z, 2, 0.5, adapt_steps=-1, **kw)
        with pytest.raises(ValueError, match=r'step_in must be shaped \[4\]'):
            o.mcmc_steps(3, z, 2, 0.5, step_in=torch.zeros(5, dtype=torch.float64), **kw)
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        assert 'mcmc_adapt' not in inspect.getsource(cls.__init__)
        o = bound(cls, family)
        o.device = 'cpu'
        with pytest.raises(NotImplementedError, match='adaptive'):
            o.mcmc_steps(3, None, 2, 0.1, adapt_steps=2)
        with pytest.raises(NotImplementedError, match='adaptive'):
            o.mcmc_steps(3, None, 2, 0.1, step_in=np.ones(4))
        with pytest.raises(NotImplementedError):
            o.mcmc_adapt_refusal(3)


# ---- the front ends on stub flows ------------------------------------------------------------------------------------------------
class _StubFlow(object):
    """what the front ends ask of the flow, recorded.  Its rule: a launch that starts inside the adapting phase doubles every step and
    accepts every local step; a frozen launch keeps the steps and accepts no local step; global steps are always accepted"""
    device = 'cpu'

    def __init__(self, D, adapt=True):
        self._sym = {'mcmc': object(), 'mcmc_tempered': object(), 'mcmc_mixed': object()}
        if adapt:
            self._sym['mcmc_adapt'] = object()
        self.D, self.calls, self.refuse, self.asked = D, [], None, []

    def mcmc_adapt_refusal(self, like_id):
        self.asked.append(like_id)
        return self.refuse

    def mcmc_mixed_refusal(self, like_id):
        return None

    def forward(self, x):
        import torch
        return torch.as_tensor(np.asarray(x, np.float32)), None

    def mcmc_steps(self, like_id, z, steps, step_size, **kw):
        import torch
        C = z.shape[0]
        s0, k, A = kw.get('step0', 0), kw.get('global_every', 0), kw.get('adapt_steps')
        step_in = kw.get('step_in')
        self.calls.append((steps, s0, A, None if step_in is None else step_in.clone(), step_size, kw.get('target_accept'), kw.get('beta')))
        n_glob = sum(ac.kind(t, k) for t in range(s0, s0 + steps))
        adapting = A is not None and s0 < A
        out = dict(z=z, x=z, lp=torch.zeros(C, dtype=torch.float64), logl=torch.zeros(C, dtype=torch.float64),
                   hist_z=torch.zeros(C, steps, self.D), hist_x=torch.zeros(C, steps, self.D),
                   hist_logl=torch.zeros(C, steps, dtype=torch.float64),
                   n_accept=torch.full((C,), n_glob + (steps - n_glob if adapting or A is None else 0), dtype=torch.int32))
        if k:
            out['n_accept_global'] = torch.full((C,), n_glob, dtype=torch.int32)
        if A is not None or step_in is not None:
            start = torch.full((C,), float(np.float32(step_size)), dtype=torch.float64) if step_in is None else step_in
            grow = 2.0 * torch.linspace(1.0, 1.5, C, dtype=torch.float64) if adapting and steps > 0 else 1.0
            out['step'] = start * grow
        return out


class _StubTrainer(object):
    def __init__(self, net):
        self.netG = net

    def train(self, samples, jitter=0.0, **kw):
        pass


def _bare_sampler(D, net, cls=None):
    from nnest_amd.mcmc import MCMCSampler

    class _Like(object):
        hip_like_id, hip_like_params = 3, (0.5,)

    cls = cls or MCMCSampler
    s = cls.__new__(cls)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = D, 0, 0, _StubTrainer(net)
    s.total_calls = s.total_accepted = s.total_rejected = 0
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = _Like(), None, None, True, 1.0
    s.transform = lambda x: x
    s._probe_agrees = lambda like_id, params, **kw: True   # (the one step of _device_target that needs a device)
    s.single_or_primary_process = True
    s.chain_stats = False
    s.logger = logging.getLogger('test_mcmc_adapt_check')
    return s


def test_front_end_carries_the_step_across_launches_and_books_it(caplog):
    D, N, S, A = 3, 8, 23, 10
    net = _StubFlow(D)
    s = _bare_sampler(D, net)
    init = np.zeros((N, D), np.float32)
    with caplog.at_level(logging.INFO, logger='test_mcmc_adapt_check'):
        out = s._mcmc_sample_device(S, init_samples=init, seed=1, chunk_steps=7, global_every=5, adapt_steps=A, target_accept=0.3)
    assert out[0].shape == (N, S + 1, D)
    # the start as it was; then launches of 7, with the one across adapt_steps run as two
    assert [c[:3] for c in net.calls] == [(0, 0, None), (7, 0, A), (3, 7, A), (4, 10, A), (7, 14, A), (2, 21, A)] and net.asked == [3]
    assert all(c[5] == 0.3 for c in net.calls[1:])
    import torch
    grow = (2.0 * torch.linspace(1.0, 1.5, N, dtype=torch.float64)).numpy()   # (the stub's own factors)
    step0 = float(np.float32(2 / D ** 0.5))
    assert net.calls[1][3] is None
    assert np.array_equal(net.calls[2][3].numpy(), step0 * grow)           # step_out of one launch is step_in of the next
    for c in net.calls[3:]:
        assert np.array_equal(c[3].numpy(), (step0 * grow) * grow)
    assert np.array_equal(s.step_sizes, (step0 * grow) * grow) and s.step_sizes.shape == (N,)
    # global steps 4, 9 | 14, 19; local adapting steps 8 a chain, all accepted; local frozen steps 11 a chain, none accepted
    assert s.global_proposed == N * 4 and s.global_accepted == N * 4
    assert s.adapt_acceptance == 1.0 and s.frozen_acceptance == 0.0
    assert s.total_accepted == N * (8 + 4) and s.total_rejected == N * 11
    msg = [r.getMessage() for r in caplog.records if 'step adapted over' in r.getMessage()]
    assert msg and 'adapting acceptance' in msg[0] and 'frozen acceptance' in msg[0] and 'step mean' in msg[0]
    # a run that ends inside the adapting phase has no frozen steps
    s3 = _bare_sampler(D, _StubFlow(D))
    s3._mcmc_sample_device(6, init_samples=init, seed=1, adapt_steps=A)
    assert s3.adapt_acceptance == 1.0 and math.isnan(s3.frozen_acceptance)
    # 0: the call as it was -- no new keyword reaches the flow, nothing is asked of the library, nothing is left behind
    net2 = _StubFlow(D)
    s2 = _bare_sampler(D, net2)
    s2._mcmc_sample_device(S, init_samples=init, seed=1, chunk_steps=12)
    assert [c[:4] for c in net2.calls] == [(0, 0, None, None), (12, 0, None, None), (11, 12, None, None)] and net2.asked == []
    assert all(c[5] is None for c in net2.calls) and not hasattr(s2, 'step_sizes') and not hasattr(s2, 'adapt_acceptance')
    with pytest.raises(ValueError, match='adapt_steps=-1'):
        s2._mcmc_sample_device(S, init_samples=init, adapt_steps=-1)


def test_front_ends_name_what_the_adaptation_does_not_take():
    from nnest_amd.smc import SMCSampler
    D = 3
    train = np.random.RandomState(0).normal(size=(40, D))
    words = 'mcmc adapt: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only'
    net = _StubFlow(D)
    net.refuse = words
    s = _bare_sampler(D, net)
    with pytest.raises(ValueError, match=r'the fused route does not take the flow _StubFlow: mcmc adapt: GeneralisedNormal base'):
        s.run(5, 8, train, route='fused', adapt_steps=3)
    assert net.calls == []
    s = _bare_sampler(D, _StubFlow(D, adapt=False))   # a family without the kernel
    with pytest.raises(ValueError, match='no fused adaptive-step'):
        s.run(5, 8, train, route='fused', adapt_steps=3)
    s = _bare_sampler(D, _StubFlow(D))
    for route in (None, 'host'):   # worded as for global_every
        with pytest.raises(ValueError, match=r"adapt_steps=3 needs route='fused': .* built into the fused route's kernels only"):
            s.run(5, 8, train, route=route, adapt_steps=3)
    with pytest.raises(ValueError, match='adapt_steps=-1'):
        s.run(5, 8, train, route='fused', adapt_steps=-1)
    with pytest.raises(ValueError, match='target_accept=1.0'):
        s.run(5, 8, train, route='fused', adapt_steps=3, target_accept=1.0)
    for fn in (s.run.__func__, s._mcmc_sample_device.__func__):
        par = inspect.signature(fn).parameters
        assert par['adapt_steps'].default == 0 and par['target_accept'].default == 0.234
    # SMCSampler: attributes, not arguments; the host loop names the fused route
    assert SMCSampler.adapt_fraction == 0.0 and SMCSampler.target_accept == 0.234
    assert 'adapt_fraction' not in inspect.signature(SMCSampler.run).parameters

    class _Prior(object):
        def sample(self, n):
            return np.zeros((n, D))

    for net in (_StubFlow(D, adapt=False), _StubFlow(D)):
        smc = _bare_sampler(D, net, cls=SMCSampler)
        smc.sample_prior = _Prior().sample
        smc._next_seed = lambda: 1
        net.refuse = words
        smc.adapt_fraction = 0.5
        with pytest.raises(ValueError, match='adapt_fraction=0.5 needs the fused route'):
            smc.run(num_particles=8, mcmc_steps=2)
        with pytest.raises(ValueError, match='adapt_fraction=0.5 needs the fused route'):
            smc.run(num_particles=8, mcmc_steps=2, route='host')
        with pytest.raises(ValueError, match='the fused route does not take'):
            smc.run(num_particles=8, mcmc_steps=2, route='fused')
        for bad in (-0.1, 1.5):
            smc.adapt_fraction = bad
            with pytest.raises(ValueError, match='adapt_fraction='):
                smc.run(num_particles=8, mcmc_steps=2)
        smc.adapt_fraction, smc.target_accept = 0.5, 0.0
        with pytest.raises(ValueError, match='target_accept='):
            smc.run(num_particles=8, mcmc_steps=2)


def test_smc_hands_the_population_step_from_stage_to_stage(monkeypatch, caplog):
    """the stages of a fused run on a stub flow, with the device's reweighting, resampling and training stood in for: every particle
    enters a stage at the step the stage before left -- exp(mean(log step_i)) of its ends --, stage 0 at step_size"""
    import torch
    from nnest_amd import flow
    from nnest_amd.smc import SMCSampler
    D, N, S = 3, 8, 9
    ladder = iter([0.25, 0.5, 1.0])
    monkeypatch.setattr(flow, 'smc_reweight', lambda logl, beta, frac: (torch.tensor([next(ladder), 0.1, N / 2.0, 0.0], dtype=torch.float64), None))
    monkeypatch.setattr(flow, 'smc_resample', lambda m, theta, logl, seed, stage: (None, theta, logl))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda dev=None: None)

    def sampler(net):
        smc = _bare_sampler(D, net, cls=SMCSampler)
        smc.sample_prior = lambda n: np.zeros((n, D))
        smc._next_seed = lambda: 1
        smc._smc_start_fused = lambda n, target: (torch.zeros(n, D), torch.zeros(n, dtype=torch.float64), None)
        smc._smc_train = lambda theta, jitter: (theta, np.zeros(D), np.ones(D))
        smc._install_transform = lambda mean, std: None
        return smc

    net = _StubFlow(D)
    smc = sampler(net)
    smc.adapt_fraction, smc.target_accept = 0.5, 0.3
    with caplog.at_level(logging.INFO, logger='test_mcmc_adapt_check'):
        smc.run(num_particles=N, mcmc_steps=S, step_size=0.5)
    assert smc.smc_route == 'fused' and smc.betas == [0.25, 0.5, 1.0] and net.asked == [3]
    A = 5   # ceil(0.5 * 9)
    assert [c[:4] for c in net.calls] == [(S, 0, A, None)] * 3 and [c[5] for c in net.calls] == [0.3] * 3
    assert [c[6] for c in net.calls] == [0.25, 0.5, 1.0]
    gm = lambda s0: float(torch.exp(torch.log(float(np.float32(s0)) * 2.0 * torch.linspace(1.0, 1.5, N, dtype=torch.float64)).mean()).item())
    want = [gm(0.5)]
    want.append(gm(want[0]))
    want.append(gm(want[1]))
    assert [c[4] for c in net.calls] == [0.5, want[0], want[1]]   # (each stage enters at the step the one before left)
    assert smc.step_sizes == want and len(smc.step_sizes) == len(smc.betas) and want[0] != want[-1]
    assert len([r for r in caplog.records if 'population step' in r.getMessage()]) == 3
    # 0.0: the run as it was -- no new keyword reaches the flow, nothing is asked, no step is booked
    ladder = iter([0.5, 1.0])
    net2 = _StubFlow(D)
    smc2 = sampler(net2)
    smc2.run(num_particles=N, mcmc_steps=S, step_size=0.5)
    assert [c[:6] for c in net2.calls] == [(S, 0, None, None, 0.5, None)] * 2 and net2.asked == [] and smc2.step_sizes == []
