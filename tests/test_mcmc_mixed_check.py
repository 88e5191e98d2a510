"""CPU checks of the mixed walk (include/nnest_hip.h nnest_mcmc_mixed_steps; tests/mcmc_mixed_check.py restates it): the schedule; the
global rule leaves an exactly sampled target invariant and forgets a point start (tests/slice_invariance.py's statistics); the
library exports the entries and their argument checks answer without a device; the bindings and the front ends ask for the step
only where it exists."""
import ctypes
import inspect
import logging
import os
import re

import numpy as np
import pytest

from tests import mcmc_mixed_check as mc
from tests.mcmc_walk_check import numpy_draws
from tests.slice_invariance import assert_invariant, min_corrected_p, stationarity_pvalues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_mcmc_mixed_steps', 'nnest_spline_mcmc_mixed_steps', 'nnest_mcmc_mixed_check', 'nnest_spline_mcmc_mixed_check')


# ---- the schedule -----------------------------------------------------------------------------------------------------------
def test_schedule():
    assert not any(mc.kind(t, 0) for t in range(50))
    assert all(mc.kind(t, 1) for t in range(50))
    assert [t for t in range(12) if mc.kind(t, 2)] == [1, 3, 5, 7, 9, 11]
    assert [t for t in range(12) if mc.kind(t, 3)] == [2, 5, 8, 11]
    assert [t for t in range(40) if mc.kind(t, 10)] == [9, 19, 29, 39]


@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_schedule_across_a_cut(k):
    """a launch that starts at a step0 that is no multiple of k takes the kinds of the one run: mixed_run by global index, and the
    phase counter the kernels keep (t % k, advanced by one per step) against the definition"""
    N, D, S, step0 = 6, 2, 11, 7
    lp_fn = lambda q: -0.5 * np.sum(np.asarray(q, np.float64) ** 2, axis=1) * 3.0
    rng = np.random.RandomState(k)
    draws = numpy_draws(rng, N, D, step0 + S)
    z0 = rng.standard_normal((N, D)).astype(np.float32)
    one = mc.mixed_run(z0, lp_fn(z0), draws, 0.5, lp_fn, k)
    a = mc.mixed_run(z0, lp_fn(z0), draws[:step0], 0.5, lp_fn, k)
    b = mc.mixed_run(a[0], a[1], draws[step0:], 0.5, lp_fn, k, step0=step0)
    assert np.array_equal(np.concatenate([a[2], b[2]], 1), one[2]) and np.array_equal(b[0], one[0])
    assert np.array_equal(a[4] + b[4], one[4]) and np.array_equal(a[5] + b[5], one[5]) and a[6] + b[6] == one[6]
    assert one[6] == ((step0 + S) // k if k else 0)
    # the kernels' phase counter (mcmc_mixed.h MixedPhase)
    ph = step0 % k if k else 0
    for t in range(step0, step0 + S):
        g = bool(k) and ph + 1 == k
        ph = 0 if g else ph + 1
        assert g == mc.kind(t, k), (t, k)
    if k == 0:   # every step local: rw_run's run
        from tests.mcmc_walk_check import rw_run
        r = mc.mixed_run(z0, lp_fn(z0), draws, 0.5, lp_fn, 0)
        w = rw_run(z0, lp_fn(z0), draws, 0.5, lp_fn)
        assert np.array_equal(r[2], w[2]) and np.array_equal(r[4], w[4]) and not r[5].any()


# ---- the global rule on an exactly sampled 2-D target: N(0, SIG^2 [[1, c], [c, 1]]) in the box [-1, 1]^2, identity flow ------------
SIG, C2 = 0.6, 0.5
PREC = np.linalg.inv(SIG * SIG * np.array([[1.0, C2], [C2, 1.0]]))


def lp_2d(q):
    q = np.asarray(q, np.float64)
    inside = np.all(np.abs(q) <= 1.0, axis=1)
    return np.where(inside, -0.5 * np.einsum('ni,ij,nj->n', q, PREC, q), -np.inf)


def exact_2d(rng, n):
    out, have = [], 0
    L = np.linalg.cholesky(np.linalg.inv(PREC))
    while have < n:
        x = rng.standard_normal((4 * n, 2)) @ L.T
        x = x[np.all(np.abs(x) <= 1.0, axis=1)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


def test_global_rule_leaves_the_target_invariant():
    N, S = 4000, 6
    rng = np.random.RandomState(11)
    z0 = exact_2d(rng, N).astype(np.float32)
    for k in (1, 2):
        z, _, _, _, n_acc, n_glob, n_g = mc.mixed_run(z0, lp_2d(z0), numpy_draws(rng, N, 2, S), 0.4, lp_2d, k)
        assert n_g == S // k and 0.1 < n_glob.sum() / float(N * n_g) < 0.9
        assert np.all(np.abs(z) <= 1.0)
        assert_invariant(stationarity_pvalues(z, exact_2d(rng, N)), what='mixed walk in numpy, k=%d' % k)


def test_global_rule_forgets_a_point_start_and_local_steps_do_not():
    """every walker starts from one point in a corner of the box.  k = 1: after S = 40 global steps (measured: every walker has moved,
    global acceptance 0.34) the sample passes against exact draws.  The same start after 40 local steps of size 0.02 is rejected: the
    statistic has power."""
    N, S = 4000, 40
    rng = np.random.RandomState(12)
    z0 = np.tile(np.array([[0.9, 0.85]], np.float32), (N, 1))
    draws = numpy_draws(rng, N, 2, S)
    z, _, _, _, n_acc, n_glob, n_g = mc.mixed_run(z0, lp_2d(z0), draws, 0.02, lp_2d, 1)
    print('global acceptance %.3f, moved %d of %d' % (n_glob.sum() / float(N * n_g), int((n_acc > 0).sum()), N))
    assert n_g == S and np.all(n_acc > 0)
    fresh = exact_2d(rng, N)
    assert_invariant(stationarity_pvalues(z, fresh), what='mixed walk in numpy from a point, k=1')
    zl = mc.mixed_run(z0, lp_2d(z0), draws, 0.02, lp_2d, 0)[0]
    assert min_corrected_p(stationarity_pvalues(zl, fresh)) < 1e-6


def test_global_step_refuses_from_outside_to_outside():
    z0 = np.array([[2.0, 0.0], [0.1, 0.1]], np.float32)
    eps = np.array([[3.0, 0.0], [0.2, 0.0]], np.float32)
    rec = {}
    z, lp = mc.global_step(z0, lp_2d(z0), eps, np.array([0.0, 0.0], np.float32), lp_2d, record=rec)
    assert np.isnan(rec['margin'][0]) and not rec['accept'][0] and rec['accept'][1]   # (u = 0: log u = -inf, anything finite moves)
    assert np.array_equal(z[0], z0[0]) and np.array_equal(z[1], eps[1])


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
    assert _lib.SIGNATURES['nnest_spline_mcmc_mixed_steps'] == _lib.SIGNATURES['nnest_mcmc_mixed_steps']   # one argument list
    # the tempered entry's arguments plus (int global_every, int *n_accept_global_dev) before the stream
    t = _lib.SIGNATURES['nnest_mcmc_tempered_steps']
    assert _lib.SIGNATURES['nnest_mcmc_mixed_steps'] == t[:-1] + [ctypes.c_int, ctypes.c_void_p] + t[-1:]
    assert lib.nnest_hip_version() == 15


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)
    for fn in (lib.nnest_mcmc_mixed_steps, lib.nnest_spline_mcmc_mixed_steps):
        def steps(h=None, like=L, lo=None, hi=None, z_in=p, z_out=p, x_out=p, lp_out=p, C=8, S=2, step=0.3, beta=1.0, k=2, n_glob=p):
            return fn(h, like, p, p, lo, hi, z_in, None, None, z_out, x_out, lp_out, p, None, None, None, p, C, S, ctypes.c_float(step),
                      0, 0, 0, ctypes.c_double(beta), k, n_glob, None)

        assert steps() == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()
        assert steps(n_glob=None) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (optional)
        assert steps(k=0) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()           # (valid: every step local)
        assert steps(k=-1) == E_ARG and b'global_every=-1' in lib.nnest_hip_last_error()
        for bad in (-0.5, float('nan'), float('inf')):
            assert steps(beta=bad) == E_ARG and b"the likelihood's power" in lib.nnest_hip_last_error()
        assert steps(beta=0.0) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()       # (valid: the prior alone)
        assert steps(like=None) == E_ARG and b'NULL' in lib.nnest_hip_last_error()
        assert steps(C=0) == E_ARG and b'C=0' in lib.nnest_hip_last_error()
        assert steps(S=-1) == E_ARG and b'steps=-1' in lib.nnest_hip_last_error()
        assert steps(step=float('nan')) == E_ARG and b'step_size' in lib.nnest_hip_last_error()
        assert steps(z_out=None) == E_ARG and b'NULL device buffer' in lib.nnest_hip_last_error()
        assert steps(z_out=None, S=0) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (steps = 0 writes no z)
        assert steps(lo=p) == E_ARG and b'both or neither' in lib.nnest_hip_last_error()
        bad_like = _lib.like_spec(99, 1.0)
        assert steps(like=ctypes.byref(bad_like)) == E_ARG and b'likelihood id' in lib.nnest_hip_last_error()
    for fn in (lib.nnest_mcmc_mixed_check, lib.nnest_spline_mcmc_mixed_check):
        assert fn(None, 3) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()
    # the refusal of a non-Gaussian base is worded as the importance check words it
    for unit in ('nnest_abi.hip', 'nnest_spline.hip'):
        text = open(os.path.join(ROOT, 'nnest_amd', 'csrc', unit)).read()
        assert '"mcmc mixed: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only"' in text
        assert '"importance: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only"' in text


def bound(cls, family, **named):
    """an instance of the flow class with its C symbols bound as its constructor binds them, without a handle (no GPU)"""
    from nnest_amd import _lib
    o = object.__new__(cls)
    o._lib = _lib.load()
    o._h = None
    o._bind(family, **named)
    return o


def test_one_body_bound_per_family():
    from nnest_amd import _lib
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.flow import _HipFlow, HipNVP
    from nnest_amd.maf import HipMAF
    from nnest_amd.spline import HipSpline
    lib = _lib.load()
    for cls in (HipNVP, HipSpline):
        assert 'mcmc_steps' not in cls.__dict__ and cls.mcmc_steps is _HipFlow.mcmc_steps   # one body
        assert cls.mcmc_mixed_refusal is _HipFlow.mcmc_mixed_refusal
    assert "mcmc_mixed='nnest_mcmc_mixed_steps'" in inspect.getsource(HipNVP.__init__)
    assert "mcmc_mixed_check='nnest_mcmc_mixed_check'" in inspect.getsource(HipNVP.__init__)
    assert "mcmc_mixed='nnest_spline_mcmc_mixed_steps'" in inspect.getsource(HipSpline.__init__)
    assert "mcmc_mixed_check='nnest_spline_mcmc_mixed_check'" in inspect.getsource(HipSpline.__init__)
    assert bound(HipSpline, 'nnest_spline', mcmc_mixed='nnest_spline_mcmc_mixed_steps')._sym['mcmc_mixed'] is lib.nnest_spline_mcmc_mixed_steps
    assert bound(HipNVP, 'nnest_nvp', mcmc_mixed='nnest_mcmc_mixed_steps')._sym['mcmc_mixed'] is lib.nnest_mcmc_mixed_steps
    par = inspect.signature(_HipFlow.mcmc_steps).parameters
    assert par['global_every'].default == 0
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        assert 'mcmc_mixed' not in inspect.getsource(cls.__init__)
        o = bound(cls, family)
        o.device = 'cpu'
        with pytest.raises(NotImplementedError):
            o.mcmc_steps(3, None, 2, 0.1, global_every=2)
        with pytest.raises(NotImplementedError):
            o.mcmc_mixed_refusal(3)
    o = bound(HipNVP, 'nnest_nvp', mcmc='nnest_mcmc_steps', mcmc_mixed='nnest_mcmc_mixed_steps')
    with pytest.raises(ValueError, match='global_every=-1'):
        o.mcmc_steps(3, None, 2, 0.1, global_every=-1)


# ---- the front ends on stub flows ------------------------------------------------------------------------------------------------
class _StubFlow(object):
    """what the front ends ask of the flow, recorded"""
    device = 'cpu'

    def __init__(self, D, mixed=True):
        self._sym = {'mcmc': object(), 'mcmc_tempered': object()}
        if mixed:
            self._sym['mcmc_mixed'] = object()
        self.D, self.calls, self.refuse, self.asked = D, [], None, []

    def mcmc_mixed_refusal(self, like_id):
        self.asked.append(like_id)
        return self.refuse

    def forward(self, x):
        import torch
        return torch.as_tensor(np.asarray(x, np.float32)), None

    def mcmc_steps(self, like_id, z, steps, step_size, **kw):
        import torch
        C = z.shape[0]
        self.calls.append((steps, kw.get('step0', 0), kw.get('global_every')))
        k = kw.get('global_every', 0)
        out = dict(z=z, x=z, lp=torch.zeros(C, dtype=torch.float64), logl=torch.zeros(C, dtype=torch.float64),
                   hist_z=torch.zeros(C, steps, self.D), hist_x=torch.zeros(C, steps, self.D),
                   hist_logl=torch.zeros(C, steps, dtype=torch.float64), n_accept=torch.full((C,), steps, dtype=torch.int32))
        if k:
            s0 = kw.get('step0', 0)
            out['n_accept_global'] = torch.full((C,), sum(mc.kind(t, k) for t in range(s0, s0 + steps)), dtype=torch.int32)
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
    s.logger = logging.getLogger('test_mcmc_mixed_check')
    return s


def test_front_end_books_and_logs_the_global_steps(caplog):
    D, N, S = 3, 8, 23
    net = _StubFlow(D)
    s = _bare_sampler(D, net)
    init = np.zeros((N, D), np.float32)
    with caplog.at_level(logging.INFO, logger='test_mcmc_mixed_check'):
        out = s._mcmc_sample_device(S, init_samples=init, seed=1, chunk_steps=7, global_every=5)
    assert out[0].shape == (N, S + 1, D)
    assert net.calls == [(0, 0, None), (7, 0, 5), (7, 7, 5), (7, 14, 5), (2, 21, 5)] and net.asked == [3]
    assert s.global_proposed == N * (S // 5) and s.global_accepted == N * (S // 5)
    assert s.total_accepted == N * S and s.total_rejected == 0
    assert [r for r in caplog.records if 'global acceptance' in r.getMessage()]
    # 0: the call as it was -- no new keyword reaches the flow, nothing is asked of the library, nothing is left behind
    net2 = _StubFlow(D)
    s2 = _bare_sampler(D, net2)
    s2._mcmc_sample_device(S, init_samples=init, seed=1, chunk_steps=12)
    assert net2.calls == [(0, 0, None), (12, 0, None), (11, 12, None)] and net2.asked == [] and not hasattr(s2, 'global_proposed')
    with pytest.raises(ValueError, match='global_every=-1'):
        s2._mcmc_sample_device(S, init_samples=init, global_every=-1)


def test_front_ends_name_what_the_global_step_does_not_take():
    from nnest_amd.smc import SMCSampler
    D = 3
    train = np.random.RandomState(0).normal(size=(40, D))
    # the library's words on the base, asked before any launch, are the reason
    words = 'mcmc mixed: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only'
    net = _StubFlow(D)
    net.refuse = words
    s = _bare_sampler(D, net)
    with pytest.raises(ValueError, match=r'the fused route does not take the flow _StubFlow: mcmc mixed: GeneralisedNormal base'):
        s.run(5, 8, train, route='fused', global_every=5)
    assert net.calls == []
    # a family without the kernel
    s = _bare_sampler(D, _StubFlow(D, mixed=False))
    with pytest.raises(ValueError, match='no fused mixed'):
        s.run(5, 8, train, route='fused', global_every=5)
    # the host step loop has no global step; a negative schedule is no schedule
    s = _bare_sampler(D, _StubFlow(D))
    for route in (None, 'host'):
        with pytest.raises(ValueError, match="needs route='fused'"):
            s.run(5, 8, train, route=route, global_every=5)
    with pytest.raises(ValueError, match='global_every=-1'):
        s.run(5, 8, train, route='fused', global_every=-1)
    # SMCSampler: the host loop names the fused route
    class _Prior(object):
        def sample(self, n):
            return np.zeros((n, D))

    for net, word in ((_StubFlow(D, mixed=False), 'fused route'), (_StubFlow(D), 'fused route')):
        smc = _bare_sampler(D, net, cls=SMCSampler)
        smc.sample_prior = _Prior().sample
        smc._next_seed = lambda: 1
        if 'mcmc_mixed' in net._sym:
            net.refuse = words
        smc.global_every = 2   # (an attribute: tests/test_smc_check.py pins run's argument list)
        with pytest.raises(ValueError, match=word):
            smc.run(num_particles=8, mcmc_steps=2)
        with pytest.raises(ValueError, match=word):
            smc.run(num_particles=8, mcmc_steps=2, route='host')
        smc.global_every = -1
        with pytest.raises(ValueError, match='global_every=-1'):
            smc.run(num_particles=8, mcmc_steps=2)
    assert SMCSampler.global_every == 0
    for fn in (s.run.__func__, s._mcmc_sample_device.__func__):
        assert inspect.signature(fn).parameters['global_every'].default == 0
