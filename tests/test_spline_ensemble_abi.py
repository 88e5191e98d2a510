"""CPU checks of the spline flow's fused stretch-move kernel at the C-ABI and Python boundaries (no compute calls without a GPU): the
header declares and the library exports nnest_spline_ensemble_steps / nnest_spline_ensemble_max_walkers, their argument checks answer
without a device, HipSpline binds the entry and the families without one do not, and the front end routes to it on route='fused'
only."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_spline_ensemble_steps', 'nnest_spline_ensemble_max_walkers')


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
    assert _lib.SIGNATURES['nnest_spline_ensemble_steps'] == _lib.SIGNATURES['nnest_ensemble_steps']   # one argument list
    assert lib.nnest_hip_version() == 15
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    assert 'TWO-PUBLISH RULE' in text


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    assert lib.nnest_spline_ensemble_max_walkers(None, 3) == -1
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)

    def steps(h=None, like=L, t_std=p, t_mean=p, lo=None, hi=None, z_in=p, z_out=ctypes.c_void_p(128), x_out=p, lp_out=p, hist_z=p,
              hist_x=p, hist_lp=p, work=p, C=8, S=2):
        return lib.nnest_spline_ensemble_steps(h, like, t_std, t_mean, lo, hi, z_in, None, z_out, x_out, lp_out, hist_z, hist_x, hist_lp,
                                               None, work, C, S, 0, 0, 0, 0.0, None)

    assert steps() == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()
    assert steps(like=None) == E_ARG and b'NULL' in lib.nnest_hip_last_error()
    for name in ('t_std', 't_mean', 'z_in', 'z_out', 'x_out', 'lp_out', 'hist_z', 'hist_x', 'hist_lp', 'work'):
        assert steps(**{name: None}) == E_ARG, name
        assert b'NULL device buffer' in lib.nnest_hip_last_error(), name
    assert steps(lo=p) == E_ARG and b'both or neither' in lib.nnest_hip_last_error()
    assert steps(z_out=p) == E_ARG and b'z_in_dev' in lib.nnest_hip_last_error()
    assert steps(S=-1) == E_ARG and b'steps=-1' in lib.nnest_hip_last_error()
    assert steps(C=0) == E_ARG and b'C=0' in lib.nnest_hip_last_error()
    assert steps(C=1) == E_ARG
    bad = _lib.like_spec(99, 1.0)
    assert steps(like=ctypes.byref(bad)) == E_ARG and b'likelihood id' in lib.nnest_hip_last_error()


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
    from nnest_amd.fastslow import HipFastSlowNVP
    from nnest_amd.flow import _HipFlow, HipNVP
    from nnest_amd.maf import HipMAF
    from nnest_amd.spline import HipSpline
    lib = _lib.load()
    for cls in (HipNVP, HipSpline):
        assert 'ensemble_steps' not in cls.__dict__ and 'ensemble_max_walkers' not in cls.__dict__
        assert cls.ensemble_steps is _HipFlow.ensemble_steps and cls.ensemble_max_walkers is _HipFlow.ensemble_max_walkers   # one body
    assert "ensemble='nnest_spline_ensemble_steps'" in inspect.getsource(HipSpline.__init__)
    assert "ensemble='nnest_ensemble_steps'" in inspect.getsource(HipNVP.__init__)
    sp = bound(HipSpline, 'nnest_spline', ensemble='nnest_spline_ensemble_steps', ensemble_max_walkers='nnest_spline_ensemble_max_walkers')
    assert sp._sym['ensemble'] is lib.nnest_spline_ensemble_steps and sp._sym['ensemble'] is not lib.nnest_ensemble_steps
    assert sp._sym['ensemble_max_walkers'] is lib.nnest_spline_ensemble_max_walkers
    # the default route: the NVP alone
    assert HipNVP.ensemble_fused_by_default is True
    for cls in (HipSpline, HipMAF, HipCholesky, _HipFlow):
        assert cls.ensemble_fused_by_default is False, cls
    assert not getattr(HipFastSlowNVP, 'ensemble_fused_by_default', False)
    # a family that binds no `ensemble` symbol cannot reach another family's entry point
    assert 'ensemble' not in inspect.getsource(HipCholesky.__init__)
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        o = bound(cls, family)
        o.device = 'cpu'
        assert 'ensemble' not in o._sym and 'ensemble_max_walkers' not in o._sym
        with pytest.raises(NotImplementedError):
            o.ensemble_steps(3, None, 2)


class _StubSpline(object):
    """what _ensemble_sample asks of the flow, recorded: a family with the `ensemble` entry whose default route is 'rounds'"""
    ensemble_fused_by_default = False
    device = 'cpu'

    def __init__(self, D, cap=1 << 12):
        self._sym = {'ensemble': object(), 'ensemble_max_walkers': object()}
        self.D, self.cap, self.calls = D, cap, []

    def prior_sample(self, n):
        import torch
        return torch.zeros(n, self.D)

    def ensemble_max_walkers(self, like_id):
        return self.cap

    def ensemble_steps(self, like_id, z, steps, **kw):
        import torch
        C = z.shape[0]
        self.calls.append((like_id, C, steps, kw['step0']))
        return dict(z=z, x=z, lp=torch.zeros(C, dtype=torch.float64), hist_z=torch.zeros(C, steps, self.D),
                    hist_x=torch.zeros(C, steps, self.D), hist_lp=torch.zeros(C, steps, dtype=torch.float64),
                    n_accept=torch.ones(C, dtype=torch.int32))


class _StubTrainer(object):
    def __init__(self, net):
        self.netG = net


def _bare_sampler(D, net, monkeypatch, agrees=True):
    from nnest_amd import ensemble_rounds
    from nnest_amd.ensemble import EnsembleSampler

    class _Like(object):
        hip_like_id, hip_like_params = 3, (0.5,)

    s = EnsembleSampler.__new__(EnsembleSampler)
    s.x_dim, s.num_derived, s.trainer = D, 0, _StubTrainer(net)
    s.total_calls = s.total_accepted = s.total_rejected = 0
    s._ensemble_affine = lambda: (np.ones(D), np.zeros(D))
    s._user_loglike, s._user_prior, s._transform_prior = _Like(), None, True
    s._probe_agrees = lambda like_id, params, **kw: agrees   # (the one step of _device_target that needs a device)
    rounds = []

    def fake_rounds(flow, z, steps, state=None, **kw):
        import torch
        C = z.shape[0]
        rounds.append((C, steps))
        st = ensemble_rounds.EnsembleState(z, z, torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.int32))
        return st, dict(hist_z=torch.zeros(C, steps, D), hist_x=torch.zeros(C, steps, D),
                        hist_lp=torch.zeros(C, steps, dtype=torch.float64), hist_derived=np.zeros((C, steps, 0)))

    monkeypatch.setattr(ensemble_rounds, 'ensemble_rounds', fake_rounds)
    return s, rounds


def test_the_spline_takes_the_fused_route_only_when_asked(monkeypatch):
    D, N, S = 3, 16, 5
    net = _StubSpline(D)
    s, rounds = _bare_sampler(D, net, monkeypatch)
    out = s._ensemble_sample(S, N, seed=1)
    assert s.ensemble_route == 'rounds' and rounds == [(N, S)] and net.calls == [] and out[0].shape == (N, S, D)
    out = s._ensemble_sample(S, N, seed=1, route='fused', chunk_steps=2)
    assert s.ensemble_route == 'fused' and net.calls == [(3, N, 2, 0), (3, N, 2, 2), (3, N, 1, 4)] and len(rounds) == 1
    assert out[0].shape == (N, S, D) and s.total_accepted == N * 3
    # where the fused kernel does not take the run, route='fused' is refused: the population, the likelihood, the family
    net.cap = N - 1
    with pytest.raises(ValueError, match='fused route'):
        s._ensemble_sample(S, N, seed=1, route='fused')
    net.cap = 1 << 12
    s2, _ = _bare_sampler(D, net, monkeypatch, agrees=False)
    s2.loglike, s2._user_prior = None, None
    with pytest.raises(ValueError, match='fused route'):
        s2._ensemble_sample(S, N, seed=1, route='fused')
    del net._sym['ensemble']
    with pytest.raises(ValueError, match='fused route'):
        s._ensemble_sample(S, N, seed=1, route='fused')
    # a family whose default is the fused route (the NVP) keeps it at route=None
    nvp = _StubSpline(D)
    nvp.ensemble_fused_by_default = True
    s3, rounds3 = _bare_sampler(D, nvp, monkeypatch)
    s3._ensemble_sample(S, N, seed=1)
    assert s3.ensemble_route == 'fused' and rounds3 == []


def test_run_and_bootstrap_take_route():
    from nnest_amd.ensemble import EnsembleSampler
    for fn in (EnsembleSampler.run, EnsembleSampler.bootstrap):
        par = inspect.signature(fn).parameters
        assert 'route' in par and par['route'].default is None, fn.__name__
        assert 'route=route' in inspect.getsource(fn)
    # the bootstrap's x-space run keeps its own choice
    src = inspect.getsource(EnsembleSampler.bootstrap)
    call = src[src.index('self._ensemble_sample_x('):]
    assert 'route' not in call[:call.index(')')]
