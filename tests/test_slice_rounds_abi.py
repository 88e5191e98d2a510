"""CPU checks of the round-driven slice proposal (include/nnest_hip.h nnest_slice_rounds_*; nnest_amd/slice_rounds.py) at the C-ABI
and sampler boundaries, without compute calls: the header declares and the library exports the entry points, argument errors come back
as return codes, and the sampler's slice route no longer falls through to random-walk Metropolis -- the host route and the fused
route of a flow without a fused slice kernel both hand the batch to the round driver."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_slice_rounds_create', 'nnest_slice_rounds_destroy', 'nnest_slice_rounds_begin', 'nnest_slice_rounds_screen',
       'nnest_slice_rounds_advance', 'nnest_slice_rounds_finish')


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(nnest_[a-z0-9_]+)\s*\(', text))


def test_header_declares_and_library_exports_the_slice_round_entry_points():
    from nnest_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.nnest_hip_version() == 15


def test_slice_round_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.nnest_slice_rounds_create(0, 4, 2, ctypes.byref(h)) == 1 and not h.value
    assert lib.nnest_slice_rounds_create(8, 0, 2, ctypes.byref(h)) == 1
    assert lib.nnest_slice_rounds_create(8, 4, -1, ctypes.byref(h)) == 1
    assert lib.nnest_slice_rounds_create(8, 4, 2, None) == 1
    assert lib.nnest_slice_rounds_destroy(None) == 0
    rc = lib.nnest_slice_rounds_begin(None, None, None, None, None, 0.0, 0.5, 8, 32, None, 0, 0, None, None, None, None, None, None)
    assert rc == 1 and b'NULL' in lib.nnest_hip_last_error()
    assert lib.nnest_slice_rounds_screen(None, None, None, None, None, None, None, None) == 1
    assert lib.nnest_slice_rounds_advance(None, None, None, None, None) == 1
    assert lib.nnest_slice_rounds_finish(None, None, None, None, None, None, None, None) == 1


class _Net(object):
    """a stand-in flow on the CPU (identity map): what the sampler's slice route asks of netG before it hands over"""
    device = torch.device('cpu')

    def __init__(self, fused_slice):
        self._fused_slice = fused_slice

    def forward(self, x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
        return x.clone(), torch.zeros(x.shape[0])

    inverse = forward

    def supports_fused_slice(self, C):
        return self._fused_slice

    def slice_steps(self, *args, **kwargs):
        raise AssertionError('the fused slice kernel must not be asked for a flow without one')

    def mh_steps(self, *args, **kwargs):
        raise AssertionError('the slice proposal must not run Metropolis')


class _Trainer(object):
    def __init__(self, fused_slice=False):
        self.netG = _Net(fused_slice)


def _fake_driver(calls, nd=0):
    def slice_rounds(flow, z, logl, loglstar, width, steps, loglike=None, like_id=None, num_derived=0, init_derived=None, history=False,
                     **kw):
        C, D = z.shape
        calls.append(dict(loglike=loglike, like_id=like_id, loglstar=loglstar, width=width, steps=steps, history=history, **kw))
        rows = np.zeros((3, D), np.float32)
        if loglike is not None:
            loglike(rows)   # the driver evaluates the packed rows through the host protocol
        hx = z[:, None, :].repeat(1, steps + 1, 1)
        return dict(x=z.clone(), n_call=torch.full((C,), 3, dtype=torch.int32), n_move=torch.full((C,), steps, dtype=torch.int32),
                    moved=torch.ones(C, dtype=torch.bool), n_eval=torch.full((C,), 5, dtype=torch.int32), hist_x=hx if history else None,
                    hist_z=hx if history else None, hist_logl=logl[:, None].repeat(1, steps + 1) if history else None,
                    derived=np.zeros((C, nd)) if nd else None, hist_derived=np.zeros((C, steps + 1, nd)) if nd else None, rounds=7)
    return slice_rounds


def _sampler(tmp_path, fused_slice=False, num_derived=0):
    from nnest_amd.priors import UniformPrior
    from nnest_amd.sampler import Sampler

    def like(x):
        x = np.atleast_2d(x)
        ll = -np.sum(x ** 2, axis=1)
        return (ll, np.zeros((x.shape[0], num_derived))) if num_derived else ll

    return Sampler(2, like, prior=UniformPrior(2, -1, 1), transform_prior=False, trainer=_Trainer(fused_slice), log_dir=str(tmp_path),
                   fused=False, num_derived=num_derived, mcmc_proposal='slice', log_level=40)


def test_host_route_dispatches_to_the_round_driver(tmp_path, monkeypatch):
    from nnest_amd import slice_rounds as sr
    calls = []
    monkeypatch.setattr(sr, 'slice_rounds', _fake_driver(calls, nd=2))
    s = _sampler(tmp_path, num_derived=2)
    monkeypatch.setattr(s, '_mcmc_sample_host', lambda *a, **k: pytest.fail('slice fell back to the Metropolis host loop'))
    C, S = 6, 4
    init = np.random.RandomState(0).uniform(-0.5, 0.5, size=(C, 2))
    out = s._mcmc_sample(S, step_size=0.3, init_samples=init, init_loglikes=-np.sum(init ** 2, axis=1),
                         init_derived=np.zeros((C, 2)), loglstar=-1.0, seed=11, walker_offset=40)
    samples, latent, derived, loglikes, scale, ncall = out
    assert len(calls) == 1 and calls[0]['like_id'] is None and calls[0]['loglike'] == s.loglike
    assert calls[0]['seed'] == 11 and calls[0]['walker_offset'] == 40 and calls[0]['width'] == pytest.approx(0.6)
    assert samples.shape == (C, S + 1, 2) and latent.shape == (C, S + 1, 2) and derived.shape == (C, S + 1, 2)
    assert loglikes.shape == (C, S + 1) and scale == 0.3 and ncall == 3 * C
    assert s.total_calls == 3 and s.total_accepted == C * S and s.total_rejected == 0
    with pytest.raises(NotImplementedError):
        s._mcmc_sample(S, init_samples=init, init_loglikes=np.zeros(C), loglstar=None)


def test_fused_route_without_a_fused_slice_kernel_uses_the_device_likelihood(tmp_path, monkeypatch):
    from nnest_amd import slice_rounds as sr
    calls = []
    monkeypatch.setattr(sr, 'slice_rounds', _fake_driver(calls))
    s = _sampler(tmp_path, fused_slice=False)
    s._fused_like_id, s._linear_scale = 0, 5.0
    C, S = 5, 3
    init = np.random.RandomState(1).uniform(-0.5, 0.5, size=(C, 2))
    ends, scale, ncall = s._mcmc_endpoints_fused(S, 0.25, False, init, np.zeros(C), -1.0, 0, 123)
    assert len(calls) == 1 and calls[0]['like_id'] == 0 and calls[0]['loglike'] is None and calls[0]['seed'] == 123
    assert tuple(ends.shape) == (C, 4) and bool(torch.all(ends[:, 3] == 1)) and ncall == 3 * C
    assert s.total_calls == 3 * C and s.total_accepted == C * S
