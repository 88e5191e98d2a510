"""GPU: MCMCSampler and EnsembleSampler with chain_stats=True log the reference's chain-statistics lines (sampler.py:451-452,
:712-713; mcmc.py:119-120, ensemble.py:224-225) at the reference's steps, in its format, with the values of the float64
restatement (tests/chain_stats_check.py) on the returned samples; with the default nothing is logged and nothing changes."""
import logging
import re

import numpy as np
import pytest
import torch

import nnest_amd
from tests import chain_stats_check as chk

pytestmark = pytest.mark.gpu

LINE = re.compile(r'^(?:Step \[(\d+)\] acceptance|Acceptance) \[([0-9.]+)\] min ESS \[([0-9.]+)\] max ESS \[([0-9.]+)\] '
                  r'average jump \[([0-9.]+)\]$')


class _Capture(logging.Handler):
    def __init__(self):
        super(_Capture, self).__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _stats_lines(handler):
    return [m for m in (LINE.match(l) for l in handler.lines) if m]


def _expected(samples, T):
    x = np.asarray(samples[:, :T], np.float64)
    mu, sd = chk.moments(x)
    ess, _ = chk.ess_from_p(chk.autocorr(x, mu, sd, lags=range(1, T)), T)
    return chk.acceptance(x), ess, chk.jump(x)


def _check_line(m, samples, T, step):
    assert (m.group(1) is None) == (step is None) and (step is None or int(m.group(1)) == step)
    acc, ess, jump = _expected(samples, T)
    text = '[%5.4f] min ESS [%5.4f] max ESS [%5.4f] average jump [%5.4f]' % (acc, np.min(ess), np.max(ess), jump)
    got = '[%s] min ESS [%s] max ESS [%s] average jump [%s]' % m.group(2, 3, 4, 5)
    if got != text:   # a last-digit difference is a rounding tie of float32 against float64 arithmetic, nothing more
        vals = [float(v) for v in m.group(2, 3, 4, 5)]
        np.testing.assert_allclose(vals, [acc, np.min(ess), np.max(ess), jump], rtol=1e-4, atol=1.01e-4)


def _gauss_training(D, n=2000, seed=0):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((n, D)) * np.linspace(0.5, 2.0, D) + np.arange(D)


def _loglike(D):
    sc = np.linspace(0.5, 2.0, D)

    def loglike(x):
        return -0.5 * np.sum(((np.atleast_2d(x) - np.arange(D)) / sc) ** 2, axis=1)
    return loglike


def test_mcmc_sampler_logs_chain_stats(tmp_path):
    D, C, S, every = 3, 20, 60, 25
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(D, _loglike(D), log_dir=str(tmp_path), flow='nvp', chain_stats=True)
    h = _Capture()
    s.logger.addHandler(h)
    try:
        s.run(S, C, _gauss_training(D), stats_interval=every)
    finally:
        s.logger.removeHandler(h)
    x = s.samples[:, :, :D]
    found = _stats_lines(h)
    steps = [every * k for k in range(1, S // every + 1)]
    assert len(found) == len(steps) + 1
    for m, it in zip(found, steps):
        _check_line(m, x, it + 1, it)                    # sampler.py:451-452: it + 1 states at step it
    _check_line(found[-1], x, S + 1, None)              # mcmc.py:119-120


def test_ensemble_sampler_logs_chain_stats(tmp_path):
    D, N, S, every = 3, 16, 30, 10
    np.random.seed(2)
    torch.manual_seed(2)
    s = nnest_amd.EnsembleSampler(D, _loglike(D), log_dir=str(tmp_path), flow='nvp', chain_stats=True)
    h = _Capture()
    s.logger.addHandler(h)
    try:
        s.run(S, N, _gauss_training(D), stats_interval=every)
    finally:
        s.logger.removeHandler(h)
    x = s.samples[:, :, :D]
    found = _stats_lines(h)
    steps = [it for it in range(every, S + 1, every) if it > 1]
    assert len(found) == len(steps) + 1
    for m, it in zip(found, steps):
        _check_line(m, x, it, it)                        # sampler.py:712-713: `it` states at step it
    _check_line(found[-1], x, S, None)                   # ensemble.py:224-225


def test_default_logs_no_chain_stats(tmp_path):
    D = 3
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(D, _loglike(D), log_dir=str(tmp_path), flow='nvp')
    assert s.chain_stats is False
    h = _Capture()
    s.logger.addHandler(h)
    try:
        s.run(30, 10, _gauss_training(D), stats_interval=10)
    finally:
        s.logger.removeHandler(h)
    assert not _stats_lines(h)


def test_sampler_chain_stats_method(tmp_path):
    s = nnest_amd.MCMCSampler(3, _loglike(3), log_dir=str(tmp_path), flow='nvp', chain_stats=True)
    rng = np.random.RandomState(4)
    x = rng.standard_normal((8, 40, 3)).astype(np.float32)
    x[:, 5] = x[:, 4]
    h = _Capture()
    s.logger.addHandler(h)
    try:
        acc, ess, jump = s._chain_stats(x, step=7)
        acc2, ess2, jump2 = s._chain_stats(x, mean=np.zeros(3), std=np.ones(3))
    finally:
        s.logger.removeHandler(h)
    found = _stats_lines(h)
    assert len(found) == 2
    _check_line(found[0], x, 40, 7)
    assert acc == chk.acceptance(x.astype(np.float64)) and acc2 == acc
    np.testing.assert_allclose(jump, chk.jump(x.astype(np.float64)), rtol=1e-5)
    x64 = x.astype(np.float64)
    e0, _ = chk.ess_from_p(chk.autocorr(x64, np.zeros(3), np.ones(3)), 40)
    np.testing.assert_allclose(ess2, e0, rtol=1e-5)
