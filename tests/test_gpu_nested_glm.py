"""NestedSampler on a regression likelihood of user data (likelihoods.GLMData) with the slice proposal: the MCMC batches run in the
fused kernels of that likelihood (nnest_slice_glm_steps, nnest_spline_slice_glm_steps; Sampler._slice_glm, slice_route 'fused-glm'),
everything else keeps the host callable.  Build-defined: the reference has neither the likelihood nor the proposal.

log Z against the grid quadrature of the 2-D logistic regression of the existing tests (tests/test_gpu_mcmc_glm.py quadrature) under
the unit box on x and x -> 5 x, i.e. the uniform prior on [-5, 5]^2.  The bound is 5 sigma with sigma = sqrt(H / N) (Skilling 2006:
the standard deviation of nested sampling's log Z with N live points), H the information of the posterior against the prior,
computed here on the same grid from the reference integral -- not from the sampler's own logzerr.  Run with  pytest -m gpu."""
import numpy as np
import pytest
import torch

from tests import glm_check as gk
from tests.test_gpu_mcmc_glm import quadrature

pytestmark = pytest.mark.gpu

N_LIVE, HALF = 200, 5.0
RUN = dict(mcmc_num_chains=50, mcmc_steps=10, train_iters=200)


def information(like, lo, hi, m=801):
    """H = int p log(p / pi) = E_p[log L] - log Z of the posterior p = L pi / Z against the uniform prior pi on [lo, hi]^2, on
    quadrature's grid (trapezoid, float64).  Returns (log Z, H)"""
    g = np.linspace(lo, hi, m)
    w1 = np.full(m, g[1] - g[0])
    w1[[0, -1]] *= 0.5
    X, Y = np.meshgrid(g, g, indexing='ij')
    th = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
    ll = np.concatenate([like.loglike_rows(th[i:i + 200000]) for i in range(0, len(th), 200000)])
    top = ll.max()
    w = np.exp(ll - top) * np.outer(w1, w1).reshape(-1)
    tot = w.sum()
    logz = float(top + np.log(tot) - 2.0 * np.log(hi - lo))
    return logz, float((w * ll).sum() / tot - logz)


_REF = {}


def reference():
    """(the likelihood's recipe, exact log Z, sigma); computed once"""
    if not _REF:
        like = gk.make_like(2, 40, 'logistic', 5)
        exact = quadrature(like, -HALF, HALF)[0] - 2.0 * np.log(2.0 * HALF)
        logz, H = information(like, -HALF, HALF)
        assert abs(logz - exact) < 1e-9 and 1.0 < H < 10.0, (logz, exact, H)
        _REF.update(exact=exact, sigma=float(np.sqrt(H / N_LIVE)), H=H)
    return _REF


def sampler(tmp_path, flow, seed, proposal='slice'):
    from nnest_amd.nested import NestedSampler
    like = gk.make_like(2, 40, 'logistic', 5)
    np.random.seed(seed)
    torch.manual_seed(seed)
    s = NestedSampler(2, like, transform=lambda x: HALF * x, log_dir=str(tmp_path), num_live_points=N_LIVE, log_level=30, flow=flow,
                      mcmc_proposal=proposal)
    return s, like


def count_calls(s):
    """(rows through the host callable, candidates the slice kernels report a likelihood for): counters filled as the run goes"""
    host, kernel = [0], [0]
    inner = s.loglike

    def loglike(x):
        out = inner(x)
        host[0] += len(out[0])
        return out
    s.loglike = loglike
    netG = s.trainer.netG
    launch = netG.slice_steps

    def slice_steps(*a, **kw):
        assert kw.get('like_glm') is not None and a[0] is None
        res = launch(*a, **kw)
        kernel[0] += int(res['n_call'].sum())
        return res
    netG.slice_steps = slice_steps
    return host, kernel


@pytest.mark.parametrize('flow', ['nvp', 'spline'])
def test_log_z_through_the_fused_route(tmp_path, flow):
    ref = reference()
    s, like = sampler(tmp_path / 'fused', flow, 1)
    assert s._slice_glm is not None and s._fused_like_id is None and s._slice_glm.like_glm['n'] == 40
    host, kernel = count_calls(s)
    s.run(**RUN)
    assert s.slice_route == 'fused-glm'
    assert kernel[0] > 0 and host[0] >= N_LIVE and s.total_calls == kernel[0] + host[0], (s.total_calls, kernel[0], host[0])
    off = abs(s.logz - ref['exact']) / ref['sigma']
    print('%s fused-glm: log Z %.4f (own error %.4f), quadrature %.4f, H %.3f, sigma %.4f: off by %.2f sigma; %d kernel + %d host calls' % (
        flow, s.logz, s.logzerr, ref['exact'], ref['H'], ref['sigma'], off, kernel[0], host[0]))
    assert off <= 5.0, (s.logz, ref)
    # the same seed with the fused route disabled: the host protocol, the parent commit's only route
    h, _ = sampler(tmp_path / 'host', flow, 1)
    h._slice_glm = None
    h.run(**RUN)
    assert h.slice_route == 'host' and np.isfinite(h.logz)
    print('%s host     : log Z %.4f (own error %.4f): off by %.2f sigma' % (flow, h.logz, h.logzerr, abs(h.logz - ref['exact']) / ref['sigma']))


def test_the_metropolis_proposal_keeps_the_host_protocol(tmp_path):
    """mcmc_proposal='mh' on a GLMData: no device target for the slice kernels, and every likelihood row of a batch goes through the
    host callable"""
    s, like = sampler(tmp_path, 'nvp', 2, proposal='mh')
    assert s._slice_glm is None and s._fused_like_id is None and s.slice_route is None
    u = np.random.RandomState(1).uniform(-0.6, 0.6, size=(32, 2))
    l = like.loglike_rows(HALF * u)
    star = float(np.quantile(l, 0.2))
    before, rows = s.total_calls, like.num_evaluations
    s._mcmc_sample(5, init_samples=u[l > star], init_loglikes=l[l > star], loglstar=star)
    assert s.total_calls > before and s.total_calls - before == like.num_evaluations - rows
    assert s.slice_route is None


def test_without_the_unit_box_under_a_linear_scale_there_is_no_device_target(tmp_path):
    """another transform (not x -> s x) keeps the slice proposal of a GLMData on the host protocol"""
    from nnest_amd.nested import NestedSampler
    like = gk.make_like(2, 40, 'logistic', 5)
    s = NestedSampler(2, like, transform=lambda x: HALF * x + 0.5, log_dir=str(tmp_path), num_live_points=N_LIVE, log_level=30, flow='nvp',
                      mcmc_proposal='slice')
    assert s._slice_glm is None
