"""GPU: the chain-statistics kernels (include/nnest_hip.h nnest_chain_stats*, nnest_amd.evaluation) against the reference's own
outputs (tests/golden/chain_stats_ref.npz) and the float64 restatement (tests/chain_stats_check.py) at every kernel shape; input
handling in place (strides, the affine on load, the lag-blocked stop), repeatability, additivity of the sums, argument errors."""
import os

import numpy as np
import pytest
import torch

from nnest_amd import _lib, evaluation
from tests import chain_stats_check as chk

pytestmark = pytest.mark.gpu
E_ARG = 1   # NNEST_E_ARG (include/nnest_hip.h)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chain_stats_ref.npz')


def chains(C, T, D, rho=0.8, reject=0.3, seed=0, scale=None):
    """AR(1) chains with repeated (rejected) steps, float32"""
    rng = np.random.RandomState(seed)
    x = np.zeros((C, T, D))
    x[:, 0] = rng.standard_normal((C, D))
    for j in range(1, T):
        x[:, j] = rho * x[:, j - 1] + np.sqrt(1 - rho ** 2) * rng.standard_normal((C, D))
        keep = rng.uniform(size=C) < reject
        x[keep, j] = x[keep, j - 1]
    if scale is not None:
        x = x * scale
    return x.astype(np.float32)


def check_against_restatement(r, x, mean=None, std=None):
    x64 = np.asarray(x, np.float64)
    C, T, D = x.shape
    assert r['acceptance'] == chk.acceptance(x64)
    np.testing.assert_allclose(r['jump_distance'], chk.jump(x64), rtol=1e-5)
    mu0, sd0 = chk.moments(x64)
    mu = mu0 if mean is None else mean
    sd = sd0 if std is None else std
    np.testing.assert_allclose(r['mean'], mu, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r['std'], sd, rtol=1e-9)
    stop = r['stop_lag']
    n = min(stop, T - 1)
    p_ref = chk.autocorr(x64, mu, sd, lags=range(1, n + 1))
    p = r['p'][:n]
    np.testing.assert_allclose(p, p_ref, rtol=1e-5, atol=1e-6 * max(1.0, np.abs(p_ref).max()))
    # ESS: the restatement's rule on the kernel's own p_s, and on the float64 p_s where no p_s lies near the threshold
    ess_own, stop_own = chk.ess_from_p(r['p'], T)
    assert stop_own == stop
    np.testing.assert_allclose(r['ess'], ess_own, rtol=1e-12)
    if np.min(np.abs(p_ref - 0.05)) > 1e-5:
        ess_ref, stop_ref = chk.ess_from_p(np.vstack([p_ref, np.zeros((max(T - 1 - n, 0), D))]), T)
        assert stop_ref == stop
        np.testing.assert_allclose(r['ess'], ess_ref, rtol=1e-5)
    if C > 1:
        np.testing.assert_allclose(r['rhat'], chk.rhat(x64), rtol=1e-5)
    else:
        assert r['rhat'] is None


@pytest.mark.parametrize('name', [str(c) for c in np.load(GOLD)['cases']])
def test_golden_cases(name):
    g = np.load(GOLD)
    x = g[name + '_x']
    mean = g[name + '_mean'] if name + '_mean' in g else None
    std = g[name + '_std'] if name + '_std' in g else None
    r = evaluation.chain_stats(x, mean=mean, std=std, all_lags=True, return_p=True)
    assert r['acceptance'] == g[name + '_acceptance']
    np.testing.assert_allclose(r['jump_distance'], g[name + '_jump'], rtol=1e-5)
    pg = g[name + '_p']
    np.testing.assert_allclose(r['p'], pg, rtol=1e-5, atol=1e-6 * max(1.0, np.abs(pg).max()))
    np.testing.assert_allclose(r['ess'], g[name + '_ess'], rtol=1e-5)
    if x.shape[0] > 1:
        np.testing.assert_allclose(r['rhat'], g[name + '_rhat'], rtol=1e-5)
    # the reference's functions by name
    assert evaluation.acceptance_rate(x) == g[name + '_acceptance']
    np.testing.assert_allclose(evaluation.mean_jump_distance(x), g[name + '_jump'], rtol=1e-5)
    mu, sd = (r['mean'], r['std'])
    np.testing.assert_allclose(evaluation.effective_sample_size(x, mu, sd), g[name + '_ess'], rtol=1e-5)
    np.testing.assert_allclose(evaluation.auto_correlation_time(x, 1, mu, sd), pg[0], rtol=1e-5, atol=1e-6 * max(1.0, np.abs(pg).max()))
    if x.shape[0] > 1:
        np.testing.assert_allclose(evaluation.gelman_rubin_diagnostic(x), g[name + '_rhat'], rtol=1e-5)
        np.testing.assert_allclose(evaluation.gelman_rubin_diagnostic(x, mu=mu), chk.rhat(x.astype(np.float64), mu), rtol=1e-5)


SHAPES = [(1, 2, 1), (2, 3, 2), (17, 64, 5), (1000, 251, 50), (17, 1025, 100), (2, 1025, 5), (1000, 2, 100), (1, 251, 50),
          (17, 3, 1), (1000, 64, 2), (2, 251, 100), (1, 1025, 2), (17, 251, 1), (1000, 3, 5), (2, 64, 50)]


@pytest.mark.parametrize('C,T,D', SHAPES)
def test_shapes_against_restatement(C, T, D):
    x = chains(C, T, D, rho=0.9 if T > 300 else 0.8, seed=C + T + D)
    r = evaluation.chain_stats(x, return_p=True)
    check_against_restatement(r, x)


def test_every_lag_and_scales():
    x = chains(17, 300, 5, rho=0.97, reject=0.2, seed=3, scale=np.array([1e-2, 1.0, 10.0, 1e2, 3.0]))
    r = evaluation.chain_stats(x, all_lags=True, return_p=True)
    x64 = x.astype(np.float64)
    mu, sd = chk.moments(x64)
    p_ref = chk.autocorr(x64, mu, sd)
    np.testing.assert_allclose(r['p'], p_ref, rtol=1e-5, atol=1e-6 * np.abs(p_ref).max())


def test_strided_prefix_in_place():
    h = torch.from_numpy(chains(40, 600, 7, seed=5)).cuda()
    for t in (2, 120, 333):
        a = evaluation.chain_stats(h[:, :t], return_p=True)
        b = evaluation.chain_stats(h[:, :t].contiguous(), return_p=True)
        for k in ('acceptance', 'jump_distance', 'stop_lag'):
            assert a[k] == b[k]
        for k in ('ess', 'rhat', 'mean', 'std', 'p'):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    # a view whose dimension stride is not 1 is copied, with the same result
    hv = torch.from_numpy(chains(40, 50, 7, seed=6)).cuda().transpose(0, 1).contiguous().transpose(0, 1)
    a = evaluation.chain_stats(hv)
    b = evaluation.chain_stats(hv.contiguous())
    assert np.array_equal(a['ess'], b['ess'])


def test_affine_on_load():
    x = chains(17, 251, 5, seed=7)
    a = np.array([0.5, 2.0, 3.0, 1e-2, 7.0])
    b = np.array([1.0, -3.0, 0.0, 10.0, 0.25])
    r = evaluation.chain_stats(x, affine=(a, b), return_p=True)
    v = x.astype(np.float64) * a + b
    check_against_restatement(r, v)
    r2 = evaluation.chain_stats(torch.from_numpy(v.astype(np.float32)).cuda())
    assert r2['acceptance'] == r['acceptance']
    np.testing.assert_allclose(r2['ess'], r['ess'], rtol=1e-4)


def test_lag_blocked_stop_equals_every_lag():
    for (C, T, D, rho) in ((17, 1025, 5, 0.99), (1000, 251, 50, 0.8), (4, 3000, 3, 0.995)):
        x = chains(C, T, D, rho=rho, seed=T)
        a = evaluation.chain_stats(x, return_p=True)
        b = evaluation.chain_stats(x, all_lags=True, return_p=True)
        assert a['stop_lag'] == b['stop_lag']
        assert np.array_equal(a['ess'], b['ess'])
        n = min(a['stop_lag'], T - 1)
        assert np.array_equal(a['p'][:n], b['p'][:n])
        assert not np.isnan(b['p']).any()


def test_bitwise_repeatable_and_numpy_equals_tensor():
    x = chains(1000, 251, 50, seed=11)
    a = evaluation.chain_stats(x, return_p=True)
    b = evaluation.chain_stats(x, return_p=True)
    c = evaluation.chain_stats(torch.from_numpy(x).cuda(), return_p=True)
    for r in (b, c):
        for k in ('acceptance', 'jump_distance', 'stop_lag'):
            assert a[k] == r[k]
        for k in ('ess', 'rhat', 'mean', 'std', 'p'):
            assert np.array_equal(a[k], r[k], equal_nan=True), k


def _staged_sums(lib, t, aff, center, work, st):
    C, T, D = t.shape
    sums = torch.empty(3 + 3 * D, dtype=torch.float64, device='cuda')
    _lib.check(lib.nnest_chain_stats_chains(_lib.ptr(t), C, T, D, t.stride(0), t.stride(1), aff, _lib.ptr(center), _lib.ptr(work),
                                            _lib.ptr(sums), st))
    return sums


def test_half_batch_sums_add_up():
    """the chain sums and the lag sums of two halves, added, give the whole batch (the sharded path); ShardedChainStats too"""
    lib = _lib.load()
    x = torch.from_numpy(chains(34, 251, 5, seed=13)).cuda()
    C, T, D = x.shape
    st = _lib.current_stream(x.device)
    whole = evaluation.chain_stats(x)
    halves = [x[:17], x[17:]]
    works = [torch.empty(lib.nnest_chain_stats_work_words(17, T, D), dtype=torch.float64, device='cuda') for _ in halves]
    mu = torch.from_numpy(whole['mean']).cuda()
    sd = torch.from_numpy(whole['std']).cuda()
    sums = [_staged_sums(lib, h, None, mu, w, st) for h, w in zip(halves, works)]   # the same centre on both halves
    total = sums[0] + sums[1]
    for w in works:
        _lib.check(lib.nnest_chain_stats_prepare(_lib.ptr(total), 17, T, D, _lib.ptr(mu), _lib.ptr(sd), _lib.ptr(w), st))
    lag = [torch.empty((256, D), dtype=torch.float64, device='cuda') for _ in halves]
    for h, w, l in zip(halves, works, lag):
        _lib.check(lib.nnest_chain_stats_lags(_lib.ptr(h), 17, T, D, h.stride(0), h.stride(1), None, 1, 256, 0, _lib.ptr(w), _lib.ptr(l), st))
    lag_total = lag[0] + lag[1]
    out = torch.empty(4 + 4 * D, dtype=torch.float64, device='cuda')
    _lib.check(lib.nnest_chain_stats_advance(_lib.ptr(total), _lib.ptr(lag_total), 17, T, D, 1, 256, 0, _lib.ptr(works[0]), None, st))
    _lib.check(lib.nnest_chain_stats_finish(_lib.ptr(total), 17, T, D, 0, _lib.ptr(works[0]), _lib.ptr(out), st))
    o = out.cpu().numpy()
    assert o[0] == whole['acceptance'] and o[3] == C
    np.testing.assert_allclose(o[1], whole['jump_distance'], rtol=1e-12)
    np.testing.assert_allclose(o[4:4 + D], whole['ess'], rtol=1e-9)
    np.testing.assert_allclose(o[4 + D:4 + 2 * D], whole['rhat'], rtol=1e-9)
    # the same through ShardedChainStats, one rank standing for two: its all-reduce doubles the sums of a batch of two equal halves
    xx = torch.cat([x[:17], x[:17]])
    ref = evaluation.chain_stats(xx, mean=whole['mean'], std=whole['std'])
    acc, ess, jump = evaluation.ShardedChainStats(lambda t: t.mul_(2.0))(x[:17], whole['mean'], whole['std'])
    assert acc == ref['acceptance']
    np.testing.assert_allclose(ess, ref['ess'], rtol=1e-9)
    np.testing.assert_allclose(jump, ref['jump_distance'], rtol=1e-12)


def test_bad_arguments_return_codes_and_launch_nothing():
    lib = _lib.load()
    x = torch.from_numpy(chains(4, 10, 3)).cuda()
    work = torch.zeros(lib.nnest_chain_stats_work_words(4, 10, 3), dtype=torch.float64, device='cuda')
    out = torch.full((16,), 7.0, dtype=torch.float64, device='cuda')
    st = _lib.current_stream(x.device)
    P, W, O = _lib.ptr(x), _lib.ptr(work), _lib.ptr(out)
    assert lib.nnest_chain_stats_work_words(0, 10, 3) == -1
    assert lib.nnest_chain_stats_work_words(4, 1, 3) == -1
    assert lib.nnest_chain_stats_work_words(4, 10, 0) == -1
    bad = [(P, 0, 10, 3, 30, 3), (P, 4, 1, 3, 30, 3), (P, 4, 10, 0, 30, 3), (None, 4, 10, 3, 30, 3), (P, 4, 10, 3, -30, 3),
           (P, 4, 10, 3, 30, -3)]
    for (xp, C, T, D, cs, ss) in bad:
        assert lib.nnest_chain_stats(xp, C, T, D, cs, ss, None, None, None, 0, W, None, O, st) == E_ARG
    assert lib.nnest_chain_stats(P, 4, 10, 3, 30, 3, None, None, None, 0, None, None, O, st) == E_ARG
    assert lib.nnest_chain_stats(P, 4, 10, 3, 30, 3, None, None, None, 0, W, None, None, st) == E_ARG
    assert lib.nnest_chain_stats(P, 4, 10, 3, 30, 3, None, None, None, 64, W, None, O, st) == E_ARG
    assert lib.nnest_chain_stats(P, 4, 10, 3, 30, 3, None, None, None, _lib.CHAIN_STATS_RHAT_AT_MEAN, W, None, O, st) == E_ARG
    lag = torch.zeros((256, 3), dtype=torch.float64, device='cuda')
    assert lib.nnest_chain_stats_lags(P, 4, 10, 3, 30, 3, None, 1, 100, 0, W, _lib.ptr(lag), st) == E_ARG
    assert lib.nnest_chain_stats_lags(P, 4, 10, 3, 30, 3, None, 0, 256, 0, W, _lib.ptr(lag), st) == E_ARG
    assert b'chain_stats' in lib.nnest_hip_last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(out == 7.0)) and bool(torch.all(work == 0.0)) and bool(torch.all(lag == 0.0))
    with pytest.raises(ValueError):
        evaluation.chain_stats(np.zeros((3, 1, 2), np.float32))


def test_large_offset_moments():
    """chain means far from zero compared with their spread: the centred sums keep std and R-hat at float64 accuracy"""
    x = (chains(200, 251, 4, seed=21).astype(np.float64) * 0.5 + np.array([1e5, -3e4, 2e4, 7.0])).astype(np.float32)
    r = evaluation.chain_stats(x, return_p=True)
    check_against_restatement(r, x)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(evaluation.gelman_rubin_diagnostic(x, mu=x64.reshape(-1, 4).mean(0)),
                               chk.rhat(x64, x64.reshape(-1, 4).mean(0)), rtol=1e-5)
