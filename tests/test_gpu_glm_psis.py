"""GPU checks of Pareto-smoothed leave-one-out and the matrix of terms of the regression likelihoods (include/nnest_hip.h
nnest_glm_terms, nnest_glm_psis, nnest_glm_psis_work_bytes, nnest_glm_psis_tail_cap; flow.glm_terms, flow.glm_psis,
GLMData.pointwise(psis=True), GLMData.log_lik, evaluation.predictive_criteria(psis=True)):
  1. nnest_glm_terms against float64 within tests/glm_pointwise_check.py's per-term bound, its column maxima and live counts the
     bits of nnest_glm_pointwise's slots 2 and 5;
  2. the selection, exactly: c, M, N_body and the sorted tail against nnest_amd/psis.py on the device's own exported l; B and B2
     within (S + 4) 2^-52 relative;
  3. the fit -- khat, sigma, elpd_psis, psis_ess -- against the same within tests/psis_check.GPU_TOL = 8 x the float64 definition's
     worst distance from long double (floor 1e-13);
  4. dead draws are excluded; 5. duplicated draws; 6. determinism and masking; 7. guard rows and argument errors; 8. the front ends.

Data: tests/glm_check.make_like(D, n, family, D + n), draws tests/glm_pointwise_check.draws.  2. and 3. run x_dim 5, 33, 65, 128 (one
per tile count) x n 1, 17, 70 x S 1 (no tail), 17 (M* < 5), 24 (the last size without a fit), 25 (the first with one), 1003 (a ragged
tile), 4001 (several passes of a draw group's loop, asserted from nnest_glm_pointwise_groups) x both families.

Measured on the MI355X: 1. at most 0.183 of the per-term bound (poisson, x_dim 5; 0.016 at x_dim 128).  2. bit-equal in every case.
3. the worst distances over all cases: khat 1.92e-14 (logistic, x_dim 5), sigma 1.44e-15, elpd_psis 9.29e-15, psis_ess 5.46e-14
(poisson, x_dim 5), of 3.36e-11 allowed.  8. khat of row 0 0.7434 on both routes, elpd_psis 'fused' against 'host' within 1.44e-7
(DESIGN.md 3.19)."""
import ctypes

import numpy as np
import pytest
import torch

from nnest_amd import psis
from tests import glm_check as gk
from tests import glm_pointwise_check as pk
from tests import psis_check as pc

pytestmark = pytest.mark.gpu


def dev_terms(data, t):
    from nnest_amd import flow
    return flow.glm_terms(data, t).cpu().numpy()


def dev_psis(data, t):
    """(stats [n, 8], out [n, 16], the rows' tails) of the device"""
    from nnest_amd import _lib, flow
    stats, out, work = flow.glm_psis(data, t, with_work=True)
    n, S = int(data['n']), len(t)
    mcap = int(_lib.load().nnest_glm_psis_tail_cap(S))
    out = out.cpu().numpy()
    buf = work[:8 * n * mcap].view(torch.float64).reshape(n, mcap).cpu().numpy()
    return stats.cpu().numpy(), out, [buf[i, :int(out[i, psis.M])].copy() for i in range(n)]


def same_bits(p, q):
    return np.array_equal(np.asarray(p, np.float64).view(np.uint64), np.asarray(q, np.float64).view(np.uint64))


def compare(got, tails, l, worst, what):
    """2. and 3. of one case against nnest_amd/psis.py on the terms l"""
    S = l.shape[0]
    want, wtails = psis.psis_rows(l, return_tails=True)
    for s in (psis.C, psis.M, psis.N_BODY, psis.M_STAR, psis.FLAG):
        assert same_bits(got[:, s], want[:, s]), (what, s, got[:, s], want[:, s])
    for i in range(len(want)):
        assert same_bits(tails[i], wtails[i]), (what, i)
    for s in (psis.B, psis.B2):
        assert np.all(np.abs(got[:, s] - want[:, s]) <= (S + 4) * 2.0 ** -52 * want[:, s]), (what, s)
    rows = [dict(khat=w[psis.KHAT], sigma=w[psis.SIGMA], elpd=w[psis.ELPD], ess=w[psis.ESS]) for w in want]
    for k, v in pc.distance(got, rows).items():
        worst[k] = max(worst.get(k, 0.0), v)
        assert v <= pc.GPU_TOL, (what, k, v)
    assert np.all(got[:, 14:] == 0.0)


# ---- 1. the matrix of terms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', pc.WIDTHS)
def test_terms_against_float64(family, D):
    from nnest_amd import flow
    worst = 0.0
    for n in pc.ROWS:
        data = pc.case_data(family, D, n)
        _, _, y, _ = gk._parts(data)
        for S in (1003, 17, 1):
            t = pk.draws(S, D, 7 * D + n + S)
            got = dev_terms(data, t)
            _, eta, l = gk.exact(data, t)
            e = gk.eta_error(data, t)
            lip = np.ones_like(eta) if family == 'logistic' else np.abs(y) + np.exp(eta + e)
            mag = np.abs(l) + np.abs(y * eta) + (np.exp(eta) if family == 'poisson' else 0.0)
            delta = lip * e + 16 * 2.0 ** -53 * mag   # (glm_pointwise_check.pointwise_bounds' delta_is)
            assert got.shape == (S, n) and np.all(np.isfinite(got))
            worst = max(worst, float(np.max(np.abs(got - l) / delta)))
            st = flow.glm_pointwise(data, t).cpu().numpy()
            assert same_bits(np.max(-got, axis=0), st[:, 2]) and np.array_equal(st[:, 5], np.full(n, float(S)))
    print('terms, worst share of the per-term bound, %s D=%d: %.3g' % (family, D, worst))
    assert worst <= 1.0


# ---- 2., 3. the selection and the fit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', pc.WIDTHS)
def test_selection_exactly_and_fit_within_tolerance(family, D):
    from nnest_amd import _lib
    worst = {}
    for fam, d, n, S, seed in pc.gpu_cases():
        if (fam, d) != (family, D):
            continue
        if S == 4001:
            G = int(_lib.load().nnest_glm_pointwise_groups(S, n))
            assert G >= 1 and ((S + 15) // 16) // G >= 2   # (several passes of a draw group's loop)
        data = pc.case_data(family, D, n)
        t = pk.draws(S, D, seed)
        l = dev_terms(data, t)
        stats, got, tails = dev_psis(data, t)
        assert same_bits(np.max(-l, axis=0), stats[:, 2])
        compare(got, tails, l, worst, (family, D, n, S))
        fitted = got[:, psis.M] >= 5
        assert np.all(fitted == (S >= 25)) and np.all(np.isfinite(got[fitted, psis.KHAT])) and np.all(np.isposinf(got[~fitted, psis.KHAT]))
    print('fit against the float64 definition, worst distances, %s D=%d: %s (allowed %.3g)'
          % (family, D, ', '.join('%s %.3g' % kv for kv in sorted(worst.items())), pc.GPU_TOL))


# ---- 4. dead draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_dead_draws_are_excluded(family):
    D, n, S = 33, 70, 1003
    data = pc.case_data(family, D, n)
    t = pk.draws(S, D, 11)
    bad = t.copy()
    rows = (3, 500, S - 1)
    for r, c, v in zip(rows, (0, D // 2, D - 1), (np.nan, np.inf, -np.inf)):
        bad[r, c] = v
    l = dev_terms(data, bad)
    assert np.all(np.isnan(l[list(rows)])) and np.all(np.isfinite(np.delete(l, rows, axis=0)))
    _, got, tails = dev_psis(data, bad)
    worst = {}
    compare(got, tails, l, worst, 'dead')
    _, ref, rtails = dev_psis(data, np.delete(t, rows, axis=0))
    for s in (psis.C, psis.M, psis.N_BODY, psis.M_STAR, psis.FLAG):
        assert same_bits(got[:, s], ref[:, s])
    assert all(same_bits(a, b) for a, b in zip(tails, rtails))
    rr = [dict(khat=w[psis.KHAT], sigma=w[psis.SIGMA], elpd=w[psis.ELPD], ess=w[psis.ESS]) for w in ref]
    assert max(pc.distance(got, rr).values()) <= pc.GPU_TOL
    # all dead: the empty result
    _, got, tails = dev_psis(data, np.full((5, D), np.nan, np.float32))
    assert np.array_equal(got, np.stack([psis.empty_row()] * n), equal_nan=True) and all(len(x) == 0 for x in tails)
    _, got, _ = dev_psis(data, np.zeros((0, D), np.float32))
    assert np.array_equal(got, np.stack([psis.empty_row()] * n), equal_nan=True)


# ---- 5. duplicated draws --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_duplicated_draws_go_in_or_out_together(family):
    D, n = 5, 17
    data = pc.case_data(family, D, n)
    t = np.repeat(pk.draws(400, D, 13), 5, axis=0)
    _, got, tails = dev_psis(data, t)
    compare(got, tails, dev_terms(data, t), {}, 'dup')
    assert np.all(got[:, psis.M] % 5 == 0) and np.all(got[:, psis.M] > 0)


# ---- 6. determinism and masking ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_same_bits_over_four_calls_and_masked_padding(family):
    for D, n, S in ((5, 70, 4001), (65, 17, 1003)):
        data = pc.case_data(family, D, n)
        junk = dict(data)
        for k, fill in (('at', 1e30), ('y', np.nan), ('o', -np.inf)):
            a = np.array(data[k], np.float32)
            a[..., n:] = fill
            a[..., n + 1:] = 7.25
            junk[k] = a
        t = pk.draws(S, D, 5)
        _, first, ftails = dev_psis(data, t)
        for d in (data, data, data, junk):
            _, again, tails = dev_psis(d, t)
            assert same_bits(again, first) and all(same_bits(a, b) for a, b in zip(tails, ftails))
        assert same_bits(dev_terms(junk, t), dev_terms(data, t))


# ---- 7. guard rows and argument errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_guard_rows_stay_untouched_and_argument_errors(family):
    from nnest_amd import _lib, flow
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    GUARD = -77.5
    for D, n in ((5, 17), (33, 70)):
        data = pc.case_data(family, D, n)
        spec, keep = flow.glm_spec(data, dev)
        for S in (0, 3, 40, 1003):
            t = torch.from_numpy(pk.draws(max(S, 1), D, S)).to(dev)
            stats = flow.glm_pointwise(data, t[:S])
            nbytes, mcap = int(lib.nnest_glm_psis_work_bytes(S, n)), int(lib.nnest_glm_psis_tail_cap(S))
            assert nbytes % 8 == 0 and nbytes >= 8 * n * mcap
            work = torch.full((nbytes // 8 + 4,), GUARD, dtype=torch.float64, device=dev)
            out = torch.full((n + 1, 16), GUARD, dtype=torch.float64, device=dev)
            terms = torch.full((S * n + 3,), GUARD, dtype=torch.float64, device=dev)
            _lib.check(lib.nnest_glm_psis(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(stats), _lib.ptr(out), _lib.ptr(work), S, D,
                                          _lib.current_stream(dev)))
            _lib.check(lib.nnest_glm_terms(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(terms), S, D, _lib.current_stream(dev)))
            torch.cuda.synchronize()
            o, w, tm = out.cpu().numpy(), work.cpu().numpy(), terms.cpu().numpy()
            assert np.all(o[n] == GUARD) and not np.any(o[:n] == GUARD) and np.all(w[nbytes // 8:] == GUARD), (D, n, S)
            assert np.all(tm[S * n:] == GUARD) and not np.any(tm[:S * n] == GUARD)
            tail = w[:n * mcap].reshape(n, mcap)
            for i in range(n):   # (the tail buffer: a row's slots behind its M_i are not written)
                M = int(o[i, psis.M])
                assert np.all(tail[i, M:] == GUARD) and not np.any(tail[i, :M] == GUARD)
            if S == 0:
                assert np.array_equal(o[:n], np.stack([psis.empty_row()] * n), equal_nan=True)
    # argument errors: NNEST_E_ARG, the outputs untouched
    assert lib.nnest_glm_psis_work_bytes((1 << 20) + 1, 4) == -1 and lib.nnest_glm_psis_work_bytes(10, 0) == -1
    assert lib.nnest_glm_psis_work_bytes(1 << 20, 65536) == -1 and lib.nnest_glm_psis_work_bytes(1 << 20, 1024) > 0
    assert lib.nnest_glm_psis_tail_cap(-1) == -1 and lib.nnest_glm_psis_tail_cap(0) == 1 and lib.nnest_glm_psis_tail_cap(4001) == 190
    out.fill_(GUARD)
    work.fill_(GUARD)
    args = lambda **kw: [kw.get('spec', ctypes.byref(spec)), kw.get('t', _lib.ptr(t)), kw.get('stats', _lib.ptr(stats)), kw.get('out', _lib.ptr(out)),
                         kw.get('work', _lib.ptr(work)), kw.get('S', 1003), kw.get('D', D), _lib.current_stream(dev)]
    for kw in (dict(S=-1), dict(S=(1 << 20) + 1), dict(D=D + 1), dict(spec=None), dict(t=None), dict(stats=None), dict(out=None), dict(work=None)):
        assert lib.nnest_glm_psis(*args(**kw)) == 1, kw
    bad = _lib.GlmSpec(spec.at_dev, spec.y_dev, spec.o_dev, 0.0, n, 64 * ((n + 63) // 64) + 1, D, spec.family)
    assert lib.nnest_glm_psis(*args(spec=ctypes.byref(bad))) == 1
    for kw in (dict(S=-1), dict(D=D + 1), dict(out=None), dict(t=None)):
        a = args(**kw)
        assert lib.nnest_glm_terms(a[0], a[1], a[3], a[5], a[6], a[7]) == 1, kw
    torch.cuda.synchronize()
    assert bool(torch.all(out == GUARD)) and bool(torch.all(work == GUARD))


# ---- 8. the front ends --------------------------------------------------------------------------------------------------------------------------
def test_front_ends_fused_against_host():
    """tests/psis_check.outlier_case: row 0 sits at A = 4 with y = 0 against the trend, so its leave-one-out weights have a heavy tail.
    On the CPU (route 'host', seeds 0, 1, 2): khat of row 0 is 0.94, 0.74, 0.79, every other row at most 0.21, and on the rows with
    khat < 0.5 |elpd_psis - elpd_isloo| <= 2.5e-5."""
    from nnest_amd.evaluation import predictive_criteria
    from nnest_amd.likelihoods import GLMData
    A, y, th = pc.outlier_case(1)
    like = GLMData(A, y, family='logistic')
    S = len(th)
    before = like.pointwise(th, route='fused')
    assert sorted(before) == ['elpd_isloo', 'elpd_waic', 'isloo_ess', 'lppd', 'mean_logl', 'n_live', 'p_waic']
    res = {}
    for route in ('host', 'fused'):
        pw = like.pointwise(th, route=route, psis=True)
        assert like.pointwise_route == route
        assert sorted(set(pw) - set(before)) == ['elpd_psis', 'p_loo', 'pareto_k', 'psis_ess', 'psis_tail']
        k = pw['pareto_k']
        assert k[0] > 0.5 and np.all(k[1:] < 0.5), k
        assert np.all(pw['psis_ess'] <= pw['n_live']) and np.all(pw['n_live'] == S)
        assert np.max(np.abs(pw['elpd_psis'] - pw['elpd_isloo'])[k < 0.5]) <= 0.01
        np.testing.assert_allclose(pw['p_loo'], pw['lppd'] - pw['elpd_psis'], rtol=0, atol=1e-12)
        assert np.all(pw['psis_tail'] <= psis.tail_target(S)) and np.all(pw['psis_tail'] >= psis.tail_target(S) - 2)
        res[route] = pw
    for key in before:   # (psis=True leaves the other entries as they are)
        assert same_bits(res['fused'][key], before[key])
    print('fused against host: khat row 0 %.4f / %.4f, worst |elpd_psis| difference %.3g' % (
        res['fused']['pareto_k'][0], res['host']['pareto_k'][0], np.max(np.abs(res['fused']['elpd_psis'] - res['host']['elpd_psis']))))
    crit = predictive_criteria(like, th, psis=True)
    assert crit['route'] == 'fused' and crit['n_pareto_k_bad'] >= 1 and crit['max_pareto_k'] == res['fused']['pareto_k'][0]
    assert np.isfinite(crit['elpd_psis']) and np.isfinite(crit['elpd_psis_se']) and crit['p_loo'] > 0.0
    assert 'elpd_psis' not in predictive_criteria(like, th)
    ll = like.log_lik(th[:1003])
    assert like.log_lik_route == 'fused' and ll.shape == (1003, 30)
    np.testing.assert_allclose(ll, like.log_lik(th[:1003], route='host'), rtol=0, atol=1e-4)
    with pytest.raises(ValueError, match='thin'):
        like.pointwise(np.zeros(((1 << 20) + 1, 1)), psis=True)
