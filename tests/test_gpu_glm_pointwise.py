"""GPU checks of the pointwise predictive statistics of the regression likelihoods (include/nnest_hip.h nnest_glm_pointwise,
nnest_glm_predict, nnest_glm_pointwise_groups; flow.glm_pointwise, flow.glm_predict, GLMData.pointwise, GLMData.predict,
evaluation.predictive_criteria):
  1. both entries against float64 within the a-priori bounds of tests/glm_pointwise_check.py, at every tile width, around the
     16-row block, the 64-row groups and the padding of ld, with garbage in the padded rows;
  2. dead draws (NaN, +inf, -inf coordinates) are not counted and poison nothing;
  3. the same call twice gives the same bits;
  4. nothing is written behind stats[n] or the partials' end;
  5. a run cut into launches and merged on the host is the same run;
  6. the front ends, 'fused' against 'host', on the draws of a fused Metropolis run.

Data: tests/glm_check.make_like(D, n, family, D + n); draws N(0, 1) U(0.2, 1.0) per row (tests/glm_pointwise_check.draws).  The
large S of 1. is 1003: 63 tiles of 16 with a ragged last one, over G <= 16 draw groups (asserted from nnest_glm_pointwise_groups),
so that every workgroup runs three or four passes of its draw loop.

Measured on the MI355X, the worst share of each bound over all cases of 1.: a, b, lppd, elpd_isloo and mean 0.142 (poisson, x_dim 1,
at S = 1, where the five coincide), var 0.030, isloo_ess 0.037, predict mean 0.154, predict var 0.032; at x_dim 128 nothing is above
0.0093.  In 6., 'fused' against 'host': at most 0.104 (b, logistic) for pointwise and 0.040 for predict."""
import ctypes

import numpy as np
import pytest
import scipy.special
import torch

from tests import glm_check as gk
from tests import glm_pointwise_check as pk

pytestmark = pytest.mark.gpu

S_BIG = 1003
WIDTHS = [1, 5, 32, 33, 64, 65, 100, 128]
ROWS = [1, 15, 16, 17, 63, 64, 65, 70, 200]


def groups_of(S, n):
    from nnest_amd import _lib
    return int(_lib.load().nnest_glm_pointwise_groups(int(S), int(n)))


def run(data, t, predict=False):
    from nnest_amd import flow
    fn = flow.glm_predict if predict else flow.glm_pointwise
    return fn(data, t).cpu().numpy()


def garbage_in_padding(data):
    """the descriptor with something else in the padded rows n .. ld - 1 of at, y and o"""
    n = int(data['n'])
    out = dict(data)
    for k, fill in (('at', 1e30), ('y', np.nan), ('o', -np.inf)):
        a = np.array(data[k], np.float32)
        a[..., n:] = fill
        a[..., n + 1:] = 7.25
        out[k] = a
    return out


def same_bits(p, q):
    return np.array_equal(np.asarray(p).view(np.uint64), np.asarray(q).view(np.uint64))


def rel_close(p, q, tol=1e-12):
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    with np.errstate(invalid='ignore'):
        return bool(np.all((p == q) | (np.abs(p - q) <= tol * np.maximum(np.abs(p), np.abs(q)))))


# ---- 1. against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', WIDTHS)
def test_against_float64_within_the_bounds(family, D):
    worst = {}
    for n in ROWS:
        if n == 200 and D not in (5, 65):
            continue
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        junk = garbage_in_padding(data)
        for S in (S_BIG, 1, 17):
            G, tiles = groups_of(S, n), (S + 15) // 16
            assert G >= 1 and (S != S_BIG or (tiles // G >= 2 and S % 16 != 0))   # two passes and more a workgroup, a ragged tail
            t = pk.draws(S, D, 7 * D + n + S)
            for predict, (bounds, want) in ((False, pk.data_bounds(data, t)), (True, pk.data_predict_bounds(data, t))):
                got = run(data, t, predict)
                assert got.shape == want.shape and not np.any(np.isnan(got))
                for k, v in pk.shares(got, want, bounds).items():
                    key = ('predict ' if predict else '') + k
                    worst[key] = max(worst.get(key, 0.0), v)
                assert same_bits(run(junk, t, predict), got), (n, S, predict)   # (rows n .. ld - 1 are masked)
    print('worst shares of the bounds, %s D=%d: %s' % (family, D, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    assert worst.pop('cnt') == 0.0 and worst.pop('predict cnt') == 0.0
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 2. dead draws ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', [5, 65])
def test_dead_draws_are_not_counted(family, D):
    n = 70
    data = gk.make_like(D, n, family, D + n).hip_like_glm
    t = pk.draws(S_BIG, D, 11)
    bad = t.copy()
    rows, cols = (3, 500, S_BIG - 1), (0, D // 2, D - 1)
    for r, c, v in zip(rows, cols, (np.nan, np.inf, -np.inf)):
        bad[r, c] = v
    keep = np.setdiff1d(np.arange(S_BIG), rows)
    for predict in (False, True):
        got, ref = run(data, bad, predict), run(data, t[keep], predict)
        assert not np.any(np.isnan(got))
        assert np.array_equal(got[:, -3], np.full(n, S_BIG - 3.0)) and np.array_equal(ref[:, -3], got[:, -3])
        assert rel_close(got, ref), np.max(np.abs(got - ref))
    # draws that are all dead: the empty statistics
    from nnest_amd import _lib
    dead = np.full((5, D), np.nan, np.float32)
    assert np.array_equal(run(data, dead), _lib.empty_glm_pointwise(n)) and np.array_equal(run(data, dead, True), np.zeros((n, 3)))


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_the_same_call_twice_gives_the_same_bits(family):
    for D, n, S in ((5, 40, 5000), (65, 200, S_BIG), (128, 17, 333)):
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        t = pk.draws(S, D, 5)
        for predict in (False, True):
            first = run(data, t, predict)
            for _ in range(3):
                assert same_bits(run(data, t, predict), first)


# ---- 4. bounds of the outputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('predict', [False, True])
def test_guard_rows_stay_untouched(family, predict):
    from nnest_amd import _lib, flow
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    fn, slots = (lib.nnest_glm_predict, 3) if predict else (lib.nnest_glm_pointwise, 8)
    for D, n in ((5, 17), (33, 70)):
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        spec, keep = flow.glm_spec(data, dev)
        for S in (0, 1, 3, 17):
            G = groups_of(S, n)
            assert G == (0 if S == 0 else 1)
            t = torch.from_numpy(pk.draws(max(S, 1), D, S)).to(dev)
            stats = torch.full((n + 1, slots), -77.5, dtype=torch.float64, device=dev)
            partials = torch.full((max(G, 1) * n + 1, slots), -77.5, dtype=torch.float64, device=dev)
            _lib.check(fn(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(stats), _lib.ptr(partials), S, D, _lib.current_stream(dev)))
            torch.cuda.synchronize()
            st, pa = stats.cpu().numpy(), partials.cpu().numpy()
            assert np.all(st[n] == -77.5) and np.all(pa[G * n:] == -77.5), (D, n, S)
            assert not np.any(st[:n] == -77.5)
            if S == 0:
                assert np.array_equal(st[:n], _lib.empty_glm_pointwise(n, slots))
            else:
                assert np.array_equal(st[:n, -3], np.full(n, float(S))) and same_bits(st[:n], run(data, t[:S].cpu().numpy(), predict))


# ---- 5. a run cut into launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D,n', [(5, 40), (65, 200), (128, 63)])
def test_a_cut_run_is_the_same_run(family, D, n):
    from nnest_amd import _lib
    data = gk.make_like(D, n, family, D + n).hip_like_glm
    t = pk.draws(S_BIG, D, 21)
    for predict in (False, True):
        whole = run(data, t, predict)
        merged = _lib.empty_glm_pointwise(n, whole.shape[1])
        for first, count in ((0, 400), (400, 13), (413, S_BIG - 413)):
            merged = _lib.merge_glm_pointwise(merged, run(data, t[first:first + count], predict))
        assert np.array_equal(merged[:, -3], whole[:, -3]) and rel_close(merged, whole), np.max(np.abs(merged - whole))


# ---- 6. the front ends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_front_ends_fused_against_host(tmp_path, family):
    """The host route is float64 from the float64 data and the float64 draws (sampler.samples holds T(x) in float64); the fused
    route reads the descriptor, whose A and offset are rounded to float32, and the draws rounded to float32.  So beside the
    evaluation's own e_is = gamma_{D + 2} (|o_i| + sum_c |A[i, c]| |theta_sc|) (tests/glm_check.eta_error) the eta of the rounded
    inputs is off the host's by at most gamma (|o_i| + sum_c |A[i, c]| |theta_sc|), gamma = 2 v / (1 - 2 v), v = 2^-24: one
    rounding to nearest of each A[i, c] and of each theta_sc -- (1 + v)^2 - 1 <= gamma on every product -- and one of o_i, the
    products and the sum then exact in this accounting."""
    import nnest_amd
    from nnest_amd.evaluation import predictive_criteria
    from tests.test_gpu_mcmc_glm import laplace_draws
    like = gk.make_like(2, 40, family, 5)
    rng = np.random.RandomState(3)
    N, steps, A = 64, 150, 50
    train = laplace_draws(like, rng, 2000)
    init = (train[:N] - train.mean(0)) / train.std(0)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(2, like, log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.run(steps, N, train, init_samples=init, route='fused', seed=1, adapt_steps=A, global_every=5)
    assert s.mcmc_route == 'fused'
    x = s.samples[:, A + 1:, :]
    th = np.asarray(x, np.float64).reshape(-1, 2)
    S = th.shape[0]
    assert S == N * (steps - A)
    v = 2.0 ** -24
    gamma = 2.0 * v / (1.0 - 2.0 * v)
    e = gk.eta_error(like.hip_like_glm, th) + gamma * (np.abs(like.offset) + np.abs(th) @ np.abs(like.A).T)
    eta = like.offset + th @ like.A.T
    # pointwise
    bounds = pk.pointwise_bounds(family, like.y, eta, gk.terms(family, eta, like.y), e)
    host, route_h = like.pointwise_stats(x, route='host')
    fused, route_f = like.pointwise_stats(x, route='fused', chunk=2500)   # (four launches, merged)
    assert (route_h, route_f) == ('host', 'fused')
    sh = pk.shares(fused, host, bounds)
    print('%s pointwise, fused against host, shares of the bounds: %s' % (family, ', '.join('%s %.3g' % kv for kv in sorted(sh.items()))))
    assert sh.pop('cnt') == 0.0 and all(val <= 1.0 for val in sh.values()), sh
    pw = like.pointwise(x)   # (None: 'fused' where a device is available)
    assert like.pointwise_route == 'fused' and np.array_equal(pw['n_live'], np.full(40, float(S)))
    norm = -scipy.special.gammaln(like.y + 1.0) if family == 'poisson' else np.zeros(40)
    assert family != 'poisson' or np.any(norm < -0.5)
    raw = pk.derived(like.pointwise_stats(x, route='fused')[0])
    for k, r in (('lppd', 'lppd'), ('elpd_isloo', 'elpd_isloo'), ('mean_logl', 'mean')):
        np.testing.assert_allclose(pw[k], raw[r] + norm, rtol=0, atol=1e-12)   # (the Poisson lgamma term is there)
    np.testing.assert_allclose(pw['elpd_waic'], pw['lppd'] - pw['p_waic'], rtol=0, atol=1e-12)
    res = predictive_criteria(like, x)
    assert res['route'] == 'fused' and res['n_samples'] == S
    assert all(np.isfinite(res[k]) for k in ('elpd_waic', 'p_waic', 'lppd', 'elpd_isloo', 'elpd_waic_se', 'lppd_se', 'min_isloo_ess'))
    assert res['p_waic'] > 0.0 and res['elpd_waic'] < res['lppd'] and 1.0 <= res['min_isloo_ess'] <= S
    # predict
    A_new, o_new = rng.uniform(-1, 1, (13, 2)) / np.sqrt(2.0), rng.uniform(-0.2, 0.2, 13)
    eta_n = o_new + th @ A_new.T
    new = dict(at=A_new.T.astype(np.float32), o=o_new.astype(np.float32), y=np.zeros(13, np.float32), n=13, family=family, logl0=0.0)
    e_n = gk.eta_error(new, th) + gamma * (np.abs(o_new) + np.abs(th) @ np.abs(A_new).T)
    mu = pk.inverse_link(family, eta_n)
    pb = pk.predict_bounds(family, eta_n, mu, e_n)
    ph, pf = like.predict(x, A_new, o_new, route='host'), like.predict(x, A_new, o_new, route='fused')
    assert like.predict_route == 'fused' and np.array_equal(pf['n_live'], ph['n_live']) and np.all(pf['n_live'] == S)
    share_mean = np.max(np.abs(pf['mean'] - ph['mean']) / pb['mean'])
    share_var = np.max(np.abs(pf['sd'] ** 2 - ph['sd'] ** 2) / pb['var'])
    print('%s predict, fused against host, shares of the bounds: mean %.3g, var %.3g' % (family, share_mean, share_var))
    assert share_mean <= 1.0 and share_var <= 1.0
    np.testing.assert_allclose(ph['mean'], mu.mean(axis=0), rtol=1e-12)
