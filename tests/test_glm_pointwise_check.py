"""CPU checks of the pointwise predictive statistics of the regression likelihoods (GLMData.pointwise, GLMData.predict,
evaluation.predictive_criteria; include/nnest_hip.h nnest_glm_pointwise, nnest_glm_predict): the a-priori bounds of
tests/glm_pointwise_check.py against three legal float32 restatements, the merge, the host routes against the check module and
against direct float64, the properties the criteria must have, dead draws, and the library's entries and their argument errors,
which need no device."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import scipy.special

from tests import glm_check as gk
from tests import glm_pointwise_check as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_glm_pointwise_groups', 'nnest_glm_pointwise', 'nnest_glm_predict')
ORDERS = ('forward', 'reversed', 'pairwise')


# ---- 1. the bounds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', [1, 5, 33, 64, 65, 128])
def test_bounds_hold_for_three_orders(family, D):
    worst = {}
    for n in (1, 17, 70):
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        for S in (2, 17, 1003):
            t = pk.draws(S, D, 7 * D + n + S)
            for predict, (bounds, want) in ((False, pk.data_bounds(data, t)), (True, pk.data_predict_bounds(data, t))):
                assert np.all(np.isfinite(bounds['Delta'])) and np.all(want[:, -3] == S)
                for order in ORDERS:
                    got = pk.float32_stats(data, t, order, predict=predict)
                    for k, v in pk.shares(got, want, bounds).items():
                        key = ('predict ' if predict else '') + k
                        worst[key] = max(worst.get(key, 0.0), v)
    print('worst shares of the bounds, %s D=%d: %s' % (family, D, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    assert worst.pop('cnt') == 0.0 and worst.pop('predict cnt') == 0.0
    assert all(v <= 1.0 for v in worst.values()), worst
    # not vacuous: what a float32 eta costs is seen in the statistics that depend on it
    assert max(worst['lppd'], worst['mean']) > 1e-3 and worst['predict mean'] > 1e-3, worst


# ---- 2. the merge -----------------------------------------------------------------------------------------------------------------
def _close(p, q, tol=1e-12):
    p, q = np.asarray(p), np.asarray(q)
    same = (p == q) | (np.isnan(p) & np.isnan(q))
    scale = np.maximum(np.abs(p), np.abs(q))
    with np.errstate(invalid='ignore'):
        return np.all(same | (np.abs(p - q) <= tol * np.where(np.isfinite(scale), np.maximum(scale, 1.0), 1.0)))


@pytest.mark.parametrize('impl', ['check', 'lib'])
def test_merge_is_associative_and_takes_empty_sets(impl):
    from nnest_amd import _lib
    merge = pk.merge if impl == 'check' else _lib.merge_glm_pointwise
    r = np.random.RandomState(3)
    l = r.normal(-3.0, 2.0, size=(90, 6))
    l[:, 2] = np.nan            # a row with no live draw at all
    l[:40, 3] = np.nan          # a row that is dead in the first two parts
    l[5, 0] = -np.inf
    cuts = (l[:13], l[13:40], l[40:])
    for fn, whole in ((pk.stats, pk.stats(l)), (lambda v: pk.predict_stats(np.exp(v), v), pk.predict_stats(np.exp(l), l))):
        a, b, c = (fn(v) for v in cuts)
        left, right = merge(merge(a, b), c), merge(a, merge(b, c))
        assert _close(left, right) and _close(left, whole) and _close(merge(c, merge(a, b)), whole)
        e = pk.empty(6, whole.shape[1])
        assert np.array_equal(merge(e, e), e)
        assert np.array_equal(merge(e, whole), whole, equal_nan=True) and np.array_equal(merge(whole, e), whole, equal_nan=True)
        assert not np.any(np.isnan(left))
    whole = pk.stats(l)
    assert np.array_equal(whole[2], [-np.inf, 0, -np.inf, 0, 0, 0, 0, 0]) and whole[0, 5] == 89 and whole[3, 5] == 50
    assert np.array_equal(_lib.empty_glm_pointwise(4), pk.empty(4)) and np.array_equal(_lib.empty_glm_pointwise(4, 3), pk.empty(4, 3))
    with pytest.raises(ValueError):
        _lib.merge_glm_pointwise(np.zeros((3, 8)), np.zeros((3, 3)))


# ---- 3. the host routes against the check module ------------------------------------------------------------------------------------
def _posterior_like_draws(like, S, seed, spread=0.3):
    th, _ = gk.posterior_mode(like, -3.0, 3.0)
    r = np.random.RandomState(seed)
    return th + spread * r.standard_normal((S, like.x_dim))


@pytest.mark.parametrize('family', gk.FAMILIES)
def test_host_route_against_the_check_module(family, caplog):
    from nnest_amd.evaluation import predictive_criteria
    like = gk.make_like(4, 37, family, 11)
    x = _posterior_like_draws(like, 500, 1)
    eta = like.offset + x @ like.A.T
    l = gk.terms(family, eta, like.y)
    want = pk.derived(pk.stats(l))
    norm = -scipy.special.gammaln(like.y + 1.0) if family == 'poisson' else 0.0
    for chunk in (None, 1, 77, 500):
        pw = like.pointwise(x, route='host', chunk=chunk)
        assert like.pointwise_route == 'host'
        np.testing.assert_allclose(pw['lppd'], want['lppd'] + norm, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pw['elpd_isloo'], want['elpd_isloo'] + norm, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pw['mean_logl'], want['mean'] + norm, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pw['p_waic'], want['var'], rtol=1e-11, atol=1e-14)
        np.testing.assert_allclose(pw['elpd_waic'], want['lppd'] + norm - want['var'], rtol=0, atol=1e-12)
        np.testing.assert_allclose(pw['isloo_ess'], want['isloo_ess'], rtol=1e-11)
        assert np.array_equal(pw['n_live'], np.full(37, 500.0))
    # [N, steps, D] is flattened
    pw3 = like.pointwise(x.reshape(20, 25, 4), route='host')
    assert all(np.array_equal(pw3[k], pw[k]) for k in pw)
    # the direct formulae
    np.testing.assert_allclose(pw['lppd'], scipy.special.logsumexp(l, axis=0) - np.log(500) + norm, atol=1e-12)
    np.testing.assert_allclose(pw['elpd_isloo'], -(scipy.special.logsumexp(-l, axis=0) - np.log(500)) + norm, atol=1e-12)
    with caplog.at_level(logging.INFO, logger='nnest_amd.evaluation'):
        res = predictive_criteria(like, x, route='host')
    assert res['route'] == 'host' and res['n_samples'] == 500
    for k in ('elpd_waic', 'p_waic', 'lppd', 'elpd_isloo'):
        assert abs(res[k] - np.sum(pw[k])) <= 1e-10 and np.array_equal(res['pointwise'][k], pw[k])
        assert abs(res[k + '_se'] - np.sqrt(37 * np.var(pw[k], ddof=1))) <= 1e-10
    assert res['min_isloo_ess'] == np.min(pw['isloo_ess']) and 1.0 <= res['min_isloo_ess'] <= 500.0
    lines = [rec.getMessage() for rec in caplog.records if rec.name == 'nnest_amd.evaluation']
    assert len(lines) == 1 and 'elpd_waic' in lines[0] and 'route [host]' in lines[0]
    for bad in (x[:, :3], x[0], np.zeros((2, 3, 4, 4))):
        with pytest.raises(ValueError):
            like.pointwise(bad, route='host')
    with pytest.raises(ValueError):
        like.pointwise(x, route='gpu')


# ---- 4. draws that are all the same theta -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_identical_draws(family):
    like = gk.make_like(3, 21, family, 4)
    th = np.array([0.3, -0.7, 0.2])
    eta = like.offset + like.A @ th
    if family == 'logistic':
        logp = like.y * eta - np.logaddexp(0.0, eta)
    else:
        logp = like.y * eta - np.exp(eta) - scipy.special.gammaln(like.y + 1.0)
    pw = like.pointwise(np.tile(th, (50, 1)), route='host', chunk=7)
    assert np.all(pw['p_waic'] >= 0.0) and np.all(pw['p_waic'] <= 1e-24)   # (0 but for the rounding of the mean, squared)
    for k in ('lppd', 'elpd_isloo', 'mean_logl', 'elpd_waic'):
        np.testing.assert_allclose(pw[k], logp, rtol=0, atol=1e-12)
    np.testing.assert_allclose(pw['isloo_ess'], 50.0, rtol=1e-12)
    assert abs(np.sum(logp) + like.logl_const - like.loglike_rows(th[None])[0]) <= 1e-10   # (the rows add up to the likelihood)


# ---- 5. the criteria's inequalities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_waic_inequalities(family):
    like = gk.make_like(5, 70, family, 9)
    pw = like.pointwise(_posterior_like_draws(like, 300, 2), route='host')
    assert np.all(pw['p_waic'] >= 0.0) and np.all(pw['elpd_waic'] <= pw['lppd'])
    assert np.all(pw['mean_logl'] <= pw['lppd']) and np.all(pw['elpd_isloo'] <= pw['lppd'])   # (Jensen; harmonic <= arithmetic mean)
    assert np.all(pw['isloo_ess'] >= 1.0) and np.all(pw['isloo_ess'] <= 300.0 * (1 + 1e-12))
    one = like.pointwise(_posterior_like_draws(like, 1, 2), route='host')
    assert np.all(np.isnan(one['p_waic'])) and np.all(np.isfinite(one['lppd'])) and np.all(one['n_live'] == 1)


# ---- 6. a dead draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_a_nan_coordinate_kills_its_draw_for_every_row(family):
    like = gk.make_like(4, 33, family, 6)
    x = _posterior_like_draws(like, 120, 3)
    bad = np.insert(x, 57, x[10], axis=0)
    bad[57, 2] = np.nan
    ref, got = like.pointwise(x, route='host', chunk=200), like.pointwise(bad, route='host', chunk=200)
    ref_p, got_p = like.predict(x, like.A[:9], route='host'), like.predict(bad, like.A[:9], route='host')
    assert np.array_equal(got['n_live'], np.full(33, 120.0)) and np.array_equal(got_p['n_live'], np.full(9, 120.0))
    for r, g in ((ref, got), (ref_p, got_p)):
        for k in r:
            assert not np.any(np.isnan(g[k]))
            np.testing.assert_allclose(g[k], r[k], rtol=1e-12, atol=1e-13, err_msg=k)
    # nothing live at all
    dead = like.pointwise(np.full((3, 4), np.nan), route='host')
    assert np.all(dead['n_live'] == 0) and np.all(dead['isloo_ess'] == 0)
    assert all(np.all(np.isnan(dead[k])) for k in ('lppd', 'elpd_isloo', 'mean_logl', 'p_waic', 'elpd_waic'))
    none = like.pointwise(np.zeros((0, 4)), route='host')
    assert np.all(none['n_live'] == 0) and np.all(np.isnan(none['lppd']))


# ---- 7. predict ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
def test_predict_host_against_direct_float64(family):
    like = gk.make_like(4, 37, family, 11)
    x = _posterior_like_draws(like, 400, 5)
    r = np.random.RandomState(8)
    A_new, o_new = r.uniform(-1, 1, (13, 4)) / 2.0, r.uniform(-0.2, 0.2, 13)
    for off in (o_new, None):
        eta = (0.0 if off is None else off) + x @ A_new.T
        mu = 1.0 / (1.0 + np.exp(-eta)) if family == 'logistic' else np.exp(eta)
        p = like.predict(x, A_new, offset_new=off, route='host')
        np.testing.assert_allclose(p['mean'], mu.mean(axis=0), rtol=1e-13)
        np.testing.assert_allclose(p['sd'], mu.std(axis=0, ddof=1), rtol=1e-11)
        assert np.array_equal(p['n_live'], np.full(13, 400.0)) and like.predict_route == 'host'
    assert np.all(np.isnan(like.predict(x[:1], A_new, route='host')['sd']))
    for bad in (dict(A_new=A_new[:, :3]), dict(A_new=A_new[0]), dict(A_new=np.zeros((0, 4))), dict(A_new=A_new, offset_new=o_new[:5]),
                dict(A_new=np.where(A_new > 0.4, np.nan, A_new)), dict(A_new=A_new, offset_new=np.full(13, np.inf)),
                dict(A_new=np.zeros((65537, 4)))):
        with pytest.raises(ValueError):
            like.predict(x, route='host', **bad)
    # the bounds of the check module hold for predict's restatements too (test 1 has the grid); here: they are not vacuous
    data = like.hip_like_glm
    t = pk.draws(300, 4, 2)
    bounds, want = pk.data_predict_bounds(data, t)
    assert all(0.0 < v <= 1.0 for k, v in pk.shares(pk.float32_stats(data, t, 'reversed', predict=True), want, bounds).items() if k != 'cnt')


# ---- 8. the library ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from nnest_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.nnest_hip_version() == 15


def test_groups_need_no_device():
    from nnest_amd import _lib
    G = _lib.load().nnest_glm_pointwise_groups
    assert G(0, 40) == 0 and G(1, 40) == 1 and G(17, 40) == 1 and G(1 << 30, 65536) == 1
    for S, n in ((-1, 40), ((1 << 30) + 1, 40), (5, 0), (5, 65537)):
        assert G(S, n) == -1
    for n in (1, 40, 64, 65, 1024, 4097, 65536):
        for S in (1, 16, 17, 64, 65, 1003, 250000, 1 << 30):
            g = G(S, n)
            tiles = (S + 15) // 16
            assert 1 <= g <= 1024 and (g == 1 or g * n <= 65536)          # bounded partials: at most 4 MB
            assert g == 1 or tiles // g >= 2                                  # every group runs at least two passes of its loop
    assert G(250000, 1024) * ((1024 + 63) // 64) == 1024 and G(250000, 40) == 1024   # the whole device at small n


def test_argument_errors_are_reported_not_thrown():
    """every refusal comes before a launch, in the library's words, and leaves the outputs alone: the buffers here are host arrays
    holding a guard pattern (nothing reads or writes them: no device is needed)"""
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    guard = dict((name, np.full(64, 0x5A, np.uint8)) for name in ('stats', 'partials'))
    st, pa = (ctypes.c_void_p(guard[k].ctypes.data) for k in ('stats', 'partials'))
    p = ctypes.c_void_p(64)   # (inputs; never dereferenced)
    err = lib.nnest_hip_last_error

    def spec(**kw):
        s = _lib.GlmSpec(64, 64, 64, -3.25, 40, 64, 5, 0)
        for key, val in kw.items():
            setattr(s, key, val)
        return s

    bad_specs = [(dict(at_dev=None), b'NULL at_dev, y_dev or o_dev'), (dict(y_dev=None), b'NULL at_dev, y_dev or o_dev'),
                 (dict(o_dev=None), b'NULL at_dev, y_dev or o_dev'), (dict(D=0), b'glm: D=0'), (dict(D=129), b'glm: D=129'),
                 (dict(n=0), b'glm: n=0'), (dict(n=65537, ld=65600), b'glm: n=65537'), (dict(ld=32), b'glm: ld=32'),
                 (dict(ld=100), b'glm: ld=100'), (dict(n=65, ld=64), b'glm: ld=64'), (dict(ld=65600), b'glm: ld=65600'),
                 (dict(family=2), b'glm: family=2'), (dict(family=-1), b'glm: family=-1'),
                 (dict(logl0=float('inf')), b'glm: logl0='), (dict(logl0=float('nan')), b'glm: logl0=')]
    good = spec()
    for fn, what in ((lib.nnest_glm_pointwise, b'glm pointwise'), (lib.nnest_glm_predict, b'glm predict')):
        assert fn(None, p, st, pa, 4, 5, None) == E_ARG and b'glm is NULL' in err()
        for kw, words in bad_specs:
            s = spec(**kw)
            assert fn(ctypes.byref(s), p, st, pa, 4, s.D, None) == E_ARG and words in err(), kw
        assert fn(ctypes.byref(good), p, st, pa, 4, 4, None) == E_ARG and b"the likelihood's D=5 is not D=4" in err()
        assert fn(ctypes.byref(good), p, st, pa, -1, 5, None) == E_ARG and what + b': S=-1' in err()
        assert fn(ctypes.byref(good), p, st, pa, (1 << 30) + 1, 5, None) == E_ARG and what + b': S=1073741825' in err()
        for args in ((None, st, pa), (p, None, pa), (p, st, None)):
            for S in (0, 4):
                assert fn(ctypes.byref(good), args[0], args[1], args[2], S, 5, None) == E_ARG and what + b': NULL' in err()
    for name, a in guard.items():
        assert np.all(a == 0x5A), name
