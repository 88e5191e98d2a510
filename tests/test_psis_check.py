"""CPU checks of Pareto-smoothed leave-one-out's float64 definition (nnest_amd/psis.py; include/nnest_hip.h nnest_glm_psis; DESIGN.md
3.19) against tests/psis_check.py's long-double restatement:
  1. the fit recovers a known shape on generalised-Pareto samples;
  2. the cutoff rule: a bin edge, at most M* draws below it, one bin more would be too many, ties never split, no tail for a
     constant row, no fit below 25 draws;
  3. the planted faults are caught by the comparison the GPU tests make;
  4. float64 against long double on the GPU tests' cases: the scale of their tolerance (psis_check.F64_VS_LD).

Measured: 4. at most 4.13e-12 (khat, logistic x_dim 33, n 70, S 25: a tail of five values), sigma 2.2e-15, elpd_psis 8.0e-15, psis_ess
3.0e-14; 1. means over 20 seeds 0.109 / 0.496 / 0.913 at k = 0.1 / 0.5 / 0.9 (sd 0.023 to 0.041)."""
import numpy as np
import pytest

from nnest_amd import psis
from tests import glm_check
from tests import glm_pointwise_check as pk
from tests import psis_check as pc


def terms_of(family, D, n, S, seed=3):
    return pc.host_terms(pc.case_data(family, D, n), pk.draws(S, D, seed))


# ---- 1. known k ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0.1, 0.5, 0.9])
def test_fit_recovers_a_known_shape(k):
    got = []
    for seed in range(20):
        u = np.random.RandomState(100 * seed + int(10 * k)).uniform(size=1500)
        x = np.sort(2.0 * np.expm1(-k * np.log1p(-u)) / k)
        khat = psis.gpd_fit(x)[2]
        assert abs(khat - k) <= 0.15, (seed, khat)
        got.append(khat)
    print('k = %.1f: mean khat over 20 seeds %.3f, sd %.3f' % (k, np.mean(got), np.std(got)))
    assert abs(np.mean(got) - k) <= 0.04


# ---- 2. the cutoff ------------------------------------------------------------------------------------------------------------------
def check_cutoff(l):
    out, tails = psis.psis_rows(l, return_tails=True)
    for i in range(l.shape[1]):
        col = l[np.isfinite(l[:, i]), i]
        d = np.max(-col) - (-col)
        c, M, target = out[i, psis.C], int(out[i, psis.M]), psis.tail_target(len(col))
        assert out[i, psis.M_STAR] == target and M <= target
        assert int(np.float64(c).view(np.uint64)) & ((1 << 40) - 1) == 0 and c >= 0.0
        assert M == int(np.sum(d < c)) == len(tails[i]) and np.all(tails[i] < c) and out[i, psis.N_BODY] == int(np.sum(d >= c))
        assert np.array_equal(tails[i], np.sort(d[d < c]))
        assert int(np.sum(d < pc.edge_of(pc.key_of(c) + 1))) > target   # (one bin more would be too many)
    return out


@pytest.mark.parametrize('family', glm_check.FAMILIES)
def test_cutoff_is_the_bin_edge_the_definition_names(family):
    for D, n, S in ((5, 17, 4001), (33, 3, 1003), (1, 4, 40000)):
        out = check_cutoff(terms_of(family, D, n, S))
        assert np.all(out[:, psis.M] >= out[:, psis.M_STAR] - 2) and np.all(out[:, psis.FLAG] == 0), out[:, psis.M]


def test_ties_are_never_split():
    l = np.repeat(terms_of('logistic', 5, 6, 800), 5, axis=0)
    out = check_cutoff(l)
    assert np.all(out[:, psis.M] % 5 == 0) and np.all(out[:, psis.N_BODY] % 5 == 0) and np.all(out[:, psis.M] > 0)


def test_a_constant_row_has_no_tail_and_small_runs_no_fit():
    l = np.full((400, 2), -0.75)
    out = psis.psis_rows(l)
    assert np.all(out[:, psis.M] == 0) and np.all(out[:, psis.C] == 0.0) and np.all(np.isposinf(out[:, psis.KHAT]))
    np.testing.assert_allclose(out[:, psis.ELPD], -0.75, rtol=0, atol=1e-15)
    for S in (1, 17, 24):
        l = terms_of('poisson', 5, 4, S)
        out = check_cutoff(l)
        plain = pk.derived(pk.stats(l))['elpd_isloo']
        assert np.all(out[:, psis.M] < 5) and np.all(np.isposinf(out[:, psis.KHAT])) and np.all(out[:, psis.FLAG] == psis.F_NOFIT)
        np.testing.assert_allclose(out[:, psis.ELPD], plain, rtol=0, atol=1e-13)
    out = check_cutoff(terms_of('poisson', 5, 4, 25))
    assert np.all(out[:, psis.M] == 5) and np.all(np.isfinite(out[:, psis.KHAT]))   # (the first size with a fit)
    # nothing live: the empty block
    out = psis.psis_rows(np.full((7, 2), np.nan))
    assert np.array_equal(out, np.stack([psis.empty_row()] * 2), equal_nan=True)
    assert np.array_equal(psis.psis_rows(np.zeros((0, 2))), out, equal_nan=True)


# ---- 3. planted faults -----------------------------------------------------------------------------------------------------------------
def test_planted_faults_are_caught():
    A, y, th = pc.outlier_case(0, S=4000)
    from nnest_amd.likelihoods import GLMData
    l = GLMData(A, y, family='logistic')._row_terms(th)[:, :3]
    want = pc.rows(l)
    assert max(pc.distance(psis.psis_rows(l), want).values()) <= pc.GPU_TOL
    assert want[0]['khat'] > 0.5
    bad = pc.rows(l, 'unregularised')
    assert pc.distance(pc.block_of(bad), want)['khat'] > 1e3 * pc.GPU_TOL
    bad = pc.rows(l, 'no_truncation')
    d = pc.distance(pc.block_of(bad), want)
    assert d['khat'] == 0.0 and d['elpd'] > 1e3 * pc.GPU_TOL and d['ess'] > 1e3 * pc.GPU_TOL
    bad = pc.rows(l, 'tail_bin')
    assert all(b['M'] > w['M'] and b['M'] > w['target'] and b['c'] > w['c'] for b, w in zip(bad, want))   # (the exact comparison)


def test_outlier_row_is_flagged_on_the_host_route():
    """the construction of the GPU front-end test, on route 'host': what that test asserts on the device holds here first"""
    from nnest_amd.evaluation import predictive_criteria
    from nnest_amd.likelihoods import GLMData
    A, y, th = pc.outlier_case(1)
    like = GLMData(A, y, family='logistic')
    before = like.pointwise(th, route='host')
    pw = like.pointwise(th, route='host', psis=True)
    assert sorted(set(pw) - set(before)) == ['elpd_psis', 'p_loo', 'pareto_k', 'psis_ess', 'psis_tail']
    assert all(np.array_equal(pw[k], before[k], equal_nan=True) for k in before)
    k = pw['pareto_k']
    assert k[0] > 0.5 and np.all(k[1:] < 0.5) and np.all(pw['psis_ess'] <= pw['n_live'])
    assert np.max(np.abs(pw['elpd_psis'] - pw['elpd_isloo'])[k < 0.5]) <= 0.01
    crit = predictive_criteria(like, th, route='host', psis=True)
    assert crit['n_pareto_k_bad'] >= 1 and crit['max_pareto_k'] == k[0] and abs(crit['p_loo'] - np.sum(pw['p_loo'])) < 1e-12
    assert 'elpd_psis' not in predictive_criteria(like, th, route='host')
    with pytest.raises(ValueError, match='thin'):
        like.pointwise(np.zeros(((1 << 20) + 1, 1)), route='host', psis=True)
    assert like.log_lik(th[:50], route='host').shape == (50, 30)


# ---- 4. float64 against long double ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', glm_check.FAMILIES)
def test_float64_against_long_double_on_the_gpu_cases(family):
    worst = dict.fromkeys(pc.QUANTITIES, 0.0)
    for fam, D, n, S, seed in pc.gpu_cases():
        if fam != family:
            continue
        l = pc.host_terms(pc.case_data(fam, D, n), pk.draws(S, D, seed))
        got, tails = psis.psis_rows(l, return_tails=True)
        want = pc.rows(l)
        for i, w in enumerate(want):   # (the selection: two codes, the same bits)
            assert got[i, psis.C] == w['c'] and got[i, psis.M] == w['M'] and got[i, psis.N_BODY] == w['n_body']
            assert np.array_equal(tails[i], w['tail'])
            assert abs(got[i, psis.B] - w['B']) <= (S + 4) * 2.0 ** -52 * w['B'] and abs(got[i, psis.B2] - w['B2']) <= (S + 4) * 2.0 ** -52 * w['B2']
        for k, v in pc.distance(got, want).items():
            worst[k] = max(worst[k], v)
    print('float64 against long double, %s: %s' % (family, ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= pc.F64_VS_LD
