"""CPU checks of the invariance harness (tests/slice_invariance.py) that the GPU tests of the slice proposal rely on: its statistics
accept exact samples and a correct slice update, and they reject the stepping-out rule that caps each side separately (Neal 2003,
sec. 4.1: not reversible once the cap binds) at the walker counts the GPU tests use, while a cap that never binds passes."""
import numpy as np
import pytest

from tests import slice_invariance as si


def run(rule, max_stepout, width=0.1, D=2, N=200000, seed=0):
    rng = np.random.RandomState(seed)
    x0 = si.uniform_on(rng, N, D)
    fresh = si.uniform_on(rng, N, D)
    x1 = si.slice_update(rng, x0, width, max_stepout, rule=rule)
    x = x1
    for _ in range(4):
        x = si.slice_update(rng, x, width, max_stepout, rule=rule)
    p = {}
    for tag, pv in (('S1', si.stationarity_pvalues(x1, fresh)), ('S5', si.stationarity_pvalues(x, fresh)),
                    ('ex', si.exchangeability_pvalues(x0, x1))):
        p.update({'%s:%s' % (tag, k): v for k, v in pv.items()})
    return p


def test_exact_samples_pass():
    rng = np.random.RandomState(3)
    a, b, c = (si.uniform_on(rng, 100000, 3, lambda x: np.sum(x * x, axis=1) < 0.8) for _ in range(3))
    assert np.all(np.sum(a * a, axis=1) < 0.8) and a.shape == (100000, 3)
    si.assert_invariant(si.stationarity_pvalues(a, b))
    si.assert_invariant(si.exchangeability_pvalues(a, c))


def test_a_biased_sample_fails():
    rng = np.random.RandomState(4)
    a, b = si.uniform_on(rng, 200000, 2), si.uniform_on(rng, 200000, 2)
    a[:20000] *= 0.8   # 10 % of the walkers pulled in from the faces by 20 %
    with pytest.raises(AssertionError):
        si.assert_invariant(si.stationarity_pvalues(a, b))
    s = a[:, 0].copy()
    s1 = s + 0.01 * (np.abs(s) < 0.5)   # a drift in one direction: not exchangeable
    with pytest.raises(AssertionError):
        si.assert_invariant(si.exchangeability_pvalues(a, np.stack([s1, a[:, 1]], 1)))


@pytest.mark.parametrize('max_stepout,width', [(1, 0.1), (2, 0.05)])
def test_the_statistics_see_a_per_side_cap(max_stepout, width):
    """a binding budget: the kernels' rule passes, the per-side cap fails (the GPU tests' binding setting, at a fifth of their N)"""
    si.assert_invariant(run('budget', max_stepout, width))
    p = run('cap', max_stepout, width)
    assert si.min_corrected_p(p) < si.ALPHA, si.min_corrected_p(p)


def test_a_cap_that_never_binds_passes_with_either_rule():
    for rule in ('budget', 'cap'):
        si.assert_invariant(run(rule, 1000, 0.1, N=100000))


def test_stepout_split():
    v = np.arange(1 << 24, dtype=np.float64) / (1 << 24)
    for m in (0, 1, 8, 1000):
        J, K = si.stepout_split(v, m)
        assert np.all(J + K == 2 * m) and J.min() == 0 and J.max() == 2 * m
        counts = np.bincount(J, minlength=2 * m + 1)   # J uniform on 0..B: every value as often as 2^24 / (B + 1) allows
        assert counts.max() - counts.min() <= 1
