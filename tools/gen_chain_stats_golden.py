"""Writes tests/golden/chain_stats_ref.npz: chain batches x [C, T, D] (float32) and what the reference's own
nnest.utils.evaluation computes on them (float64 arithmetic on the float32 values; mean / std as Sampler._chain_stats forms them,
nnest/sampler.py:474-480).  Needs NNEST_REFERENCE (oracle/_refimport.py).  Every case keeps its lag autocorrelations at least
1e-6 away from the 0.05 threshold of the ESS sum; the generator tries seeds until that holds and the case shows what it is for.

    NNEST_REFERENCE=<checkout> python tools/gen_chain_stats_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle._refimport import import_reference  # noqa: E402
import chain_stats_check as chk  # noqa: E402

MARGIN = 1e-6


def ar1(rng, C, T, D, rho, scale=1.0):
    x = np.zeros((C, T, D))
    x[:, 0] = rng.standard_normal((C, D)) * scale
    for j in range(1, T):
        x[:, j] = rho * x[:, j - 1] + np.sqrt(1 - rho ** 2) * scale * rng.standard_normal((C, D))
    return x


def with_rejections(rng, x, rate):
    x = x.copy()
    for i in range(x.shape[0]):
        for j in range(1, x.shape[1]):
            if rng.uniform() < rate:
                x[i, j] = x[i, j - 1]
    return x


def case_rejected(rng):
    return with_rejections(rng, ar1(rng, 6, 40, 3, 0.6), 0.4), None, None


def case_one_coord(rng):
    x = with_rejections(rng, ar1(rng, 3, 12, 4, 0.3), 0.3)
    x[1, 5] = x[1, 4]
    x[1, 5, 2] += 0.25          # equal in every coordinate but one: an accepted step
    x[2, 7] = x[2, 6]
    x[2, 7, 0] = np.nextafter(np.float32(x[2, 7, 0]), np.float32(np.inf))
    return x, None, None


def case_ar1_dip(rng):
    # a slowly decaying AR(1) beside a dimension whose autocorrelation oscillates (AR(2), complex roots): it falls below 0.05
    # at some lag and rises above it again while the slow dimension keeps the sum going
    C, T = 4, 200
    slow = ar1(rng, C, T, 1, 0.97)
    osc = np.zeros((C, T))
    e = rng.standard_normal((C, T))
    for j in range(2, T):
        osc[:, j] = 1.6 * osc[:, j - 1] - 0.85 * osc[:, j - 2] + e[:, j]
    return np.concatenate([slow, osc[:, :, None] / osc.std()], axis=2), None, None


def case_no_stop(rng):
    return ar1(rng, 3, 30, 2, 0.995, scale=8.0), None, None


def case_c1(rng):
    return ar1(rng, 1, 50, 2, 0.8), None, None


def case_t2(rng):
    x = rng.standard_normal((5, 2, 3))
    x[1, 1] = x[1, 0]
    return x, None, None


def case_scales(rng):
    return ar1(rng, 5, 60, 3, 0.7) * np.array([1e-2, 1.0, 1e2]), None, None


def case_given(rng):
    x = ar1(rng, 4, 80, 3, 0.8) + np.array([0.5, -1.0, 2.0])
    return x, np.array([0.4, -1.1, 2.2]), np.array([0.9, 1.3, 1.1])


CASES = [('rejected', case_rejected), ('one_coord', case_one_coord), ('ar1_dip', case_ar1_dip), ('no_stop', case_no_stop),
         ('c1', case_c1), ('t2', case_t2), ('scales', case_scales), ('given', case_given)]


def shows(name, x, r):
    T = x.shape[1]
    p = r['p']
    stop = r['stop_lag']
    if name == 'ar1_dip':   # some dimension below 0.05 at a lag before the stop and above it again later
        below = p[:stop - 1] <= 0.05
        return any(below[:, d].any() and (~below[np.argmax(below[:, d]):, d]).any() for d in range(x.shape[2])) and stop > 10
    if name == 'no_stop':
        return stop == T
    if name == 'rejected':
        return r['acceptance'] < 0.8
    return True


def main():
    import_reference()
    from nnest.utils import evaluation as ev
    out = {}
    for name, make in CASES:
        for seed in range(1000):
            rng = np.random.RandomState(seed)
            x, mean, std = make(rng)
            x = x.astype(np.float32)
            x64 = x.astype(np.float64)
            r = chk.stats(x, mean, std)
            p = r['p']
            if np.min(np.abs(p - 0.05)) < MARGIN or not shows(name, x, r):
                continue
            mu = np.mean(np.reshape(x64, (-1, x.shape[2])), axis=0) if mean is None else mean
            sd = np.std(np.reshape(x64, (-1, x.shape[2])), axis=0) if std is None else std
            out[name + '_x'] = x
            if mean is not None:
                out[name + '_mean'] = mean
                out[name + '_std'] = std
            out[name + '_acceptance'] = np.float64(ev.acceptance_rate(x64))
            out[name + '_jump'] = np.float64(ev.mean_jump_distance(x64))
            out[name + '_ess'] = ev.effective_sample_size(x64, mu, sd)
            out[name + '_p'] = np.array([ev.auto_correlation_time(x64, s, mu, sd) for s in range(1, x.shape[1])])
            if x.shape[0] > 1:
                out[name + '_rhat'] = ev.gelman_rubin_diagnostic(x64)
            print('%-10s seed %3d  C=%d T=%d D=%d  acceptance %.4f  ESS %s  stop %d' % (name, seed, x.shape[0], x.shape[1], x.shape[2],
                  out[name + '_acceptance'], np.round(out[name + '_ess'], 3), r['stop_lag']))
            break
        else:
            raise SystemExit('no seed gives case %s' % name)
    out['cases'] = np.array([n for n, _ in CASES])
    path = os.path.join(ROOT, 'tests', 'golden', 'chain_stats_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
