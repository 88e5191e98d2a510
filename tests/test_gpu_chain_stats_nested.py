"""GPU: NestedSampler(chain_stats=True) writes the reference's acceptance, min ESS, max ESS and jump distance of the batch that
supplied each logged point into results.csv (nested.py:446-456), computed with the mean and std of the live points; every row
equals the float64 restatement (tests/chain_stats_check.py) on that batch's history; the native and the Python loops write the same
file byte for byte; and the run itself -- dead points, log Z, final.csv -- is the one that mcmc_history=True gives without the
statistics."""
import csv
import os

import numpy as np
import pytest
import torch

from nnest_amd.likelihoods import Rosenbrock
from nnest_amd.nested import NestedSampler
from tests import chain_stats_check as chk

pytestmark = pytest.mark.gpu

CASES = {'cfg1_rosenbrock_d2': dict(D=2, N=150, C=20, max_iters=1200),
         'fused_rosenbrock_d5': dict(D=5, N=200, C=50, max_iters=1200)}


def _run(tmp, case, native=True, chain_stats=True, mcmc_history=False, capture=None):
    c = CASES[case]
    np.random.seed(5)
    torch.manual_seed(5)
    s = NestedSampler(c['D'], Rosenbrock(c['D']), transform=lambda x: 5.0 * x, log_dir=str(tmp), num_live_points=c['N'], log_level=30,
                      flow='nvp', native_loop=native, chain_stats=chain_stats, mcmc_history=mcmc_history)
    assert s._fused_like_id is not None
    if capture is not None:
        orig = s._batch_chain_stats

        def spy(active_u, C, primary):
            h = s._chain_hist
            h = h.cpu().numpy() if torch.is_tensor(h) else np.asarray(h)
            capture.append((h.copy(), np.array(active_u, dtype=np.float64)))
            return orig(active_u, C, primary)
        s._batch_chain_stats = spy
    s.run(train_iters=100, mcmc_num_chains=c['C'], log_interval=50, max_iters=c['max_iters'])
    return s


def _rows(s):
    with open(os.path.join(s.logs['results'], 'results.csv')) as f:
        return list(csv.reader(f))[1:]


@pytest.mark.parametrize('case', sorted(CASES))
def test_rows_equal_the_restatement_on_the_batch_history(tmp_path, case):
    cap = []
    s = _run(tmp_path, case, capture=cap)
    rows = _rows(s)
    assert len(rows) == len(cap) >= 3
    for row, (h, active_u) in zip(rows, cap):
        C, T, D = h.shape
        assert C == CASES[case]['C'] and D == CASES[case]['D'] and T >= 2
        x = h.astype(np.float64)
        mu, sd = active_u.mean(axis=0), active_u.std(axis=0)
        ess, _ = chk.ess_from_p(chk.autocorr(x, mu, sd), T)
        acc, mn, mx, jump = (float(v) for v in row[1:5])
        assert acc == chk.acceptance(x)
        np.testing.assert_allclose([mn, mx], [ess.min(), ess.max()], rtol=1e-5)
        np.testing.assert_allclose(jump, chk.jump(x), rtol=1e-5)


@pytest.mark.parametrize('case', sorted(CASES))
def test_native_and_python_loops_write_the_same_results(tmp_path, case):
    a = _run(tmp_path / 'native', case, native=True)
    b = _run(tmp_path / 'python', case, native=False)
    fa = open(os.path.join(a.logs['results'], 'results.csv'), 'rb').read()
    fb = open(os.path.join(b.logs['results'], 'results.csv'), 'rb').read()
    assert fa == fb
    assert all(r[2] != 'nan' for r in _rows(a))


@pytest.mark.parametrize('case', sorted(CASES))
def test_statistics_leave_the_run_unchanged(tmp_path, case):
    a = _run(tmp_path / 'stats', case, chain_stats=True, mcmc_history=False)
    b = _run(tmp_path / 'history', case, chain_stats=False, mcmc_history=True)
    assert a.niter == b.niter and a.ncall == b.ncall and a.logz == b.logz and a.h == b.h
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.loglikes, b.loglikes) and np.array_equal(a.weights, b.weights)
    fa = open(os.path.join(a.logs['results'], 'final.csv'), 'rb').read()
    fb = open(os.path.join(b.logs['results'], 'final.csv'), 'rb').read()
    assert fa == fb
    ra, rb = _rows(a), _rows(b)
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):   # every column but the four statistics (nan without them)
        assert x[0] == y[0] and x[5:] == y[5:]
        assert y[2] == 'nan' and x[2] != 'nan'
