"""Developer measurement for EnsembleSampler.bootstrap's x-space run: the fused kernel (nnest_ensemble_x_steps)
against the round driver on an identity-flow shim -- the only x-space route before the kernel, unchanged since -- on the same
walkers and draws, and the autocorrelation kernel (nnest_chain_autocorr) on the run's history.  One warm-up launch, then `reps`
timed launches with the device idle at both ends; median, minimum and maximum in ms per launch.
   python scripts/measure_bootstrap.py [x_dim like_id walkers steps] ...   (default: 50 0 1000 250 and 20 1 1000 250)
The figures quoted in DESIGN.md and README.md are in profiles/bootstrap/summary.txt."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import flow  # noqa: E402
from nnest_amd.ensemble_rounds import ensemble_rounds  # noqa: E402
from nnest_amd.evaluation import autocorr_function  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}


class IdentityShim(object):
    """what a caller of the round driver had to write for an x-space run before IdentityFlow"""

    def __init__(self, device):
        self.device = device

    def inverse(self, z):
        return z, torch.zeros(z.shape[0], dtype=torch.float32, device=z.device)


def timed(fn, reps):
    ts, out = [], None
    for k in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(k)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = ts[1:]
    return float(np.median(ts)), min(ts), max(ts), out


args = [int(a) for a in sys.argv[1:]] or [50, 0, 1000, 250, 20, 1, 1000, 250]
for D, like_id, C, S in zip(*[iter(args)] * 4):
    x0 = torch.from_numpy(np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5).cuda()
    kw = dict(lo=np.full(D, -5.0), hi=np.full(D, 5.0))
    shim = IdentityShim(x0.device)
    print('x_dim %d, %s, %d walkers x %d steps, T = identity, box [-5, 5] (fused route: at most %d walkers resident)' % (
        D, NAMES.get(like_id, like_id), C, S, flow.ensemble_x_max_walkers(D, like_id)))
    res = {}
    for name, fn, reps in (('fused', lambda k: flow.ensemble_x_steps(like_id, x0, S, seed=k, **kw), 9),
                           ('rounds', lambda k: ensemble_rounds(shim, x0, S, like_id=like_id, seed=k, **kw), 5)):
        med, lo, hi, out = timed(fn, reps)
        res[name] = med
        n_acc = out['n_accept'] if name == 'fused' else out[0].n_accept
        print('  %-6s %9.3f ms per launch (median of %d; min %.3f, max %.3f), %8.2f us per step, acceptance %.3f' % (
            name, med, reps, lo, hi, 1e3 * med / S, float(n_acc.sum()) / (C * S)))
        hist = out['hist_x'] if name == 'fused' else out[1]['hist_z']
    print('  rounds / fused: %.1fx' % (res['rounds'] / res['fused']))
    med, lo, hi, _ = timed(lambda k: autocorr_function(hist), 5)
    print('  autocorrelation function of the [%d, %d, %d] history: %.3f ms (median of 5; min %.3f, max %.3f)' % (C, S, D, med, lo, hi))
D, C, S = 50, 100, 1000
x = torch.from_numpy(np.random.RandomState(1).normal(size=(C, S, D)).astype(np.float32)).cuda()
med, lo, hi, _ = timed(lambda k: autocorr_function(x), 5)
print('autocorrelation function of 100 walkers x 1000 steps x 50 dims (2.5e9 float64 FMAs): %.3f ms (median of 5; min %.3f, max %.3f)'
      % (med, lo, hi))
