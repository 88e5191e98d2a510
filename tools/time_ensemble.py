"""Developer diagnostic: the ensemble sampler's two routes (nnest_ensemble_steps, the fused kernel; nnest_ensemble_rounds_*, the
round driver with the device likelihood) on the same flow, walkers and draws -- ms per launch of `steps` steps, us per step.
   python tools/time_ensemble.py [x_dim like_id walkers steps] ...   (default: 50 0 1000 250 and 20 1 1000 250)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import flow  # noqa: E402
from nnest_amd.ensemble_rounds import ensemble_rounds  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}
args = [int(a) for a in sys.argv[1:]] or [50, 0, 1000, 250, 20, 1, 1000, 250]
for D, like_id, C, S in zip(*[iter(args)] * 4):
    nvp = flow.HipNVP(D, 16, 3, 1, seed=0)
    z0 = torch.from_numpy(np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5).cuda()
    kw = dict(t_std=np.full(D, 0.5), t_mean=np.zeros(D), lo=np.full(D, -5.0), hi=np.full(D, 5.0))

    def fused(seed):
        return nvp.ensemble_steps(like_id, z0, S, seed=seed, **kw)

    def rounds(seed):
        return ensemble_rounds(nvp, z0, S, like_id=like_id, seed=seed, **kw)

    print('x_dim %d, %s, %d walkers x %d steps (fused route: at most %d walkers resident)' % (D, NAMES.get(like_id, like_id), C, S,
                                                                                            nvp.ensemble_max_walkers(like_id)))
    res = {}
    for name, fn, reps in (('fused', fused, 5), ('rounds', rounds, 3)):
        ts = []
        for k in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(k)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts[1:]))
        res[name] = ms
        n_acc = out['n_accept'] if name == 'fused' else out[0].n_accept
        print('  %-6s %9.3f ms per launch (median of %d), %8.2f us per step, acceptance %.3f' % (
            name, ms, reps, 1e3 * ms / S, float(n_acc.sum()) / (C * S)))
    print('  rounds / fused: %.1fx' % (res['rounds'] / res['fused']))
