"""Times nnest_amd.evaluation.chain_stats (the nnest_chain_stats kernels) on AR(1) chains x [C, T, D] made on the device: wall time
per call (torch events around the call, median of --reps) at the shapes of DESIGN.md's chain-statistics section.  Kernel device
times: run the same script under rocprofv3 --kernel-trace --stats (a run of its own).

    python tools/time_chain_stats.py [--reps 20] [--out profiles/chain_stats/time.json]
    python tools/time_chain_stats.py --config2 off|on|both     BASELINE config 2 (Rosenbrock-50, 1000 live points, 1000 chains,
                                                              NVP flow) with NestedSampler(chain_stats=False / True): wall time
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import evaluation  # noqa: E402


def ar1(C, T, D, rho, seed=0):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    x = torch.empty((C, T, D), dtype=torch.float32, device='cuda')
    x[:, 0] = torch.randn((C, D), generator=g, device='cuda')
    c = float(np.sqrt(1.0 - rho * rho))
    for j in range(1, T):
        x[:, j] = rho * x[:, j - 1] + c * torch.randn((C, D), generator=g, device='cuda')
    return x


def time_call(x, reps, **kw):
    r = evaluation.chain_stats(x, **kw)   # warm-up (and the result)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        evaluation.chain_stats(x, **kw)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), r


def config2(which):
    import tempfile
    import time
    from nnest_amd.likelihoods import Rosenbrock
    from nnest_amd.nested import NestedSampler
    rows = []
    for on in {'off': [False], 'on': [True], 'both': [False, True]}[which]:
        np.random.seed(0)
        torch.manual_seed(0)
        s = NestedSampler(50, Rosenbrock(50), transform=lambda x: 5.0 * x, log_dir=tempfile.mkdtemp(dir='/tmp'), num_live_points=1000,
                          log_level=30, flow='nvp', chain_stats=on)
        t0 = time.time()
        s.run(mcmc_num_chains=1000)
        torch.cuda.synchronize()
        row = dict(case='config 2 NestedSampler', chain_stats=on, wall_s=round(time.time() - t0, 3), logz=s.logz, niter=s.niter,
                   batches=s.num_batches)
        with open(os.path.join(s.logs['results'], 'results.csv')) as f:
            row['log_rows'] = sum(1 for _ in f) - 1
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config2', choices=('off', 'on', 'both'), default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-long', action='store_true')
    a = ap.parse_args()
    if a.config2:
        rows = config2(a.config2)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(rows, f, indent=1)
        return
    rows = []
    # rho 0.905: p_s ~ 0.905^s crosses 0.05 near lag 30
    cases = [('1000x251x50 every lag', (1000, 251, 50, 0.905), dict(all_lags=True)),
             ('1000x251x50 stop near 30', (1000, 251, 50, 0.905), {}),
             ('10x251x50 stop near 30', (10, 251, 50, 0.905), {}),
             ('1000x251x50 moments given', (1000, 251, 50, 0.905), dict(mean=np.zeros(50), std=np.ones(50)))]
    if not a.skip_long:
        cases.append(('1000x10001x50 stop near 30', (1000, 10001, 50, 0.905), {}))
    cache = {}
    for name, (C, T, D, rho), kw in cases:
        key = (C, T, D, rho)
        if key not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            cache[key] = ar1(C, T, D, rho)
        ms, r = time_call(cache[key], a.reps, **kw)
        row = dict(case=name, C=C, T=T, D=D, ms_per_call=round(ms, 4), stop_lag=r['stop_lag'], acceptance=r['acceptance'],
                   min_ess=float(np.min(r['ess'])), max_ess=float(np.max(r['ess'])))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
