"""Developer diagnostic: the ensemble sampler's two routes through the SPLINE flow on the same HipSpline, walkers and draws -- the fused
kernel (nnest_spline_ensemble_steps) and the round driver (nnest_ensemble_rounds_* around HipSpline.inverse and the device
likelihood) -- ms per launch of `steps` steps and us per step.  The two routes alternate in one process: after a warm-up launch of
each, `reps` pairs (fused, rounds), each timed by a host clock around work that ends in a device synchronise.  Printed per route:
the mean, the standard deviation over the repetitions and the standard error of the mean; the difference of the means counts as
real when it exceeds the two standard errors combined.
   python tools/time_spline_ensemble.py [--reps R] [--out FILE] [x_dim like_id walkers steps] ...
   (default: 50 0 1000 250 and 20 1 1000 250; --out appends the report to FILE, e.g. profiles/ensemble_spline/summary.txt)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd.ensemble_rounds import ensemble_rounds  # noqa: E402
from nnest_amd.spline import HipSpline  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}


def timed(fn, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(seed)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main(argv):
    reps, out_path, nums = 7, None, []
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--out':
            out_path = next(it)
        else:
            nums.append(int(a))
    nums = nums or [50, 0, 1000, 250, 20, 1, 1000, 250]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for D, like_id, C, S in zip(*[iter(nums)] * 4):
        sp = HipSpline(D, 16, 3, seed=0)
        x0 = np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5
        z0, _ = sp.forward(x0)   # (sets the ActNorm layers from the start points)
        z0 = z0.contiguous()
        kw = dict(t_std=np.full(D, 0.5), t_mean=np.zeros(D), lo=np.full(D, -5.0), hi=np.full(D, 5.0))
        routes = {'fused': lambda seed: sp.ensemble_steps(like_id, z0, S, seed=seed, **kw),
                  'rounds': lambda seed: ensemble_rounds(sp, z0, S, like_id=like_id, seed=seed, **kw)}
        say('x_dim %d, %s, %d walkers x %d steps (fused route: at most %d walkers resident)'
            % (D, NAMES.get(like_id, like_id), C, S, sp.ensemble_max_walkers(like_id)))
        ts, acc = {n: [] for n in routes}, {}
        for name, fn in routes.items():   # warm-up: code objects, allocator
            timed(fn, 0)
        for k in range(reps):
            for name, fn in routes.items():
                ms, out = timed(fn, k + 1)
                ts[name].append(ms)
                n_acc = out['n_accept'] if name == 'fused' else out[0].n_accept
                acc[name] = float(n_acc.sum()) / (C * S)
        mean, sem = {}, {}
        for name in routes:
            t = np.asarray(ts[name])
            mean[name], sem[name] = float(t.mean()), float(t.std(ddof=1) / np.sqrt(len(t)))
            say('  %-6s %9.3f ms per launch (mean of %d; sd %.3f, se %.3f; min %.3f max %.3f), %8.2f us per step, acceptance %.3f'
                % (name, mean[name], len(t), float(t.std(ddof=1)), sem[name], float(t.min()), float(t.max()), 1e3 * mean[name] / S, acc[name]))
        diff, spread = mean['rounds'] - mean['fused'], float(np.hypot(sem['rounds'], sem['fused']))
        say('  rounds - fused: %.3f ms (spread of the two means %.3f ms); rounds / fused: %.2fx' % (diff, spread, mean['rounds'] / mean['fused']))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
