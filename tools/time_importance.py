"""Developer diagnostic: the fused importance-sampling kernels (nnest_importance_evidence, nnest_spline_importance_evidence) against the
route composed from the calls of the same build, per case (x_dim, likelihood) and flow (NVP, spline), `num_samples` samples with no
per-sample outputs:
  fused:     HipNVP / HipSpline.importance_evidence in launches of 2^22 samples, the sums merged on the host;
  composed:  torch.randn -> .mcmc_steps(steps = 0) (x, lp and logL of every row written to memory) -> lp - logb and the max / exp /
             sum reductions in torch float64, in chunks of `--chunk` rows (default 2^20: M x (2 D + 3) words must fit).
The routes alternate in one process: after a warm-up of each, `reps` rounds, each timed by device events around work that ends in a
synchronise.  Printed per route: the mean, the standard deviation, the spread (min .. max) and evaluations per second.
   python tools/time_importance.py [--reps R] [--samples N] [--chunk C] [--out FILE] [x_dim like_id] ...
   (default: 50 0 and 20 1: Rosenbrock and GaussianMix; --out appends the report to FILE, e.g. profiles/importance/summary.txt)"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import _lib, flow  # noqa: E402
from nnest_amd.spline import HipSpline  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}
LAUNCH = 1 << 22


def timed(fn, seed):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn(seed)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main(argv):
    reps, out_path, M, chunk, nums = 5, None, 1 << 22, 1 << 20, []
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--out':
            out_path = next(it)
        elif a == '--samples':
            M = int(next(it))
        elif a == '--chunk':
            chunk = int(next(it))
        else:
            nums.append(int(a))
    nums = nums or [50, 0, 20, 1]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for D, like_id in zip(*[iter(nums)] * 2):
        std, mean = np.full(D, 0.5), np.zeros(D)
        x0 = np.random.RandomState(0).normal(size=(1000, D)).astype(np.float32) * 0.5
        for flow_name in ('nvp', 'spline'):
            net = flow.HipNVP(D, 16, 3, 1, seed=0) if flow_name == 'nvp' else HipSpline(D, 16, 3, seed=0)
            net.forward(x0)   # (the spline: sets the ActNorm layers from these points)
            kw = dict(t_std=std, t_mean=mean)
            logb_const = 0.5 * D * math.log(2.0 * math.pi)

            def fused(seed):
                parts = [net.importance_evidence(like_id, min(LAUNCH, M - first), seed=seed, sample_offset=first, **kw)['sums']
                         for first in range(0, M, LAUNCH)]
                return _lib.merge_importance([tuple(p.cpu().numpy()) for p in parts])   # (the copy is the synchronise)

            def composed(seed):
                torch.manual_seed(seed)
                parts = []
                for first in range(0, M, chunk):
                    z = torch.randn(min(chunk, M - first), D, device=net.device)
                    ev = net.mcmc_steps(like_id, z, 0, 0.1, **kw)
                    logw = ev['lp'] + 0.5 * (z.double() ** 2).sum(1) + logb_const
                    live = torch.isfinite(logw)
                    a = torch.where(live, logw, torch.full_like(logw, -math.inf)).max()
                    e = torch.where(live, torch.exp(logw - a), torch.zeros_like(logw))
                    parts.append(torch.stack([a, e.sum(), (e * e).sum(), live.double().sum()]))
                return _lib.merge_importance([tuple(p.cpu().numpy()) for p in parts])

            routes = {'fused': fused, 'composed': composed}
            say('x_dim %d, %s, %s flow, %d samples (fused: launches of %d; composed: chunks of %d)'
                % (D, NAMES.get(like_id, like_id), flow_name, M, min(LAUNCH, M), min(chunk, M)))
            ts, res = {n: [] for n in routes}, {}
            for name, fn in routes.items():   # warm-up: code objects, allocator
                timed(fn, 0)
            for k in range(reps):
                for name, fn in routes.items():
                    ms, res[name] = timed(fn, k + 1)
                    ts[name].append(ms)
            m = {}
            for name in routes:
                t = np.asarray(ts[name])
                m[name] = float(t.mean())
                r = _lib.importance_result(*res[name], M)
                say('  %-9s %9.3f ms (mean of %d; sd %.3f, min %.3f .. max %.3f), %.3g evaluations / s; logz_x %.3f, ESS %.1f'
                    % (name, m[name], len(t), float(t.std(ddof=1)) if len(t) > 1 else 0.0, float(t.min()), float(t.max()),
                       M / (1e-3 * m[name]), r['logz_x'], r['ess']))
            say('  composed / fused: %.2fx; memory: fused %d bytes of partials a launch, composed %d bytes a chunk (z, x, lp, logL)'
                % (m['composed'] / m['fused'], 3 * 8 * int(_lib.load().nnest_importance_groups(min(LAUNCH, M), net._IMPORTANCE_TILE)),
                   min(chunk, M) * (8 * D + 16)))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
