"""Developer diagnostic: the mixed-walk kernels (nnest_mcmc_mixed_steps, nnest_spline_mcmc_mixed_steps) against the random-walk kernels
they generalise, per case (x_dim, likelihood) and flow (NVP, spline), `walkers` chains x `steps` steps, on the same flow (at its
initialisation: nothing is trained) and start, with the histories written:
  walk       nnest_mcmc_steps / nnest_spline_mcmc_steps -- units this tree does not touch: the parent commit's kernels;
  mixed k=0  the mixed entry with every step local: the same run bit for bit (checked here), so the difference is the price of the
             generality -- beta and the schedule as arguments, the two counters;
  mixed k=10 one global step in ten;
  mixed k=1  every step global.
The routes alternate in one process: after a warm-up of each, `reps` rounds, each launch timed by a host clock around work that
ends in a device synchronise.  Printed per route: the mean, the standard deviation and the standard error of the mean, the
acceptance and, of the global steps, the global acceptance (of an UNTRAINED flow here: a figure of the set-up, not of the move).
   python tools/time_mcmc_mixed.py [--reps R] [--out FILE] [x_dim like_id walkers steps] ...
   (default: 50 0 1000 250 and 20 1 1000 250: Rosenbrock and GaussianMix; --out appends the report to FILE, e.g.
   profiles/mcmc_mixed/summary.txt)"""
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnest_amd  # noqa: E402
from nnest_amd import _lib, likelihoods  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}
LIKES = {0: likelihoods.Rosenbrock, 1: likelihoods.GaussianMix}


def timed(fn, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(seed)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def stats(t):
    t = np.asarray(t)
    sd = float(t.std(ddof=1)) if len(t) > 1 else 0.0
    return float(t.mean()), sd, sd / np.sqrt(len(t))


def mixed_entry(net, like_id, z0, S, step, k, t_std, t_mean, seed):
    """the mixed entry itself at any global_every, 0 included (mcmc_steps keeps global_every = 0 on the existing entries)"""
    dev = z0.device
    C, D = z0.shape
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64), logl=torch.empty(C, **f64),
               hist_z=torch.empty(C, S, D, **f32), hist_x=torch.empty(C, S, D, **f32), hist_logl=torch.empty(C, S, **f64),
               n_accept=torch.empty(C, dtype=torch.int32, device=dev), n_accept_global=torch.empty(C, dtype=torch.int32, device=dev))
    lk = _lib.like_spec(like_id, 1.0, None)
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc_mixed'](
            net._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), None, None, _lib.ptr(z0), None, None, _lib.ptr(out['z']),
            _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']), _lib.ptr(out['hist_z']), _lib.ptr(out['hist_x']),
            _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, S, ctypes.c_float(step), 0, int(seed), 0, ctypes.c_double(1.0), int(k),
            _lib.ptr(out['n_accept_global']), _lib.current_stream(dev)))
    return out


def main(argv):
    reps, out_path, nums = 10, None, []
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
    tmp = tempfile.mkdtemp()
    for D, like_id, C, S in zip(*[iter(nums)] * 4):
        step = 2.0 / np.sqrt(D)
        x0 = np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5
        for flow_name in ('nvp', 'spline'):
            s = nnest_amd.MCMCSampler(D, LIKES[like_id](D), log_dir=tmp, log_level=30, flow=flow_name)
            net = s.trainer.netG
            z0, _ = net.forward(x0)   # (the spline: sets the ActNorm layers from the start points)
            z0 = z0.contiguous()
            t_std = torch.full((D,), 0.5, dtype=torch.float32, device=z0.device)
            t_mean = torch.zeros(D, dtype=torch.float32, device=z0.device)
            say('x_dim %d, %s, %s flow, %d chains x %d steps, step %.3f' % (D, NAMES.get(like_id, like_id), flow_name, C, S, step))
            routes = {'walk': lambda seed: net.mcmc_steps(like_id, z0, S, step, seed=seed, t_std=t_std, t_mean=t_mean)}
            for k in (0, 10, 1):
                routes['mixed k=%d' % k] = (lambda k: lambda seed: mixed_entry(net, like_id, z0, S, step, k, t_std, t_mean, seed))(k)
            ts, acc, accg = {n: [] for n in routes}, {}, {}
            for name, fn in routes.items():   # warm-up: code objects, allocator
                timed(fn, 0)
            same = all(torch.equal(routes['walk'](3)[key], routes['mixed k=0'](3)[key]) for key in ('z', 'x', 'lp', 'logl', 'hist_z', 'n_accept'))
            say('  mixed k=0 against walk on seed 3: %s' % ('bit-identical' if same else 'DIFFERENT'))
            for r in range(reps):
                for name, fn in routes.items():
                    ms, out = timed(fn, r + 1)
                    ts[name].append(ms)
                    acc[name] = float(out['n_accept'].sum()) / (C * S)
                    k = int(name.split('=')[1]) if '=' in name else 0
                    accg[name] = float(out['n_accept_global'].sum()) / (C * (S // k)) if k else None
            m = {}
            for name in routes:
                m[name], sd, se = stats(ts[name])
                say('  kernel %-10s %9.3f ms per launch (mean of %d; sd %.3f, se %.3f), %8.2f us per step, acceptance %.3f%s'
                    % (name, m[name], len(ts[name]), sd, se, 1e3 * m[name] / S, acc[name],
                       '' if accg[name] is None else ', global acceptance %.4f' % accg[name]))
            say('  mixed k=0 / walk: %.3fx; k=10 / walk: %.3fx; k=1 / walk: %.3fx'
                % (m['mixed k=0'] / m['walk'], m['mixed k=10'] / m['walk'], m['mixed k=1'] / m['walk']))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
