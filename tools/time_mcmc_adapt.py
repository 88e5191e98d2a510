"""Developer diagnostic: the adaptive-walk kernels (nnest_mcmc_adapt_steps, nnest_spline_mcmc_adapt_steps) against the mixed-walk kernels
they generalise, per case (x_dim, likelihood) and flow (NVP, spline), `walkers` chains x `steps` steps, on the same flow (at its
initialisation: nothing is trained) and start, with the histories written, every step local (global_every = 0):
  mixed      nnest_mcmc_mixed_steps / nnest_spline_mcmc_mixed_steps -- units this tree does not touch: the parent commit's kernels;
  adapt off  the adaptive entry with adapt_steps = 0 and no step_in: the same run bit for bit (checked here), so the difference is
             the price of carrying the step per walker;
  adapt on   adapt_steps = steps: every step moves the walkers' steps (hist_step is written too).
The routes alternate in one process: after a warm-up of each, `reps` rounds, each launch timed by a host clock around work that
ends in a device synchronise.  Printed per route: the mean, the standard deviation and the standard error of the mean, and the
acceptance; then, per case and flow, what the adaptation is for: the acceptance and evaluation.mean_jump_distance (in x) of the
second half of the run at the fixed step 2 / sqrt(x_dim) and with the step adapted over the first half.  There is no pass/fail
ratio: the figures are recorded.
   python tools/time_mcmc_adapt.py [--reps R] [--out FILE] [x_dim like_id walkers steps] ...
   (default: --reps 20, 50 0 1000 250 and 20 1 1000 250: Rosenbrock and GaussianMix; --out appends the report to FILE, e.g.
   profiles/mcmc_adapt/summary.txt)"""
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnest_amd  # noqa: E402
from nnest_amd import _lib, evaluation, likelihoods  # noqa: E402

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


def entry(net, which, like_id, z0, S, step, t_std, t_mean, seed, adapt_steps=0):
    """the mixed or the adaptive entry itself at global_every = 0 (mcmc_steps keeps that on the existing entries)"""
    dev = z0.device
    C, D = z0.shape
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64), logl=torch.empty(C, **f64),
               hist_z=torch.empty(C, S, D, **f32), hist_x=torch.empty(C, S, D, **f32), hist_logl=torch.empty(C, S, **f64),
               n_accept=torch.empty(C, dtype=torch.int32, device=dev), n_accept_global=torch.empty(C, dtype=torch.int32, device=dev))
    more = ()
    if which == 'mcmc_adapt':
        out.update(step=torch.empty(C, **f64), hist_step=torch.empty(C, S, **f64))
        more = (None, _lib.ptr(out['step']), _lib.ptr(out['hist_step']), ctypes.c_uint32(adapt_steps), ctypes.c_double(1.0),
                ctypes.c_double(0.234))
    lk = _lib.like_spec(like_id, 1.0, None)
    with torch.cuda.device(dev):
        _lib.check(net._sym[which](
            net._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), None, None, _lib.ptr(z0), None, None, _lib.ptr(out['z']),
            _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']), _lib.ptr(out['hist_z']), _lib.ptr(out['hist_x']),
            _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, S, ctypes.c_float(step), 0, int(seed), 0, ctypes.c_double(1.0), 0,
            _lib.ptr(out['n_accept_global']), *more, _lib.current_stream(dev)))
    return out


def main(argv):
    reps, out_path, nums = 20, None, []
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
            routes = {'mixed': lambda seed: entry(net, 'mcmc_mixed', like_id, z0, S, step, t_std, t_mean, seed),
                      'adapt off': lambda seed: entry(net, 'mcmc_adapt', like_id, z0, S, step, t_std, t_mean, seed),
                      'adapt on': lambda seed: entry(net, 'mcmc_adapt', like_id, z0, S, step, t_std, t_mean, seed, adapt_steps=S)}
            ts, acc = {n: [] for n in routes}, {}
            for name, fn in routes.items():   # warm-up: code objects, allocator
                timed(fn, 0)
            same = all(torch.equal(routes['mixed'](3)[key], routes['adapt off'](3)[key]) for key in ('z', 'x', 'lp', 'logl', 'hist_z', 'n_accept'))
            say('  adapt off against mixed on seed 3: %s' % ('bit-identical' if same else 'DIFFERENT'))
            for r in range(reps):
                for name, fn in routes.items():
                    ms, out = timed(fn, r + 1)
                    ts[name].append(ms)
                    acc[name] = float(out['n_accept'].sum()) / (C * S)
            m = {}
            for name in routes:
                m[name], sd, se = stats(ts[name])
                say('  kernel %-10s %9.3f ms per launch (mean of %d; sd %.3f, se %.3f), %8.2f us per step, acceptance %.3f'
                    % (name, m[name], len(ts[name]), sd, se, 1e3 * m[name] / S, acc[name]))
            say('  adapt off / mixed: %.3fx; adapt on / mixed: %.3fx' % (m['adapt off'] / m['mixed'], m['adapt on'] / m['mixed']))
            # what it is for: the second half of the run at the fixed step and with the step adapted over the first half
            half = S // 2
            kw = dict(seed=1, t_std=t_std, t_mean=t_mean)
            for name, more in (('fixed step', {}), ('adapted', dict(adapt_steps=half))):
                a = net.mcmc_steps(like_id, z0, half, step, history=False, **more, **kw)
                b = net.mcmc_steps(like_id, a['z'], S - half, step, lp=a['lp'], logl=a['logl'], step0=half,
                                   **(dict(more, step_in=a['step']) if more else {}), **kw)
                tx = torch.cat([a['x'][:, None], b['hist_x']], 1).double().cpu().numpy() * 0.5
                say('  steps %d .. %d, %-10s acceptance %.4f, mean_jump_distance %.5f%s' % (
                    half, S - 1, name + ':', float(b['n_accept'].sum()) / (C * (S - half)), float(np.mean(evaluation.mean_jump_distance(tx))),
                    '' if not more else ', steps %.4g .. %.4g (geometric mean %.4g)' % (
                        float(b['step'].min()), float(b['step'].max()), float(torch.exp(torch.log(b['step']).mean())))))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
