"""Developer diagnostic: the kernels of the Gaussian likelihood from user data (nnest_mcmc_gdata_steps, nnest_spline_mcmc_gdata_steps)
against the adaptive-walk kernels at the same shape, per x_dim and flow (NVP, spline), `walkers` chains x `steps` steps, on the same
flow (at its initialisation: nothing is trained), T and start, with the histories written, every step local (global_every = 0) and
the adaptation off:
  adapt   nnest_mcmc_adapt_steps / nnest_spline_mcmc_adapt_steps with NNEST_LIKE_GAUSSIAN (corr 0.5) -- units this tree does not
          touch: the parent commit's kernels, on a likelihood that needs two moments of the row;
  gdata   the new entry on tests/gdata_check.make_target's dense P: D (D + 1) / 2 products per evaluation, R read from global
          memory.
The ratio gdata / adapt is the price of those products.  The routes alternate in one process: after a warm-up of each, `reps` rounds,
each launch timed by a host clock around work that ends in a device synchronise.  Printed per route: the mean, the standard
deviation and the standard error of the mean, and the acceptance; per case the ratio of the means with its standard error (first
order, from the two standard errors).  There is no pass/fail ratio: the figures are recorded.
   python tools/time_mcmc_gdata.py [--reps R] [--out FILE] [x_dim walkers steps] ...
   (default: --reps 20, 50 1000 250 and 20 1000 250; --out appends the report to FILE, e.g. profiles/mcmc_gdata/summary.txt)"""
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnest_amd  # noqa: E402
from nnest_amd import _lib, flow, likelihoods  # noqa: E402
from tests import gdata_check as gc  # noqa: E402

GAUSS, CORR = 3, 0.5


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


def entry(net, which, like, z0, S, step, t_std, t_mean, seed):
    """the adaptive or the gdata entry itself at global_every = 0, adapt_steps = 0, no step_in; like: the struct the entry takes"""
    dev = z0.device
    C, D = z0.shape
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64), logl=torch.empty(C, **f64),
               hist_z=torch.empty(C, S, D, **f32), hist_x=torch.empty(C, S, D, **f32), hist_logl=torch.empty(C, S, **f64),
               n_accept=torch.empty(C, dtype=torch.int32, device=dev), n_accept_global=torch.empty(C, dtype=torch.int32, device=dev),
               step=torch.empty(C, **f64), hist_step=torch.empty(C, S, **f64))
    with torch.cuda.device(dev):
        _lib.check(net._sym[which](
            net._h, ctypes.byref(like), _lib.ptr(t_std), _lib.ptr(t_mean), None, None, _lib.ptr(z0), None, None, _lib.ptr(out['z']),
            _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']), _lib.ptr(out['hist_z']), _lib.ptr(out['hist_x']),
            _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, S, ctypes.c_float(step), 0, int(seed), 0, ctypes.c_double(1.0), 0,
            _lib.ptr(out['n_accept_global']), None, _lib.ptr(out['step']), _lib.ptr(out['hist_step']), ctypes.c_uint32(0),
            ctypes.c_double(1.0), ctypes.c_double(0.234), _lib.current_stream(dev)))
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
    nums = nums or [50, 1000, 250, 20, 1000, 250]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    tmp = tempfile.mkdtemp()
    for D, C, S in zip(*[iter(nums)] * 3):
        step = 2.0 / np.sqrt(D)
        x0 = np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5
        mu, P = gc.make_target(D, D)
        data = likelihoods.GaussianData(mu, precision=P).hip_like_data
        for flow_name in ('nvp', 'spline'):
            s = nnest_amd.MCMCSampler(D, likelihoods.Gaussian(D, CORR), log_dir=tmp, log_level=30, flow=flow_name)
            net = s.trainer.netG
            z0, _ = net.forward(x0)   # (the spline: sets the ActNorm layers from the start points)
            z0 = z0.contiguous()
            t_std = torch.full((D,), 0.5, dtype=torch.float32, device=z0.device)
            t_mean = torch.zeros(D, dtype=torch.float32, device=z0.device)
            spec, keep = flow.gdata_spec(data, z0.device)
            lk = _lib.like_spec(GAUSS, 1.0, (CORR,))
            say('x_dim %d, %s flow, %d chains x %d steps, step %.3f' % (D, flow_name, C, S, step))
            routes = {'adapt': lambda seed: entry(net, 'mcmc_adapt', lk, z0, S, step, t_std, t_mean, seed),
                      'gdata': lambda seed: entry(net, 'mcmc_gdata', spec, z0, S, step, t_std, t_mean, seed)}
            ts, acc = {n: [] for n in routes}, {}
            for name, fn in routes.items():   # warm-up: code objects, allocator
                timed(fn, 0)
            for r in range(reps):
                for name, fn in routes.items():
                    ms, out = timed(fn, r + 1)
                    ts[name].append(ms)
                    acc[name] = float(out['n_accept'].sum()) / (C * S)
            m, e = {}, {}
            for name in routes:
                m[name], sd, e[name] = stats(ts[name])
                say('  kernel %-6s %9.3f ms per launch (mean of %d; sd %.3f, se %.3f), %8.2f us per step, acceptance %.3f'
                    % (name, m[name], len(ts[name]), sd, e[name], 1e3 * m[name] / S, acc[name]))
            ratio = m['gdata'] / m['adapt']
            say('  gdata / adapt: %.3fx +- %.3f (%d products per evaluation)'
                % (ratio, ratio * np.hypot(e['gdata'] / m['gdata'], e['adapt'] / m['adapt']), D * (D + 1) // 2))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
