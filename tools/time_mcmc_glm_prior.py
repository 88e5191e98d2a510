"""Developer diagnostic: the kernels of the regression likelihoods of user data under normal priors (nnest_mcmc_glm_prior_steps,
nnest_spline_mcmc_glm_prior_steps)
1. against the kernels without the prior at the same shape (nnest_mcmc_glm_steps, nnest_spline_mcmc_glm_steps: units this change
   does not edit), per x_dim, flow (NVP, spline) and family, `walkers` chains x `steps` steps, on the same flow (at its
   initialisation: nothing is trained), T, data and start, with the histories written, every step local (global_every = 0) and the
   adaptation off.  The prior adds 2 D float32 operations, D float64 products and four shuffles to an evaluation of n D products:
   the ratio prior / glm is the price of that, and of the registers or LDS reads it takes.
2. through the front end: MCMCSampler.run(route='fused') against route='host' with the same callable and the same GaussianPrior
   -- the only route this pair had before --, the flow trained once beforehand (its training is outside the clock).
The sides alternate in one process: after a warm-up of each, `reps` rounds, each launch timed by a host clock around work that ends
in a device synchronise.  Printed per side: the mean, the standard deviation and the standard error of the mean; per case the ratio
of the means with its standard error (first order, from the two standard errors).  There is no pass/fail ratio: the figures are
recorded.
   python tools/time_mcmc_glm_prior.py [--reps R] [--rows N] [--fe-reps R] [--out FILE] [x_dim walkers steps] ...
   (default: --reps 20 --rows 1024 --fe-reps 20, 50 1000 250 and 20 1000 250; --fe-reps 0 skips part 2; --out appends the report to
   FILE, e.g. profiles/mcmc_glm_prior/summary.txt)"""
import ctypes
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnest_amd  # noqa: E402
from nnest_amd import _lib, flow, likelihoods  # noqa: E402
from nnest_amd.priors import GaussianPrior  # noqa: E402
from tests import glm_check as gk  # noqa: E402
from time_mcmc_glm import alternate  # noqa: E402


def entry(net, like, prior, z0, S, step, t_std, t_mean, seed):
    """the glm entry (prior None) or the glm_prior entry itself at global_every = 0, adapt_steps = 0, no step_in"""
    dev = z0.device
    C, D = z0.shape
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64), logl=torch.empty(C, **f64),
               hist_z=torch.empty(C, S, D, **f32), hist_x=torch.empty(C, S, D, **f32), hist_logl=torch.empty(C, S, **f64),
               n_accept=torch.empty(C, dtype=torch.int32, device=dev), n_accept_global=torch.empty(C, dtype=torch.int32, device=dev),
               step=torch.empty(C, **f64), hist_step=torch.empty(C, S, **f64))
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc_glm' if prior is None else 'mcmc_glm_prior'](
            net._h, ctypes.byref(like), *(() if prior is None else (ctypes.byref(prior),)), _lib.ptr(t_std), _lib.ptr(t_mean), None, None,
            _lib.ptr(z0), None, None, _lib.ptr(out['z']), _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']),
            _lib.ptr(out['hist_z']), _lib.ptr(out['hist_x']), _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, S,
            ctypes.c_float(step), 0, int(seed), 0, ctypes.c_double(1.0), 0, _lib.ptr(out['n_accept_global']), None, _lib.ptr(out['step']),
            _lib.ptr(out['hist_step']), ctypes.c_uint32(0), ctypes.c_double(1.0), ctypes.c_double(0.234), _lib.current_stream(dev)))
    return out


def main(argv):
    reps, fe_reps, rows, out_path, nums = 20, 20, 1024, None, []
    fe_chains, fe_steps = 1000, 250
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--fe-reps':
            fe_reps = int(next(it))
        elif a == '--rows':
            rows = int(next(it))
        elif a == '--out':
            out_path = next(it)
        else:
            nums.append(int(a))
    nums = nums or [50, 1000, 250, 20, 1000, 250]
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    def say(s):   # (line by line: a run that is cut short keeps what it measured)
        print(s, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(s + '\n')

    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    tmp = tempfile.mkdtemp()
    for D, C, S in zip(*[iter(nums)] * 3):
        step = 2.0 / np.sqrt(D)
        x0 = np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5
        likes = dict((fam, gk.make_like(D, rows, fam, D)) for fam in gk.FAMILIES)
        prior = GaussianPrior(D, 0.0, 2.0)
        for flow_name in ('nvp', 'spline'):
            s = nnest_amd.MCMCSampler(D, likelihoods.Gaussian(D, 0.5), log_dir=tmp, log_level=30, flow=flow_name)
            net = s.trainer.netG
            z0, _ = net.forward(x0)   # (the spline: sets the ActNorm layers from the start points)
            z0 = z0.contiguous()
            t_std = torch.full((D,), 0.5, dtype=torch.float32, device=z0.device)
            t_mean = torch.zeros(D, dtype=torch.float32, device=z0.device)
            specs = dict((fam, flow.glm_spec(like.hip_like_glm, z0.device)) for fam, like in likes.items())
            pspec, pkeep = flow.gauss_prior_spec(prior.hip_gauss_prior, z0.device)
            say('x_dim %d, n %d, %s flow, %d chains x %d steps, step %.3f' % (D, rows, flow_name, C, S, step))
            sides = {}
            for fam in gk.FAMILIES:
                sides[fam] = lambda seed, fam=fam: entry(net, specs[fam][0], None, z0, S, step, t_std, t_mean, seed)
                sides[fam + '+prior'] = lambda seed, fam=fam: entry(net, specs[fam][0], pspec, z0, S, step, t_std, t_mean, seed)
            m, e = alternate(sides, reps, say, lambda name, mean, k, sd, se, out:
                             '  kernel %-14s %9.3f ms per launch (mean of %d; sd %.3f, se %.3f), %8.2f us per step, acceptance %.3f'
                             % (name, mean, k, sd, se, 1e3 * mean / S, float(out['n_accept'].sum()) / (C * S)))
            for fam in gk.FAMILIES:
                ratio = m[fam + '+prior'] / m[fam]
                say('  %s: prior / glm: %.3fx +- %.3f' % (fam, ratio, ratio * np.hypot(e[fam + '+prior'] / m[fam + '+prior'], e[fam] / m[fam])))
    if fe_reps > 0:
        for D in sorted(set(nums[0::3])):
            for fam in gk.FAMILIES:
                like = gk.make_like(D, rows, fam, D)
                prior = GaussianPrior(D, 0.0, 2.0)
                th, _ = gk.posterior_mode(like, -5.0, 5.0, iters=30)
                rng = np.random.RandomState(1)
                train = th + 0.1 * rng.normal(size=(2000, D))
                for flow_name in ('nvp', 'spline'):
                    np.random.seed(0)
                    torch.manual_seed(0)
                    s = nnest_amd.MCMCSampler(D, like, prior=prior, log_dir=tmp, log_level=30, flow=flow_name)
                    init = ((train[:fe_chains] - train.mean(0)) / train.std(0))
                    try:
                        s.run(2, fe_chains, train, init_samples=init, route='fused', seed=0)   # (trains the flow; kept for every run below)
                    except ValueError as err:   # (the probe's tolerances are absolute beyond |logL| of 1e1: a refusal is reported)
                        say('front end: x_dim %d, n %d, %s, %s flow: %s' % (D, rows, fam, flow_name, err))
                        continue
                    s.trainer.train = lambda samples, **kw: None
                    say('front end: x_dim %d, n %d, %s under GaussianPrior(0, 2), %s flow, %d chains x %d steps' % (
                        D, rows, fam, flow_name, fe_chains, fe_steps))
                    sides = dict((route, lambda seed, route=route: s.run(fe_steps, fe_chains, train, init_samples=init, route=route, seed=seed))
                                 for route in ('host', 'fused'))
                    m, e = alternate(sides, fe_reps, say, lambda name, mean, k, sd, se, out:
                                     '  route %-6s %10.2f ms per run (mean of %d; sd %.2f, se %.2f)' % (name, mean, k, sd, se))
                    ratio = m['host'] / m['fused']
                    say('  host / fused: %.2fx +- %.2f' % (ratio, ratio * np.hypot(e['host'] / m['host'], e['fused'] / m['fused'])))


if __name__ == '__main__':
    main(sys.argv[1:])
