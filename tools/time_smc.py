"""Developer diagnostic: the sequential Monte Carlo sampler (nnest_amd.SMCSampler) and its kernels.
  1. the tempered random-walk kernels (nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps) at beta = 0.5 against the
     untempered entries on the same flow and start, at the two configurations of tools/time_mcmc_walk.py (x_dim 50 Rosenbrock and
     x_dim 20 GaussianMix, 1000 chains x 250 steps).  The untempered entries of this library are, instruction for instruction, the
     parent commit's (profiles/smc/resources.txt, 3.): timing them here times the parent's kernels.  The tempered target costs one float64
     multiply per evaluation: expect the ratio within the run-to-run spread.  The ratio is recorded, not asserted.
  2. the service kernels (nnest_smc_reweight, nnest_smc_resample) at a few population sizes.
  3. a full SMCSampler.run on Rosenbrock x_dim 2 and GaussianMix x_dim 20: wall time, stages, and the per-stage split into train,
     move and reweight (with the resampling).
The routes alternate in one process: after a warm-up of each, `reps` rounds, each timed by a host clock around work that ends in a
device synchronise.  Printed per route: the mean, the standard deviation and the standard error of the mean.
   python tools/time_smc.py [--reps R] [--out FILE] [--kernels-only]
   (--out appends the report to FILE, e.g. profiles/smc/summary.txt)"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnest_amd  # noqa: E402
from nnest_amd import flow, likelihoods  # noqa: E402
from nnest_amd.priors import UniformPrior  # noqa: E402

NAMES = {0: 'rosenbrock', 1: 'gaussmix'}
LIKES = {0: likelihoods.Rosenbrock, 1: likelihoods.GaussianMix}
CASES = ((50, 0, 1000, 250), (20, 1, 1000, 250))


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


def kernels(reps, say):
    tmp = tempfile.mkdtemp()
    for D, like_id, C, S in CASES:
        step = 2.0 / np.sqrt(D)
        mean, std = np.zeros(D), np.full(D, 0.5)
        x0 = np.random.RandomState(0).normal(size=(C, D)).astype(np.float32) * 0.5
        for flow_name in ('nvp', 'spline'):
            s = nnest_amd.MCMCSampler(D, LIKES[like_id](D), log_dir=tmp, log_level=30, flow=flow_name)
            net = s.trainer.netG
            z0, _ = net.forward(x0)   # (the spline: sets the ActNorm layers from the start points)
            z0 = z0.contiguous()
            kw = dict(t_std=std, t_mean=mean)
            routes = {'untempered': lambda seed: net.mcmc_steps(like_id, z0, S, step, seed=seed, **kw)}
            routes['beta 0.5'] = lambda seed: net.mcmc_steps(like_id, z0, S, step, seed=seed, beta=0.5, **kw)
            ts, acc = {n: [] for n in routes}, {}
            for fn in routes.values():   # warm-up: code objects, allocator
                timed(fn, 0)
            for k in range(reps):
                for name, fn in routes.items():
                    ms, out = timed(fn, k + 1)
                    ts[name].append(ms)
                    acc[name] = float(out['n_accept'].sum()) / (C * S)
            say('x_dim %d, %s, %s flow, %d chains x %d steps, step %.3f' % (D, NAMES[like_id], flow_name, C, S, step))
            m = {}
            for name in routes:
                m[name], sd, se = stats(ts[name])
                say('  kernel %-10s %9.3f ms per launch (mean of %d; sd %.3f, se %.3f), %8.2f us per step, acceptance %.3f'
                    % (name, m[name], len(ts[name]), sd, se, 1e3 * m[name] / S, acc[name]))
            say('  beta 0.5 / untempered: %.3fx' % (m['beta 0.5'] / m['untempered']))


def service(reps, say):
    rng = np.random.RandomState(1)
    for N, D in ((1000, 20), (1 << 14, 20), (1 << 20, 2)):
        x = rng.uniform(-5, 5, size=(N, 2))
        logl = torch.from_numpy(-(100.0 * (x[:, 1] - x[:, 0] ** 2) ** 2 + (1.0 - x[:, 0]) ** 2)).cuda()
        theta = torch.randn(N, D, device='cuda')
        out, m = flow.smc_reweight(logl, 0.0, 0.5)
        tr, ts = [], []
        for k in range(reps + 1):
            a, (out, m) = timed(lambda seed: flow.smc_reweight(logl, 0.0, 0.5), k)
            b, _ = timed(lambda seed: flow.smc_resample(m, theta, logl, seed, 0), k)
            if k:
                tr.append(a)
                ts.append(b)
        (mr, sdr, _), (ms_, sds, _) = stats(tr), stats(ts)
        say('N %7d, D %2d: reweight %8.3f ms (sd %.3f; bisection to beta\' %.3g), resample %8.3f ms (sd %.3f); one workgroup each'
            % (N, D, mr, sdr, float(out[0]), ms_, sds))


def runs(say):
    tmp = tempfile.mkdtemp()
    for name, D, like, box, N in (('rosenbrock', 2, likelihoods.Rosenbrock(2), 5.0, 1000), ('gaussmix', 20, likelihoods.GaussianMix(20), 10.0, 1000)):
        for flow_name in ('nvp', 'spline'):
            s = nnest_amd.SMCSampler(D, like, prior=UniformPrior(D, -box, box), log_dir=tmp, log_level=30, flow=flow_name)
            np.random.seed(0)
            torch.manual_seed(0)
            ms, _ = timed(lambda seed: s.run(num_particles=N, seed=seed), 1)
            split = {k: sum(t[k] for t in s.stage_times) for k in ('reweight', 'train', 'move')}
            K = len(s.betas)
            say('SMCSampler.run %s x_dim %d, %s flow, %d particles x 25 steps: %.2f s, %d stages, log Z %.3f, route %s, ncall %d'
                % (name, D, flow_name, N, 1e-3 * ms, K, s.logz, s.smc_route, s.total_calls))
            say('  per stage: train %.1f ms, move %.2f ms, reweight + resample %.2f ms; acceptance %.2f .. %.2f'
                % (1e3 * split['train'] / K, 1e3 * split['move'] / K, 1e3 * split['reweight'] / K, min(s.acceptance), max(s.acceptance)))


def main(argv):
    reps, out_path, kernels_only = 5, None, False
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--out':
            out_path = next(it)
        elif a == '--kernels-only':
            kernels_only = True
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    kernels(reps, say)
    if not kernels_only:
        service(reps, say)
        runs(say)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
