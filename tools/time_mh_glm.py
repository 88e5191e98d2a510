"""Developer diagnostic: the Metropolis proposal on a regression likelihood of user data (nnest_mh_glm_steps, nnest_spline_mh_glm_steps;
DESIGN.md 3.23) -- the fused entry against (a) the host protocol of the same build, the only route before the fused kernels, and (b)
nnest_mcmc_glm_steps / nnest_spline_mcmc_glm_steps at the same shape: the same flow and likelihood without the constraint, the skip or
the step rule.
   python tools/time_mh_glm.py [kernels] [host] [front] [seeds] [--steps K] [--dims 20,50] [--out FILE]
kernels: n = 1024 rows, 1000 walkers x 250 steps, x_dim 20 and 50, both families, NVP and spline flow; the batch rule at the default
         lag, the batch rule at lag 0 and the fixed step of the new entry and the mcmc_glm entry ALTERNATE within each repeat; the
         means are over the repeats after a warm-up, a ratio's standard error is that of the per-repeat ratios.  Also the share of
         steps with pre (n_call / steps) and of accepted steps.
host:    at the same shape, Sampler._mcmc_endpoints_fused (mh_route 'fused-glm') against Sampler._mcmc_sample_host with the same
         callable, from the same live points, the batch rule; the same method.
front:   one NestedSampler run each way (mh_route 'fused-glm' and 'host') on the 2-D logistic regression of the tests, wall time.
seeds:   both routes' |log Z - quadrature| / sigma over seeds 0 .. 7 on that problem with `--steps` MCMC steps a batch (default 10)
         (sigma = sqrt(H / N): tests/test_gpu_nested_glm.py) -- what tests/test_gpu_nested_mh_glm.py's MCMC_STEPS was chosen from.
Every timing ends in a device synchronise; the first repeat of every route is a warm-up and is dropped."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import _lib, flow  # noqa: E402
from nnest_amd.likelihoods import GLMData  # noqa: E402
from nnest_amd.spline import HipSpline  # noqa: E402

N_ROWS, C, S, SCALE, REPEATS = 1024, 1000, 250, 3.0, 6
OUT = [sys.stdout]
DIMS = [20, 50]


def say(text=''):
    for f in OUT:
        f.write(text + '\n')
        f.flush()


def make_like(D, family, seed):
    r = np.random.RandomState(seed)
    A = r.uniform(-1.0, 1.0, size=(N_ROWS, D)) / np.sqrt(D)
    eta = A @ r.uniform(-1.0, 1.0, D)
    y = (r.uniform(size=N_ROWS) < 1.0 / (1.0 + np.exp(-eta))).astype(float) if family == 'logistic' else r.poisson(np.exp(eta + 0.5)).astype(float)
    return GLMData(A, y, family=family)


def timed(routes, prepare):
    """ms per call of each route, alternating within REPEATS repeats, the first dropped; the last result of each"""
    ms, last = {r: [] for r in routes}, {}
    for k in range(REPEATS):
        for r, run in routes.items():
            args = prepare()
            torch.cuda.synchronize()
            t = time.perf_counter()
            last[r] = run(k, *args)
            torch.cuda.synchronize()
            ms[r].append(1e3 * (time.perf_counter() - t))
    return {r: np.asarray(v[1:]) for r, v in ms.items()}, last


def ratio(t, a, b):
    q = t[a] / t[b]
    return '%6.3f +- %5.3f' % (t[a].mean() / t[b].mean(), q.std(ddof=1) / np.sqrt(len(q)))


def kernels():
    say('n = %d rows, %d walkers x %d steps, T(x) = %g x, step 0.5 / sqrt(x_dim), L* = the 20 %% quantile of the start; ms per launch, mean over '
        '%d alternating repeats; lag %d = the default' % (N_ROWS, C, S, SCALE, REPEATS - 1, _lib.MH_DEFAULT_LAG))
    say('%-7s %-9s %5s | %9s %9s %9s %9s | %15s %15s %15s | %10s | %s' % (
        'flow', 'family', 'x_dim', 'batch', 'batch l0', 'fixed', 'mcmc_glm', 'batch / mcmc', 'fixed / mcmc', 'lag 0 / fixed', 'us/step l0-fx', 'pre  acc (fixed)  pre  acc (batch)'))
    for name in ('nvp', 'spline'):
        for D in DIMS:
            net = flow.HipNVP(D, 16, 3, 1, seed=0) if name == 'nvp' else HipSpline(D, 16, 3, 8, 3.0, seed=0)
            u0 = np.random.RandomState(0).uniform(-0.6, 0.6, size=(C, D))
            z0, _ = net.forward(u0)
            sd, mu = np.full(D, SCALE, np.float32), np.zeros(D, np.float32)
            step = 0.5 / np.sqrt(D)
            for family in ('logistic', 'poisson'):
                data = make_like(D, family, 7 + D).hip_like_glm
                x0, _ = net.inverse(z0)
                l0 = flow.loglike_glm(data, x0 * SCALE, device=net.device)
                star = float(torch.quantile(l0, 0.2))
                for mode, lag in (('batch', None), ('batch', 0), (False, None)):
                    assert net.mh_glm_refusal(D, C, mode, lag) is None
                kw = dict(like_glm=data, t_std=sd, t_mean=mu)
                routes = {
                    'batch': lambda k, z, l: net.mh_steps(None, 1.0, z, l, star, step, S, dynamic='batch', seed=k, **kw),
                    'batch0': lambda k, z, l: net.mh_steps(None, 1.0, z, l, star, step, S, dynamic='batch', lag=0, seed=k, **kw),
                    'fixed': lambda k, z, l: net.mh_steps(None, 1.0, z, l, star, step, S, dynamic=False, seed=k, **kw),
                    'mcmc': lambda k, z, l: net.mcmc_steps(None, z, S, step, lo=-sd, hi=sd, seed=k, history=False, **kw)}
                t, last = timed(routes, lambda: (z0.clone(), l0.clone()))
                for r in ('batch', 'batch0'):
                    net.check_sync(last[r])
                share = lambda r: (float(last[r]['n_call'].sum()) / (C * S), float(last[r]['n_accept'].sum()) / (C * S))
                say('%-7s %-9s %5d | %9.3f %9.3f %9.3f %9.3f | %15s %15s %15s | %10.2f | %.2f %.2f  %.2f %.2f' % (
                    name, family, D, t['batch'].mean(), t['batch0'].mean(), t['fixed'].mean(), t['mcmc'].mean(), ratio(t, 'batch', 'mcmc'),
                    ratio(t, 'fixed', 'mcmc'), ratio(t, 'batch0', 'fixed'), 1e3 * (t['batch0'].mean() - t['fixed'].mean()) / S,
                    *(share('fixed') + share('batch'))))


def host():
    from nnest_amd.nested import NestedSampler
    say('Sampler._mcmc_endpoints_fused (mh_route fused-glm) against Sampler._mcmc_sample_host, the same callable and live points: n = %d rows, '
        '%d walkers x %d steps, the batch rule; ms per batch, mean over %d alternating repeats' % (N_ROWS, C, S, REPEATS - 1))
    say('%-7s %-9s %5s | %10s %12s | %18s' % ('flow', 'family', 'x_dim', 'fused-glm', 'host', 'host / fused-glm'))
    for name in ('nvp', 'spline'):
        for D in DIMS:
            for family in ('logistic', 'poisson'):
                like = make_like(D, family, 7 + D)
                with tempfile.TemporaryDirectory() as d:
                    s = NestedSampler(D, like, transform=lambda x: SCALE * x, log_dir=d, num_live_points=C, log_level=30, flow=name)
                    assert s._mh_glm is not None
                    u0 = np.random.RandomState(0).uniform(-0.6, 0.6, size=(C, D))
                    l0 = like.loglike_rows(SCALE * u0)
                    star = float(np.quantile(l0, 0.2))
                    keep = l0 > star
                    u0, l0 = u0[keep], l0[keep]
                    step = 0.5 / np.sqrt(D)
                    routes = {
                        'fused': lambda k: s._mcmc_endpoints_fused(S, step, True, u0, l0, star, 0, k),
                        'host': lambda k: s._mcmc_sample_host(S, step, True, len(l0), u0, l0, None, star, 100, 1)}
                    t, last = timed(routes, lambda: ())
                    assert s.mh_route == 'host' and s._mh_glm is not None
                say('%-7s %-9s %5d | %10.3f %12.3f | %18s   (%d walkers above L*)' % (name, family, D, t['fused'].mean(), t['host'].mean(),
                                                                                     ratio(t, 'host', 'fused'), len(l0)))


def front_like():
    from tests import glm_check as gk
    return gk.make_like(2, 40, 'logistic', 5)


def front_run(flow_name, seed, fused_route, log_dir, steps):
    from nnest_amd.nested import NestedSampler
    np.random.seed(seed)
    torch.manual_seed(seed)
    s = NestedSampler(2, front_like(), transform=lambda x: 5.0 * x, log_dir=log_dir, num_live_points=200, log_level=30, flow=flow_name)
    if not fused_route:
        s._mh_glm = None
    torch.cuda.synchronize()
    t = time.perf_counter()
    s.run(mcmc_num_chains=50, mcmc_steps=steps, train_iters=200)
    torch.cuda.synchronize()
    return s, time.perf_counter() - t


def front(seeds, steps):
    from tests.test_gpu_nested_glm import reference
    ref = reference()
    say('NestedSampler(2, GLMData 2-D logistic, transform 5 x, mcmc_proposal mh, 200 live points), 50 chains x %d steps a batch; '
        'quadrature log Z %.4f, H %.3f, sigma %.4f' % (steps, ref['exact'], ref['H'], ref['sigma']))
    for name in ('nvp', 'spline'):
        for fused_route in (True, False):
            off, secs, calls = [], [], []
            for seed in seeds:
                with tempfile.TemporaryDirectory() as d:
                    s, dt = front_run(name, seed, fused_route, d, steps)
                off.append(abs(s.logz - ref['exact']) / ref['sigma'])
                secs.append(dt)
                calls.append(s.total_calls)
                route = s.mh_route
            say('%-7s %-10s steps %2d seeds %s: run %.2f s (mean), %d likelihood calls (mean); |log Z - exact| / sigma: mean %.2f, max %.2f  [%s]' % (
                name, route, steps, list(seeds), np.mean(secs), np.mean(calls), np.mean(off), np.max(off), ' '.join('%.2f' % v for v in off)))


if __name__ == '__main__':
    args = sys.argv[1:]
    steps = 10
    if '--out' in args:
        i = args.index('--out')
        os.makedirs(os.path.dirname(os.path.abspath(args[i + 1])), exist_ok=True)
        OUT.append(open(args[i + 1], 'a'))
        del args[i:i + 2]
    if '--steps' in args:
        i = args.index('--steps')
        steps = int(args[i + 1])
        del args[i:i + 2]
    if '--dims' in args:
        i = args.index('--dims')
        DIMS[:] = [int(v) for v in args[i + 1].split(',')]
        del args[i:i + 2]
    what = args or ['kernels', 'host', 'front']
    assert torch.cuda.is_available(), 'tools/time_mh_glm.py needs an MI355X'
    say('# %s' % torch.cuda.get_device_name(0))
    if 'kernels' in what:
        kernels()
    if 'host' in what:
        host()
    if 'front' in what:
        front([1], steps)
    if 'seeds' in what:
        front(range(8), steps)
