"""Developer diagnostic: the slice proposal on a regression likelihood of user data (nnest_slice_glm_steps, nnest_spline_slice_glm_steps;
DESIGN.md 3.22) -- the fused entry against (a) slice_rounds(like_glm=...) of the same build, the device likelihood between the round
driver's launches, and (b) the host protocol, slice_rounds with the host callable: the only route before the fused kernels.
   python tools/time_slice_glm.py [kernels] [front] [seeds] [--out FILE]
kernels: n = 1024 rows, 1000 walkers x 25 updates, x_dim 20 and 50, both families, NVP and spline flow; the three routes ALTERNATE
         within each repeat, the means are over the repeats and a ratio's standard error is that of the per-repeat ratios.
front:   one NestedSampler run each way (slice_route 'fused-glm' and 'host') on the 2-D logistic regression of the tests, wall time.
seeds:   both routes' |log Z - quadrature| / sigma over 8 seeds on that problem (sigma = sqrt(H / N): tests/test_gpu_nested_glm.py).
Every timing ends in a device synchronise; the first repeat of every route is a warm-up and is dropped."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import flow  # noqa: E402
from nnest_amd.likelihoods import GLMData  # noqa: E402
from nnest_amd.slice_rounds import slice_rounds  # noqa: E402
from nnest_amd.spline import HipSpline  # noqa: E402

N_ROWS, C, S, SCALE, REPEATS = 1024, 1000, 25, 3.0, 6
OUT = [sys.stdout]


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


def kernels():
    say('n = %d rows, %d walkers x %d updates, T(x) = %g x, width 2 / sqrt(x_dim); ms per batch, mean over %d alternating repeats' % (
        N_ROWS, C, S, SCALE, REPEATS - 1))
    say('%-7s %-9s %5s | %10s %10s %10s | %16s %16s | %s' % ('flow', 'family', 'x_dim', 'fused', 'rounds-glm', 'host', 'rounds / fused', 'host / fused',
                                                            'evals/update  n_call/n_eval  rounds'))
    for name in ('nvp', 'spline'):
        for D in (20, 50):
            net = flow.HipNVP(D, 16, 3, 1, seed=0) if name == 'nvp' else HipSpline(D, 16, 3, 8, 3.0, seed=0)
            u0 = np.random.RandomState(0).uniform(-0.6, 0.6, size=(C, D))
            z0, _ = net.forward(u0)
            assert net.slice_glm_refusal() is None
            sd, mu = np.full(D, SCALE, np.float32), np.zeros(D, np.float32)
            for family in ('logistic', 'poisson'):
                like = make_like(D, family, 7 + D)
                data = like.hip_like_glm
                x0, _ = net.inverse(z0)
                l0 = flow.loglike_glm(data, x0 * SCALE, device=net.device)
                star = float(l0.min()) - 1.0
                kw = dict(like_glm=data, t_std=sd, t_mean=mu)
                host = lambda x: like.loglike_rows(SCALE * x.astype(np.float64))
                routes = {
                    'fused': lambda z, l, k: net.slice_steps(None, 1.0, z, l, star, 2.0 / np.sqrt(D), S, seed=k, **kw),
                    'rounds': lambda z, l, k: slice_rounds(net, z, l, star, 2.0 / np.sqrt(D), S, seed=k, **kw),
                    'host': lambda z, l, k: slice_rounds(net, z, l, star, 2.0 / np.sqrt(D), S, seed=k, loglike=host)}
                ms = {r: [] for r in routes}
                last = {}
                for k in range(REPEATS):
                    for r, run in routes.items():
                        z, l = z0.clone(), l0.clone()
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        last[r] = run(z, l, k)
                        torch.cuda.synchronize()
                        ms[r].append(1e3 * (time.perf_counter() - t))
                t = {r: np.asarray(v[1:]) for r, v in ms.items()}

                def ratio(a, b):
                    q = t[a] / t[b]
                    return '%7.2f +- %5.2f' % (t[a].mean() / t[b].mean(), q.std(ddof=1) / np.sqrt(len(q)))
                res = last['fused']
                ne = int(res['n_eval'].sum())
                say('%-7s %-9s %5d | %10.3f %10.3f %10.3f | %16s %16s | %.2f  %.2f  %d' % (
                    name, family, D, t['fused'].mean(), t['rounds'].mean(), t['host'].mean(), ratio('rounds', 'fused'), ratio('host', 'fused'),
                    ne / float(C * S), int(res['n_call'].sum()) / float(ne), last['rounds']['rounds']))


def front_like():
    from tests import glm_check as gk
    return gk.make_like(2, 40, 'logistic', 5)


def front_run(flow_name, seed, fused_route, log_dir):
    from nnest_amd.nested import NestedSampler
    np.random.seed(seed)
    torch.manual_seed(seed)
    s = NestedSampler(2, front_like(), transform=lambda x: 5.0 * x, log_dir=log_dir, num_live_points=200, log_level=30, flow=flow_name,
                      mcmc_proposal='slice')
    if not fused_route:
        s._slice_glm = None
    torch.cuda.synchronize()
    t = time.perf_counter()
    s.run(mcmc_num_chains=50, mcmc_steps=10, train_iters=200)
    torch.cuda.synchronize()
    return s, time.perf_counter() - t


def front(seeds):
    from tests.test_gpu_nested_glm import reference
    ref = reference()
    say('NestedSampler(2, GLMData 2-D logistic, transform 5 x, mcmc_proposal slice, 200 live points), 50 chains x 10 updates a batch; '
        'quadrature log Z %.4f, H %.3f, sigma %.4f' % (ref['exact'], ref['H'], ref['sigma']))
    for name in ('nvp', 'spline'):
        for fused_route in (True, False):
            off, secs, calls = [], [], []
            for seed in seeds:
                with tempfile.TemporaryDirectory() as d:
                    s, dt = front_run(name, seed, fused_route, d)
                off.append(abs(s.logz - ref['exact']) / ref['sigma'])
                secs.append(dt)
                calls.append(s.total_calls)
                route = s.slice_route
            say('%-7s %-10s seeds %s: run %.2f s (mean), %d likelihood calls (mean); |log Z - exact| / sigma: mean %.2f, max %.2f  [%s]' % (
                name, route, list(seeds), np.mean(secs), np.mean(calls), np.mean(off), np.max(off), ' '.join('%.2f' % v for v in off)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if '--out' in args:
        i = args.index('--out')
        os.makedirs(os.path.dirname(os.path.abspath(args[i + 1])), exist_ok=True)
        OUT.append(open(args[i + 1], 'a'))
        del args[i:i + 2]
    what = args or ['kernels', 'front']
    assert torch.cuda.is_available(), 'tools/time_slice_glm.py needs an MI355X'
    say('# %s' % torch.cuda.get_device_name(0))
    if 'kernels' in what:
        kernels()
    if 'front' in what:
        front([1])
    if 'seeds' in what:
        front(range(8))
