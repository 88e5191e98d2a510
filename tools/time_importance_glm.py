"""Developer diagnostic: the fused importance-sampling kernels on a regression likelihood of user data (nnest_importance_glm_evidence,
nnest_spline_importance_glm_evidence) against the route composed from entries that were there before them, per case (x_dim, family,
with or without the normal prior) and flow (NVP, spline), `--samples` samples with no per-sample outputs, n = `--rows` data rows:
  fused:     HipNVP / HipSpline.importance_evidence(like_glm=..., [prior_gauss=...]) in one launch, the sums read on the host;
  composed:  flow.importance_fill_noise -> .mcmc_steps(steps = 0, like_glm=..., [prior_gauss=...]) (x, lp and logL of every row
             written to memory) -> lp - logb and the max / exp / sum reductions in torch float64, in chunks of `--chunk` rows;
  host:      Sampler.importance_evidence(route='host') on the same model and flow family -- netG.sample, netG.log_probs and the
             Python likelihood in chunks of 2^16 with [chunk x n] float64 temporaries on the host --, `--host-samples` samples (fewer:
             it is slow), timed by the wall clock and scaled to `--samples`.
Without the prior the target is under the box +-3 on T(x).  fused and composed alternate in one process: after a warm-up of each,
`reps` rounds, each timed by device events around work that ends in a synchronise.  Printed per route: the mean, the standard
deviation and the standard error of the mean; per case the ratio of the means with its standard error (the two relative standard
errors in quadrature).  There is no pass/fail ratio: the figures are recorded.
   python tools/time_importance_glm.py [--reps R] [--samples N] [--host-samples N] [--rows N] [--chunk C] [--out FILE] [x_dim] ...
   (default: --reps 10 --samples 2^20 --host-samples 2^17 --rows 1024, x_dim 20 and 50; --out appends the report to FILE, e.g.
   profiles/importance_glm/summary.txt)"""
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnest_amd  # noqa: E402
from nnest_amd import _lib, flow  # noqa: E402
from nnest_amd.likelihoods import GLMData  # noqa: E402
from nnest_amd.priors import GaussianPrior, UniformPrior  # noqa: E402
from nnest_amd.spline import HipSpline  # noqa: E402

BOX = 3.0


def make_like(D, n, family, seed):
    """the tests' data (tests/glm_check.make_data): A uniform in +-1/sqrt(D), y drawn from the model at a theta in +-1"""
    r = np.random.RandomState(seed)
    A = r.uniform(-1.0, 1.0, size=(n, D)) / np.sqrt(D)
    theta = r.uniform(-1.0, 1.0, D)
    o = r.uniform(-0.2, 0.2, n)
    eta = o + A @ theta
    y = (r.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64) if family == 'logistic' else r.poisson(np.exp(eta + 0.5)).astype(np.float64)
    return GLMData(A, y, family=family, offset=o)


def timed(fn, seed):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn(seed)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main(argv):
    reps, out_path, M, M_host, n, chunk, dims = 10, None, 1 << 20, 1 << 17, 1024, 1 << 20, []
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--out':
            out_path = next(it)
        elif a == '--samples':
            M = int(next(it))
        elif a == '--host-samples':
            M_host = int(next(it))
        elif a == '--rows':
            n = int(next(it))
        elif a == '--chunk':
            chunk = int(next(it))
        else:
            dims.append(int(a))
    dims = dims or [20, 50]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for D in dims:
        std, mean = np.full(D, 0.5), np.zeros(D)
        x0 = np.random.RandomState(0).normal(size=(1000, D)).astype(np.float32) * 0.5
        logb_const = 0.5 * D * math.log(2.0 * math.pi)
        for family in ('logistic', 'poisson'):
            like = make_like(D, n, family, D)
            for with_prior in (False, True):
                prior = GaussianPrior(D, 0.0, 2.0) if with_prior else UniformPrior(D, -BOX, BOX)
                for flow_name in ('nvp', 'spline'):
                    net = flow.HipNVP(D, 16, 3, 1, seed=0) if flow_name == 'nvp' else HipSpline(D, 16, 3, seed=0)
                    net.forward(x0)   # (the spline: sets the ActNorm layers from these points)
                    kw = dict(t_std=std, t_mean=mean, like_glm=like.hip_like_glm)
                    if with_prior:
                        kw['prior_gauss'] = prior.hip_gauss_prior
                    else:
                        kw.update(lo=-np.full(D, BOX), hi=np.full(D, BOX))

                    def fused(seed):
                        return tuple(net.importance_evidence(None, M, seed=seed, **kw)['sums'].cpu().numpy())   # (the copy is the synchronise)

                    def composed(seed):
                        parts = []
                        for first in range(0, M, chunk):
                            z = flow.importance_fill_noise(min(chunk, M - first), D, seed=seed, sample_offset=first, device=net.device)
                            ev = net.mcmc_steps(None, z, 0, 0.1, **kw)
                            logw = ev['lp'] + 0.5 * (z.double() ** 2).sum(1) + logb_const
                            live = torch.isfinite(logw)
                            a = torch.where(live, logw, torch.full_like(logw, -math.inf)).max()
                            e = torch.where(live, torch.exp(logw - a), torch.zeros_like(logw))
                            parts.append(torch.stack([a, e.sum(), (e * e).sum(), live.double().sum()]))
                        return _lib.merge_importance([tuple(p.cpu().numpy()) for p in parts])

                    routes = {'fused': fused, 'composed': composed}
                    say('x_dim %d, n %d, %s, %s, %s flow, %d samples (composed: chunks of %d)'
                        % (D, n, family, 'GaussianPrior' if with_prior else 'box', flow_name, M, min(chunk, M)))
                    ts, res = {name: [] for name in routes}, {}
                    for name, fn in routes.items():   # warm-up: code objects, allocator
                        timed(fn, 0)
                    for k in range(reps):
                        for name, fn in routes.items():
                            ms, res[name] = timed(fn, k + 1)
                            ts[name].append(ms)
                    m, se = {}, {}
                    for name in routes:
                        t = np.asarray(ts[name])
                        m[name] = float(t.mean())
                        se[name] = float(t.std(ddof=1) / np.sqrt(len(t))) if len(t) > 1 else 0.0
                        r = _lib.importance_result(*res[name], M)
                        say('  %-9s %9.3f ms (mean of %d; sd %.3f, standard error %.3f), %.3g evaluations / s; logz_x %.3f, ESS %.1f'
                            % (name, m[name], len(t), float(t.std(ddof=1)) if len(t) > 1 else 0.0, se[name], M / (1e-3 * m[name]), r['logz_x'],
                               r['ess']))
                    ratio = m['composed'] / m['fused']
                    say('  composed / fused: %.2fx +- %.2f' % (ratio, ratio * math.hypot(se['composed'] / m['composed'], se['fused'] / m['fused'])))
                    # the host route, through the front end on a flow of the same family
                    with tempfile.TemporaryDirectory() as tmp:
                        s = nnest_amd.MCMCSampler(D, like, prior=prior, log_dir=tmp, log_level=30, flow=flow_name)
                        s._install_transform(mean, std)
                        s.trainer.netG.forward(x0)
                        s.importance_evidence(1 << 12, route='host')   # warm-up
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        s.importance_evidence(M_host, route='host')
                        torch.cuda.synchronize()
                        host_ms = 1e3 * (time.perf_counter() - t0) * (M / float(M_host))
                    say('  host      %9.1f ms (one call of %d samples, scaled to %d); host / fused: %.0fx' % (host_ms, M_host, M, host_ms / m['fused']))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
