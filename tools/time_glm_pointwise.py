"""Developer diagnostic: the pointwise predictive statistics of the regression likelihoods (nnest_glm_pointwise) against the same
statistics composed from this build's torch -- the only route there was before the entry --, per x_dim and family, at n data rows
and S draws that are on the device already:
   fused   one call of nnest_glm_pointwise (its two kernels) into preallocated statistics and partials;
   torch   chunks of `--chunk` draws: float32 t @ A^T + o, the float64 term, torch.logsumexp of l, -l and -2 l over the draws, the
           count, mean and torch.var of l; the chunks joined by torch.logaddexp and Chan's rule.  The [chunk, n] float64 blocks are
           what this route cannot avoid; the chunk is sized to keep them at 256 MB.
The sides alternate in one process: after a warm-up of each, `reps` rounds, each call timed by a host clock around work that ends in
a device synchronise.  Printed per side: the mean, the standard deviation and the standard error of the mean; per case the ratio of
the means with its standard error (first order, from the two standard errors), and how far the two sides' lppd, elpd_isloo and
variance are apart (they differ by the order of the float32 sums).  There is no pass/fail ratio: the figures are recorded.
   python tools/time_glm_pointwise.py [--reps R] [--rows N] [--draws S] [--chunk C] [--out FILE] [x_dim] ...
   (default: --reps 20 --rows 1024 --draws 250000 --chunk 32768, x_dim 20 and 50; --out appends the report to FILE, e.g.
   profiles/glm_pointwise/summary.txt)"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nnest_amd import _lib, flow  # noqa: E402
from tests import glm_check as gk  # noqa: E402
from tests import glm_pointwise_check as pk  # noqa: E402
from time_mcmc_glm import alternate  # noqa: E402


def fused(spec, t, stats, partials):
    dev = t.device
    S, D = t.shape
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nnest_glm_pointwise(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(stats), _lib.ptr(partials), S, D,
                                                   _lib.current_stream(dev)))
    return stats


def composed(family, A32, o32, y64, t, chunk):
    """{lse(l), lse(-l), lse(-2 l), cnt, mean, M2} [n] each, over all draws"""
    acc = None
    for first in range(0, t.shape[0], chunk):
        eta = (t[first:first + chunk] @ A32.T + o32).to(torch.float64)
        if family == 'logistic':
            l = -torch.nn.functional.softplus((1.0 - 2.0 * y64) * eta)
        else:
            l = y64 * eta - torch.exp(eta)
        k = float(l.shape[0])
        part = [torch.logsumexp(l, 0), torch.logsumexp(-l, 0), torch.logsumexp(-2.0 * l, 0), k, l.mean(0), torch.var(l, 0, unbiased=False) * k]
        if acc is None:
            acc = part
        else:
            n = acc[3] + k
            d = part[4] - acc[4]
            acc = [torch.logaddexp(acc[0], part[0]), torch.logaddexp(acc[1], part[1]), torch.logaddexp(acc[2], part[2]), n,
                   acc[4] + d * (k / n), acc[5] + part[5] + d * d * (acc[3] * k / n)]
    return acc


def main(argv):
    reps, rows, S, chunk, out_path, dims = 20, 1024, 250000, 32768, None, []
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--rows':
            rows = int(next(it))
        elif a == '--draws':
            S = int(next(it))
        elif a == '--chunk':
            chunk = int(next(it))
        elif a == '--out':
            out_path = next(it)
        else:
            dims.append(int(a))
    dims = dims or [20, 50]
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    def say(s):   # (line by line: a run that is cut short keeps what it measured)
        print(s, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(s + '\n')

    dev = torch.device('cuda', 0)
    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for D in dims:
        t = torch.from_numpy(pk.draws(S, D, D)).to(dev)
        for fam in gk.FAMILIES:
            like = gk.make_like(D, rows, fam, D)
            data = like.hip_like_glm
            spec, keep = flow.glm_spec(data, dev)
            G = int(_lib.load().nnest_glm_pointwise_groups(S, rows))
            stats = torch.empty(rows, 8, dtype=torch.float64, device=dev)
            partials = torch.empty(max(G, 1) * rows * 8, dtype=torch.float64, device=dev)
            A32 = keep[0][:, :rows].T.contiguous()
            o32, y64 = keep[2][:rows].contiguous(), keep[1][:rows].to(torch.float64)
            say('x_dim %d, n %d, %s, %d draws (%d draw groups; torch in chunks of %d)' % (D, rows, fam, S, G, chunk))
            sides = {'fused': lambda seed: fused(spec, t, stats, partials), 'torch': lambda seed: composed(fam, A32, o32, y64, t, chunk)}
            last = {}

            def fmt(name, mean, k, sd, se, out):
                last[name] = out
                return '  %-6s %9.3f ms per call (mean of %d; sd %.3f, se %.3f), %7.3f ns per (row, draw) pair' % (
                    name, mean, k, sd, se, 1e6 * mean / (float(S) * rows))

            m, e = alternate(sides, reps, say, fmt)
            ratio = m['torch'] / m['fused']
            say('  torch / fused: %.2fx +- %.2f' % (ratio, ratio * np.hypot(e['torch'] / m['torch'], e['fused'] / m['fused'])))
            f = pk.derived(last['fused'].cpu().numpy())
            c = [v.cpu().numpy() if torch.is_tensor(v) else v for v in last['torch']]
            say('  apart by at most: lppd %.3g, elpd_isloo %.3g, var %.3g (relative %.3g)' % (
                np.max(np.abs(f['lppd'] - (c[0] - np.log(S)))), np.max(np.abs(f['elpd_isloo'] + (c[1] - np.log(S)))),
                np.max(np.abs(f['var'] - c[5] / (S - 1.0))), np.max(np.abs(f['var'] - c[5] / (S - 1.0)) / f['var'])))


if __name__ == '__main__':
    main(sys.argv[1:])
