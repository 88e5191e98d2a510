"""Developer diagnostic: Pareto-smoothed leave-one-out of the regression likelihoods (nnest_glm_psis) against what it costs to
stream the draws once and against the route composed from this build, per x_dim and family, at n data rows and S draws that are on
the device already:
   psis       one call of nnest_glm_psis (three digit passes and their selects, the collect pass, the fit) on the statistics of a
              nnest_glm_pointwise call made beforehand, into a preallocated result and work buffer;
   pointwise  one call of nnest_glm_pointwise: the price of ONE streaming pass with its float64 reduction;
   composed   nnest_glm_terms into a preallocated [S, n] float64 matrix, then torch.topk of the M* smallest terms per data row
              (largest = False, sorted): the selection alone -- no body sums, no fit -- and the matrix is what it cannot avoid.
The sides alternate in one process: after a warm-up of each, `reps` rounds, each call timed by a host clock around work that ends in
a device synchronise.  Printed per side: the mean, the standard deviation and the standard error of the mean; per case the ratios of
the means.  There is no pass/fail ratio: the figures are recorded.
   python tools/time_glm_psis.py [--reps R] [--rows N] [--draws S] [--out FILE] [x_dim] ...
   (default: --reps 20 --rows 1024 --draws 250000, x_dim 20 and 50; --out appends the report to FILE, e.g.
   profiles/glm_psis/summary.txt)"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nnest_amd import _lib, flow, psis  # noqa: E402
from tests import glm_check as gk  # noqa: E402
from tests import glm_pointwise_check as pk  # noqa: E402
from time_mcmc_glm import alternate  # noqa: E402


def main(argv):
    reps, rows, S, out_path, dims = 20, 1024, 250000, None, []
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--rows':
            rows = int(next(it))
        elif a == '--draws':
            S = int(next(it))
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

    lib = _lib.load()
    dev = torch.device('cuda', 0)
    say('%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    target = psis.tail_target(S)
    for D in dims:
        t = torch.from_numpy(pk.draws(S, D, D)).to(dev)
        for fam in gk.FAMILIES:
            data = gk.make_like(D, rows, fam, D).hip_like_glm
            spec, keep = flow.glm_spec(data, dev)
            G = int(lib.nnest_glm_pointwise_groups(S, rows))
            stats = torch.empty(rows, 8, dtype=torch.float64, device=dev)
            partials = torch.empty(max(G, 1) * rows * 8, dtype=torch.float64, device=dev)
            out = torch.empty(rows, 16, dtype=torch.float64, device=dev)
            work = torch.empty(int(lib.nnest_glm_psis_work_bytes(S, rows)), dtype=torch.uint8, device=dev)
            terms = torch.empty(S, rows, dtype=torch.float64, device=dev)
            stream = _lib.current_stream(dev)

            def pointwise(seed):
                _lib.check(lib.nnest_glm_pointwise(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(stats), _lib.ptr(partials), S, D, stream))
                return stats

            def smoothed(seed):
                _lib.check(lib.nnest_glm_psis(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(stats), _lib.ptr(out), _lib.ptr(work), S, D, stream))
                return out

            def composed(seed):
                _lib.check(lib.nnest_glm_terms(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(terms), S, D, stream))
                return torch.topk(terms, target, dim=0, largest=False, sorted=True).values

            pointwise(0)
            say('x_dim %d, n %d, %s, %d draws (%d draw groups; M* = %d, work %.1f MB, the matrix %.1f MB)' % (
                D, rows, fam, S, G, target, work.numel() / 1e6, terms.numel() * 8 / 1e6))
            last = {}

            def fmt(name, mean, k, sd, se, res):
                last[name] = res
                return '  %-9s %9.3f ms per call (mean of %d; sd %.3f, se %.3f), %7.3f ns per (row, draw) pair' % (
                    name, mean, k, sd, se, 1e6 * mean / (float(S) * rows))

            m, e = alternate({'psis': smoothed, 'pointwise': pointwise, 'composed': composed}, reps, say, fmt)
            for a, b in (('psis', 'pointwise'), ('composed', 'psis')):
                r = m[a] / m[b]
                say('  %s / %s: %.2fx +- %.2f' % (a, b, r, r * np.hypot(e[a] / m[a], e[b] / m[b])))
            o = last['psis'].cpu().numpy()
            k = o[:, psis.KHAT]
            say('  khat: median %.3f, max %.3f; tails %d .. %d; flags %s' % (
                np.median(k), np.max(k), o[:, psis.M].min(), o[:, psis.M].max(), sorted(set(int(v) for v in o[:, psis.FLAG]))))
            del terms, work


if __name__ == '__main__':
    main(sys.argv[1:])
