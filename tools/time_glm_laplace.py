"""Developer diagnostic: GLMData.laplace on the fused route (nnest_glm_curv + nnest_glm_newton_solve per trial) against the host route
of the same build -- float64 numpy, the only route there was before the kernels, restated -- per (n, x_dim) and family under the
tests' prior, and ONE nnest_glm_curv call alone:
   fused   like.laplace(prior, route='fused'): the data staged to the device inside the call, one curvature launch pair, one solve
           and one read of four doubles per trial;
   host    like.laplace(prior, route='host');
   curv    `--calls` back-to-back nnest_glm_curv calls into preallocated buffers between two device events, per call; beside it the
           share of the float64 matrix peak: the flops of the upper triangle and the gradient, n (D (D + 1) + 2 D), and the flops the
           MFMAs issue (whole 16 x 16 tiles), over the time, against CUs x clock x 128 flop per CU and cycle (v_mfma_f64_16x16x4_f64
           is 2048 flop in 16 passes of 4 cycles on one of a CU's four matrix cores).
The sides alternate in one process: after a warm-up of each, `reps` rounds, each call timed by a host clock around work that ends in
a device synchronise.  Printed per side: the mean, the standard deviation and the standard error of the mean; per case the ratio of
the means with its standard error (first order, from the two standard errors), and how far the two routes' modes and log Z are
apart.  There is no pass/fail ratio: the figures are recorded.
   python tools/time_glm_laplace.py [--reps R] [--calls K] [--out FILE] [n x_dim] ...
   (default: --reps 20 --calls 50, (n, x_dim) = (1024, 20), (1024, 50), (65536, 128); --out appends the report to FILE, e.g.
   profiles/glm_laplace/summary.txt)"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nnest_amd import _lib, flow  # noqa: E402
from nnest_amd.priors import GaussianPrior  # noqa: E402
from tests import glm_check as gk  # noqa: E402
from time_mcmc_glm import alternate  # noqa: E402


def curv_alone(data, D, calls, dev):
    """(ms per call, G) of `calls` back-to-back nnest_glm_curv calls"""
    lib = _lib.load()
    spec, keep = flow.glm_spec(data, dev)
    G = int(lib.nnest_glm_curv_groups(int(data['n']), D))
    theta = torch.zeros(D, dtype=torch.float64, device=dev)
    out = torch.empty(1 + D + D * D, dtype=torch.float64, device=dev)
    partials = torch.empty(G * (1 + D + D * (D + 1) // 2), dtype=torch.float64, device=dev)
    st = _lib.current_stream(dev)

    def run(k):
        for _ in range(k):
            _lib.check(lib.nnest_glm_curv(ctypes.byref(spec), _lib.ptr(theta), _lib.ptr(out), _lib.ptr(partials), D, st))

    run(3)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    run(calls)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls, G


def main(argv):
    reps, calls, out_path, nums = 20, 50, None, []
    it = iter(argv)
    for a in it:
        if a == '--reps':
            reps = int(next(it))
        elif a == '--calls':
            calls = int(next(it))
        elif a == '--out':
            out_path = next(it)
        else:
            nums.append(int(a))
    shapes = list(zip(nums[0::2], nums[1::2])) or [(1024, 20), (1024, 50), (65536, 128)]
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    def say(s):   # (line by line: a run that is cut short keeps what it measured)
        print(s, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(s + '\n')

    dev = torch.device('cuda', 0)
    info = _lib.device_info()
    peak = info['num_cu'] * info['clock_khz'] * 1e3 * 128.0
    say('%s, torch %s; %d CUs at %.0f MHz: float64 matrix peak %.1f Tflop/s' % (torch.cuda.get_device_name(0), torch.__version__, info['num_cu'],
                                                                             info['clock_khz'] / 1e3, peak / 1e12))
    for n, D in shapes:
        prior = GaussianPrior(D, np.linspace(-0.2, 0.3, D), np.linspace(1.0, 1.5, D))
        for fam in gk.FAMILIES:
            like = gk.make_like(D, n, fam, D + n)
            ms, G = curv_alone(like.hip_like_glm, D, calls, dev)
            NT = (D + 15) // 16
            useful, issued = n * (D * (D + 1) + 2.0 * D), (n / 4.0) * (NT * (NT + 1) // 2 + NT) * 2048.0
            say('n %d, x_dim %d, %s (%d row groups)' % (n, D, fam, G))
            say('  curv   %9.4f ms per nnest_glm_curv call (mean of %d back to back): %.2f %% of the float64 matrix peak in useful flops, '
                '%.2f %% in issued ones' % (ms, calls, 100.0 * useful / (ms * 1e-3) / peak, 100.0 * issued / (ms * 1e-3) / peak))
            sides = {'fused': lambda seed: like.laplace(prior=prior, route='fused'), 'host': lambda seed: like.laplace(prior=prior, route='host')}
            last = {}

            def fmt(name, mean, k, sd, se, out):
                last[name] = out
                return '  %-6s %9.3f ms per fit (mean of %d; sd %.3f, se %.3f), %d Newton iterations, %d halvings' % (
                    name, mean, k, sd, se, out.iterations, out.halvings)

            m, e = alternate(sides, reps, say, fmt)
            ratio = m['host'] / m['fused']
            say('  host / fused: %.2fx +- %.2f' % (ratio, ratio * np.hypot(e['host'] / m['host'], e['fused'] / m['fused'])))
            say('  apart by: mode %.3g (2-norm), log Z %.3g' % (np.linalg.norm(last['fused'].mode - last['host'].mode),
                                                                abs(last['fused'].logz - last['host'].logz)))


if __name__ == '__main__':
    main(sys.argv[1:])
