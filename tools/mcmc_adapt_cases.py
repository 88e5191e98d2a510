"""Developer tool, CPU only: chooses the seeds of the replay in tests/test_gpu_mcmc_adapt.py with the numpy restatement
(tests/mcmc_adapt_check.py) through the oracle's flows on the initialisation the GPU test uses -- the flows' default_init needs no
device.  Flow, width, walker offset, box and start scale are those of the mixed walk's replay (tools/mcmc_mixed_cases.py chose them;
tests/test_gpu_mcmc_mixed.py REPLAY has them); per case the first seed from 7000 + x_dim on for which, at C = 70, S = 8,
adapt_steps = 5, k = 3, adapt_rate 1 and target_accept 0.234, the restatement alone has at most 0.25 % of its 560 decisions within
ten times the lp tolerance of the threshold (the test allows 1 %), local proposals fall outside the box, local steps of the
adapting phase are both accepted and refused (so the walkers' steps spread), and of the global proposals at least 15 % are accepted
and at least 15 % refused.

Usage: python tools/mcmc_adapt_cases.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mcmc_mixed_cases as mm   # noqa: E402
from oracle import oracle as orc   # noqa: E402
from tests import mcmc_adapt_check as ac   # noqa: E402

C, S, K, ADAPT, RATE, TARGET = 70, 8, 3, 5, 1.0, 0.234
# (flow, x_dim, walker_offset): box, start scale -- the mixed walk's replay
CASES = {('nvp', 5, 0): (2.5, 0.5), ('nvp', 50, 1000): (3.0, 1.0), ('nvp', 70, 0): (3.0, 1.0), ('nvp', 100, 0): (4.0, 1.0),
         ('spline', 5, 0): (2.5, 1.0), ('spline', 40, 0): (2.5, 0.5)}


def stats(lp_fn, x_of_z, inb, z0, seed, offset, step, tol):
    D = z0.shape[1]
    eps, u = ac.mcmc_draws(seed, offset, C, 0, S, D)
    recs = []
    out = ac.adapt_run(z0, lp_fn(z0), [(eps[i], u[i]) for i in range(S)], float(np.float32(step)), lp_fn, K, ADAPT, RATE, TARGET, records=recs)
    hl, acc = out[3], out[7]
    border = out_local = acc_g = n_g = 0
    adapting = []
    for i, rec in enumerate(recs):
        lp_prev = lp_fn(z0) if i == 0 else hl[:, i - 1]
        with np.errstate(invalid='ignore'):
            m = 10.0 * tol(np.maximum(np.abs(np.where(np.isfinite(rec['lp_q']), rec['lp_q'], 0.0)),
                                      np.abs(np.where(np.isfinite(lp_prev), lp_prev, 0.0))))
            border += int((np.abs(rec['margin']) < m).sum())
        if ac.kind(i, K):
            acc_g += int(rec['accept'].sum())
            n_g += C
        else:
            out_local += int((~inb(x_of_z(rec['q'])[0])).sum())
            if i < ADAPT:
                adapting.append(acc[:, i])
    adapting = np.concatenate(adapting)
    return border / float(C * S), out_local, adapting.mean(), acc_g / float(max(1, n_g)), np.unique(out[4][:, -1]).size


def choose():
    for (name, D, offset), (half, scale) in CASES.items():
        sd, mu = mm.affine(D, D)
        # (x_dim > 50 has no recorded figure: the GPU test measures it; 1e-4 stands in for it here)
        tol = ((lambda v: 2e-5 + 1e-6 * np.abs(v)) if D <= 50 else (lambda v: 1e-4 + 0.0 * v)) if name == 'nvp' else (
            lambda v: mm.SPL_TOL * (1.0 + np.abs(v)))
        x0 = np.random.RandomState(D).normal(size=(C, D)).astype(np.float32) * scale
        if name == 'nvp':
            o, z0 = orc.NVP(D, 16, 3, 1, mm.nvp_weights(D, D)), x0
        else:
            o, z0 = mm.spline_oracle(D, D, x0)
        lp_fn, x_of_z, inb = mm.restated(o, sd, mu, half)
        found = None
        for seed in range(7000 + D, 7000 + D + 20):
            b, out_l, share, ag, distinct = stats(lp_fn, x_of_z, inb, z0, seed, offset, 1.0 / np.sqrt(D), tol)
            if b <= 0.0025 and out_l > 0 and 0.0 < share < 1.0 and 0.15 <= ag <= 0.85:
                found = (half, scale, seed, b, out_l, share, ag, distinct)
                break
        print(name, D, offset, 'box %.1f scale %.1f seed %d: borderline %.4f, local proposals outside %d, adapting acceptance %.3f, '
              'global acceptance %.3f, distinct final steps %d' % found if found else 'NOTHING FOUND')


if __name__ == '__main__':
    choose()
