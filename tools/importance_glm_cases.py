"""Developer tool, CPU only: chooses box and seed of the cases in tests/test_gpu_importance_glm.py with the numpy restatement
(tests/importance_glm_check.py) through the oracle's flows on the initialisation the GPU test uses -- the flows' default_init needs
no device.  The target of a case (flow, x_dim, n, family, sample_offset) is tests/glm_check.replay_target(x_dim, n, family), seen
through T = affine(D, D).  M is what the GPU test launches on the 256 compute units of an MI355X: 2 * tile * groups + 5 (NVP: tile 4,
4 workgroups a compute unit) or + 7 (spline: tile 16, 2 a compute unit).  Per case the first (box, seed) -- boxes 2.5, 3, 4, 5, 1.5, 1,
twenty seeds from 7300 + x_dim on -- for which the restatement alone has at most 0.25 % of its M live / dead verdicts hanging on a
coordinate of T(x) within ten times the x tolerance in force of a face of the box (the test allows 1 %), and both live and dead
samples, at least 2 % of each.  The x tolerance in force is the flow's (x_dim > 50 has no recorded figure: the GPU test measures it;
1e-5 stands in for it here).

Usage: python tools/importance_glm_cases.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mcmc_mixed_cases as mm   # noqa: E402
from oracle import oracle as orc   # noqa: E402
from tests import glm_check as gc   # noqa: E402
from tests import importance_glm_check as igc   # noqa: E402

NUM_CU = 256
BIG = (3 << 32) + 5   # a sample_offset beyond 2^32
# the flow widths of tests/test_gpu_mcmc_glm.py's REPLAY table, its rows and families
CASES = [('nvp', 5, 40, 'logistic', 0), ('nvp', 5, 70, 'poisson', BIG), ('nvp', 50, 70, 'poisson', 1000), ('nvp', 50, 40, 'logistic', BIG),
         ('nvp', 70, 70, 'logistic', 0), ('nvp', 70, 40, 'poisson', BIG), ('nvp', 100, 40, 'poisson', BIG), ('nvp', 100, 70, 'logistic', 0),
         ('spline', 5, 40, 'poisson', BIG), ('spline', 5, 70, 'logistic', 0), ('spline', 40, 70, 'logistic', BIG), ('spline', 40, 40, 'poisson', 0)]


def launch_size(name):
    return 2 * 4 * (4 * NUM_CU) + 5 if name == 'nvp' else 2 * 16 * (2 * NUM_CU) + 7


def x_tolerance(name, D):
    if name == 'spline':
        return lambda v: mm.SPL_TOL * (1.0 + np.abs(v))
    return (lambda v: 5e-5 + 0.0 * v) if D <= 50 else (lambda v: 1e-5 + 0.0 * v)


def oracle_flow(name, D):
    """the oracle on the weights of tests/test_gpu_importance.nvp_and_oracle(D, D) / spline_and_oracle(D, D)"""
    if name == 'nvp':
        return orc.NVP(D, 16, 3, 1, mm.nvp_weights(D, D))
    return mm.spline_oracle(D, D, np.random.RandomState(D).normal(size=(40, D)).astype(np.float32) * 0.5)[0]


def choose_one(case):
    name, D, n, family, off = case
    M = launch_size(name)
    sd, mu = mm.affine(D, D)
    data = gc.replay_target(D, n, family)
    o = oracle_flow(name, D)
    x_tol = x_tolerance(name, D)
    found = None
    for seed in range(7300 + D, 7300 + D + 20):
        z = igc.importance_draws(seed, off, M, D)
        x, _ = o.inverse(z)
        m = 10.0 * float(np.max(x_tol(np.abs(x))))
        for half in (2.5, 3.0, 4.0, 5.0, 1.5, 1.0):
            rs = igc.restated(o, data, sd, mu, half=half)
            border = float(igc.near_face(rs, x, m).mean())
            live = float(rs.in_prior(x).mean())
            if border <= 0.0025 and 0.02 <= live <= 0.98:
                found = (half, seed, border, live)
                break
        if found:
            break
    return ' '.join(str(v) for v in case) + (' box %.1f seed %d: borderline %.4f, live %.3f' % found if found else ' NOTHING FOUND')


def choose():
    import multiprocessing
    with multiprocessing.Pool(min(len(CASES), 8)) as pool:
        for line in pool.imap(choose_one, CASES):
            print(line, flush=True)


if __name__ == '__main__':
    choose()
