"""Developer tool, CPU only: chooses box, start scale and seed of the replay in tests/test_gpu_mcmc_glm.py with the numpy restatement
(tests/mcmc_adapt_check.py for the walk, tests/glm_check.py for the likelihood) through the oracle's flows on the initialisation
the GPU test uses -- the flows' default_init needs no device.  The target of a case (flow, x_dim, walker_offset, n, family) is
tests/glm_check.replay_target(x_dim, n, family), seen through T = affine(D, D).  Per case the first (box, start scale, seed) -- boxes 2.5, 3, 4, 5, scales 0.5 and 1, sixty seeds from 8000 + x_dim
on -- for which, at C = 70, S = 8, adapt_steps = 5, k = 3, adapt_rate 1 and target_accept 0.234, the restatement alone has at most
0.25 % of its 560 decisions within ten times the lp tolerance in force of the threshold (the test allows 1 %), local proposals fall
outside the box, local steps of the adapting phase are both accepted and refused, and of the global proposals between 15 % and 85 %
are accepted.  The lp tolerance in force is the flow's (x_dim > 50 has no recorded figure: the GPU test measures it; 1e-4 stands in
for it here, and 1e-5 for the x tolerance) plus the likelihood's bound B plus its sensitivity to the x tolerance.

Usage: python tools/mcmc_glm_cases.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mcmc_mixed_cases as mm   # noqa: E402
from oracle import oracle as orc   # noqa: E402
from tests import glm_check as gc   # noqa: E402
from tests import mcmc_adapt_check as ac   # noqa: E402

C, S, K, ADAPT, RATE, TARGET = 70, 8, 3, 5, 1.0, 0.234
# n = 40: a ragged 64-row pass, three row blocks (the spline's wave 3 has none); n = 70: two passes and five blocks, the last of
# each ragged, so that the spline's waves hold 2, 1, 1 and 1.  The families alternate over the widths; |logL| -- and with it the
# flows' relative lp tolerance and the bound B, which grows with n and x_dim -- stays small enough for the 0.25 % to be reachable
CASES = [('nvp', 5, 0, 40, 'logistic'), ('nvp', 5, 0, 70, 'poisson'), ('nvp', 50, 1000, 70, 'poisson'), ('nvp', 50, 1000, 40, 'logistic'),
         ('nvp', 70, 0, 70, 'logistic'), ('nvp', 70, 0, 40, 'poisson'), ('nvp', 100, 0, 40, 'poisson'), ('nvp', 100, 0, 70, 'logistic'),
         ('spline', 5, 0, 40, 'poisson'), ('spline', 5, 0, 70, 'logistic'), ('spline', 40, 0, 70, 'logistic'), ('spline', 40, 0, 40, 'poisson')]


def tolerances(name, D):
    """(lp tolerance at value v, x tolerance at |x| = v) of the flow: tests/test_gpu_mcmc_mixed.py's"""
    if name == 'spline':
        return (lambda v: mm.SPL_TOL * (1.0 + np.abs(v))), (lambda v: mm.SPL_TOL * (1.0 + np.abs(v)))
    if D <= 50:
        return (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    return (lambda v: 1e-4 + 0.0 * v), (lambda v: 1e-5 + 0.0 * v)


def stats(rs, z0, seed, offset, step, tol, x_tol):
    D = z0.shape[1]
    eps, u = ac.mcmc_draws(seed, offset, C, 0, S, D)
    recs = []
    out = ac.adapt_run(z0, rs.lp(z0), [(eps[i], u[i]) for i in range(S)], float(np.float32(step)), rs.lp, K, ADAPT, RATE, TARGET, records=recs)
    hz, hl, acc = out[2], out[3], out[7]
    border = out_local = acc_g = n_g = 0
    adapting = []
    for i, rec in enumerate(recs):
        z_prev = z0 if i == 0 else hz[:, i - 1]
        lp_prev = rs.lp(z0) if i == 0 else hl[:, i - 1]
        xq, xp = rs.x_of_z(rec['q'])[0], rs.x_of_z(z_prev)[0]
        like = np.maximum(rs.like_tol(xq, x_tol(np.max(np.abs(xq), axis=1))), rs.like_tol(xp, x_tol(np.max(np.abs(xp), axis=1))))
        with np.errstate(invalid='ignore'):
            m = 10.0 * (tol(np.maximum(np.abs(np.where(np.isfinite(rec['lp_q']), rec['lp_q'], 0.0)),
                                       np.abs(np.where(np.isfinite(lp_prev), lp_prev, 0.0)))) + np.where(np.isfinite(like), like, 0.0))
            border += int((np.abs(rec['margin']) < m).sum())
        if ac.kind(i, K):
            acc_g += int(rec['accept'].sum())
            n_g += C
        else:
            out_local += int((~rs.in_prior(xq)).sum())
            if i < ADAPT:
                adapting.append(acc[:, i])
    adapting = np.concatenate(adapting)
    return border / float(C * S), out_local, adapting.mean(), acc_g / float(max(1, n_g)), np.unique(out[4][:, -1]).size


def choose_one(case):
    name, D, offset, n, family = case
    sd, mu = mm.affine(D, D)
    data = gc.replay_target(D, n, family)
    tol, x_tol = tolerances(name, D)
    found = None
    for half in (2.5, 3.0, 4.0, 5.0):
        for scale in (0.5, 1.0):
            x0 = np.random.RandomState(D).normal(size=(C, D)).astype(np.float32) * scale
            if name == 'nvp':
                o, z0 = orc.NVP(D, 16, 3, 1, mm.nvp_weights(D, D)), x0
            else:
                o, z0 = mm.spline_oracle(D, D, x0)
            rs = gc.Restated(o, data, sd, mu, half)
            for seed in range(8000 + D, 8000 + D + 60):
                b, out_l, share, ag, distinct = stats(rs, z0, seed, offset, 1.0 / np.sqrt(D), tol, x_tol)
                if b <= 0.0025 and out_l > 0 and 0.0 < share < 1.0 and 0.15 <= ag <= 0.85:
                    found = (half, scale, seed, b, out_l, share, ag, distinct)
                    break
            if found:
                break
        if found:
            break
    return ' '.join(str(v) for v in case) + (' box %.1f scale %.1f seed %d: borderline %.4f, local proposals outside %d, adapting acceptance %.3f, '
                                             'global acceptance %.3f, distinct final steps %d' % found if found else ' NOTHING FOUND')


def choose():
    import multiprocessing
    with multiprocessing.Pool(min(len(CASES), 12)) as pool:
        for line in pool.imap(choose_one, CASES):
            print(line, flush=True)


if __name__ == '__main__':
    choose()
