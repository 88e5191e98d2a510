"""Developer tool, CPU only: chooses prior width, start scale and seed of the replay in tests/test_gpu_mcmc_glm_prior.py with the numpy
restatement (tests/mcmc_adapt_check.py for the walk, tests/glm_check.py for the likelihood, tests/gauss_prior_check.py for the prior
and the target) through the oracle's flows on the initialisation the GPU test uses, in the mould of tools/mcmc_glm_cases.py.  The
target of a case (flow, x_dim, walker_offset, n, family) is tests/glm_check.replay_target(x_dim, n, family) under
tests/gauss_prior_check.replay_prior(x_dim, width), seen through T = affine(D, D); no box.  Per case the first (width, start scale,
seed) -- widths 1, 2, 0.5, 4, 0.25 at scales 0.5 and 1, then, only where those find nothing, widths 1, 2, 0.5 at scales 1.5 and 2;
sixty seeds from 9000 + x_dim on -- for which, at C = 70, S = 8, adapt_steps = 5, k = 3,
adapt_rate 1 and target_accept 0.234, the restatement alone has at most 0.25 % of its 560 decisions within ten times the tolerance
in force of the threshold (the test allows 1 %), between 15 % and 85 % of the global proposals are accepted and between 10 % and
90 % of the local ones.  The tolerance in force is the flow's (x_dim > 50 has no recorded figure: the GPU test measures it; 1e-4
stands in for it here, and 1e-5 for the x tolerance) plus the likelihood's bound B, the prior's bound B_pi and the sensitivities of
both to the x tolerance.  Where nothing meets the 0.25 % the line says so and gives the best candidate seen.  That is
(spline, 40, 0, 40, poisson): the spline's lp tolerance is relative to |lp|, which the prior's D / 2 log 2 pi adds to, and a hand search
beyond this tool's lists (widths 0.25 to 4, scales up to 3, 240 seeds) found nothing under 3 of 560 (0.54 %) either; the test's table
records this tool's best, (0.5, 1.0, 9046), for it.

Usage: python tools/mcmc_glm_prior_cases.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mcmc_glm_cases as gcases   # noqa: E402
import mcmc_mixed_cases as mm   # noqa: E402
from oracle import oracle as orc   # noqa: E402
from tests import gauss_prior_check as pk   # noqa: E402
from tests import glm_check as gc   # noqa: E402
from tests import mcmc_adapt_check as ac   # noqa: E402

C, S, K, ADAPT, RATE, TARGET = gcases.C, gcases.S, gcases.K, gcases.ADAPT, gcases.RATE, gcases.TARGET
CASES = gcases.CASES   # (the replay's existing shape set: every U and NT the replays run)


def stats(rs, z0, seed, offset, step, tol, x_tol):
    D = z0.shape[1]
    eps, u = ac.mcmc_draws(seed, offset, C, 0, S, D)
    recs = []
    out = ac.adapt_run(z0, rs.lp(z0), [(eps[i], u[i]) for i in range(S)], float(np.float32(step)), rs.lp, K, ADAPT, RATE, TARGET, records=recs)
    hz, hl = out[2], out[3]
    border = acc_g = n_g = acc_l = n_l = 0
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
            acc_l += int(rec['accept'].sum())
            n_l += C
    return border / float(C * S), acc_l / float(n_l), acc_g / float(max(1, n_g)), np.unique(out[4][:, -1]).size


# (width, start scale) in the order tried: the first pass, then -- only where it finds nothing -- larger start scales
FIRST = [(w, sc) for w in (1.0, 2.0, 0.5, 4.0, 0.25) for sc in (0.5, 1.0)]
SECOND = [(w, sc) for w in (1.0, 2.0, 0.5) for sc in (1.5, 2.0)]


def choose_one(case):
    name, D, offset, n, family = case
    sd, mu = mm.affine(D, D)
    data = gc.replay_target(D, n, family)
    tol, x_tol = gcases.tolerances(name, D)
    found, best = None, None
    for width, scale in FIRST + SECOND:
        prior = pk.replay_prior(D, width)
        x0 = np.random.RandomState(D).normal(size=(C, D)).astype(np.float32) * scale
        if name == 'nvp':
            o, z0 = orc.NVP(D, 16, 3, 1, mm.nvp_weights(D, D)), x0
        else:
            o, z0 = mm.spline_oracle(D, D, x0)
        rs = pk.RestatedPrior(o, data, prior, sd, mu)
        for seed in range(9000 + D, 9000 + D + 60):
            b, al, ag, distinct = stats(rs, z0, seed, offset, 1.0 / np.sqrt(D), tol, x_tol)
            if 0.10 <= al <= 0.90 and 0.15 <= ag <= 0.85:
                if best is None or b < best[3]:
                    best = (width, scale, seed, b, al, ag, distinct)
                if b <= 0.0025:
                    found = best = (width, scale, seed, b, al, ag, distinct)
                    break
        if found:
            break
    line = ' width %.1f scale %.1f seed %d: borderline %.4f, local acceptance %.3f, global acceptance %.3f, distinct final steps %d'
    return ' '.join(str(v) for v in case) + (line % found if found else ' NOTHING FOUND; the best:' + (line % best if best else ' none'))


def choose():
    import multiprocessing
    with multiprocessing.Pool(min(len(CASES), 12)) as pool:
        for line in pool.imap(choose_one, CASES):
            print(line, flush=True)


if __name__ == '__main__':
    choose()
