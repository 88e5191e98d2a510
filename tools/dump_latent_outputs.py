#!/usr/bin/env python3
"""Dump what the fused latent-target kernels compute (developer tool): the ensemble, x-space ensemble, random-walk Metropolis and
importance kernels of both flows (solo_latent.h, spline_latent.h), at every instantiated shape and with every likelihood, so that
two builds can be compared bit for bit.

  python tools/dump_latent_outputs.py DIR          (NNEST_HIP_LIB selects the library, nnest_amd/_lib.py)
  python tools/compare_k4_outputs.py PARENT_DIR TREE_DIR [--out report.txt]

DIR receives one sub-directory of .npy files per case, every output array of the call.  Cases (small: the whole dump runs in
seconds): 37 walkers -- a partial workgroup and a partial 16-tile -- and 6 steps; the NVP at x_dim 5, 50, 70, 100 (U = 1 .. 4, each
with padded dims); the spline at the six (NTh, NH) keys, at the dims of tests/test_gpu_fused_likes.py; the seven likelihoods of
tests/fused_like_check.py with its recipes for T, a box on every case, start row 1 outside the box, start row 2 with a NaN.
Per case: the ensemble (the stretch move, and for the NVP the stretch / DE mixture; constrained 0 and 1, loglstar the median of the
start's logL), the random walk (untempered and at beta = 0.37; lp given and evaluated; steps = 0) and the importance run (M = 100
with the samples, sample_offset != 0).  The x-space ensemble runs at the NVP's cases, with T and without.
The walks behind the random walk run at the same cases and, on the data likelihoods, at every shape:
the mixed walk (global_every 3), the adaptive walk (adapt_steps below and above the 6 steps, step_in given and None, hist_step), each
also as one launch cut in two with lp, logL and the steps handed on; on the Gaussian likelihood from data, on both regression
families and on those under normal priors (the targets of tools/mcmc_gdata_cases.py, mcmc_glm_cases.py, mcmc_glm_prior_cases.py:
tests/gdata_check.replay_target, tests/glm_check.replay_target, tests/gauss_prior_check.replay_prior).  The three stand-alone kernels
(loglike_gdata, loglike_glm, logprior_gauss) run at D = 1, 31, 32, 33, 65, 128."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnest_amd import flow  # noqa: E402
from nnest_amd.spline import HipSpline  # noqa: E402
from tests import fused_like_check as fl  # noqa: E402
from tests import gauss_prior_check as pk  # noqa: E402
from tests import gdata_check as gd  # noqa: E402
from tests import glm_check as gk  # noqa: E402

C, S, M, BETA, OFFSET = 37, 6, 100, 0.37, 12345
MIX = {'stretch': 0.5, 'de': 0.5}
EVERY, CUT = 3, 3   # the mixed walk's global_every; where the launch cut in two is cut
GLMS = ((40, 'logistic'), (70, 'poisson'))   # (n, family) of the regression targets, as tools/mcmc_glm_cases.py pairs them
ALONE_DIMS = (1, 31, 32, 33, 65, 128)
# (likelihood, recipe, x_dim): Rosenbrock (compiled in) and a generic likelihood at every U, all seven likelihoods
NVP_CASES = [('rosenbrock', 'valley', 5), ('rosenbrock', 'wide', 50), ('rosenbrock', 'valley', 70), ('rosenbrock', 'valley', 100),
             ('shell', 'main', 5), ('gaussmix', 'main', 50), ('himmelblau', 'main', 70), ('double_shell', 'main', 100),
             ('gaussian', 'main', 100), ('eggbox', 'main', 2)]
# (likelihood, recipe, x_dim, hidden): Rosenbrock and a generic likelihood at every key (tests/test_gpu_fused_likes.py SPLINE_KEYS)
SPLINE_CASES = [('rosenbrock', 'valley', 5, 16), ('rosenbrock', 'valley', 40, 16), ('rosenbrock', 'valley', 70, 16),
                ('rosenbrock', 'valley', 128, 16), ('rosenbrock', 'valley', 8, 32), ('rosenbrock', 'valley', 40, 32),
                ('gaussmix', 'main', 5, 16), ('shell', 'main', 40, 16), ('himmelblau', 'main', 70, 16), ('gaussian', 'main', 128, 16),
                ('double_shell', 'main', 8, 32), ('gaussian', 'main', 40, 32), ('eggbox', 'main', 2, 16)]


def start_x(D, sd, mu, lo, hi):
    """x ~ 0.5 N(0, 1); row 1 outside the box; row 2, well inside it in every other coordinate, holds a NaN"""
    x0 = (np.random.RandomState(D).normal(size=(C, D)) * 0.5).astype(np.float32)
    x0[1, D - 1] = (hi[D - 1] + (hi[D - 1] - lo[D - 1]) - mu[D - 1]) / sd[D - 1]
    x0[2] = x0[2] * np.float32(0.25)
    x0[2, 0] = np.nan
    return x0


class Dump(object):
    def __init__(self, root):
        self.root, self.n = root, 0

    def __call__(self, case, call, res):
        d = os.path.join(self.root, '%s__%s' % (case, call))
        os.makedirs(d)
        for k, v in res.items():
            if torch.is_tensor(v):
                np.save(os.path.join(d, k + '.npy'), v.cpu().numpy())
                self.n += 1
        return res


def median_logl(logl):
    v = logl.cpu().numpy()
    return float(np.median(v[np.isfinite(v) & (v > fl.SAFE)]))


def latent_case(dump, case, net, like_id, params, D, sd, mu, lo, hi, mixes):
    kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, like_params=params)
    z0 = net.forward(start_x(D, sd, mu, lo, hi))[0].contiguous()
    step = 1.0 / np.sqrt(D)
    begin = dump(case, 'mcmc-s0', net.mcmc_steps(like_id, z0, 0, step, seed=11, **kw))
    star = median_logl(begin['logl'])
    dump(case, 'mcmc', net.mcmc_steps(like_id, z0, S, step, seed=11, **kw))
    dump(case, 'mcmc-lp', net.mcmc_steps(like_id, z0, S, step, lp=begin['lp'], logl=begin['logl'], seed=12, step0=3, walker_offset=5, **kw))
    t0 = dump(case, 'mcmc-b-s0', net.mcmc_steps(like_id, z0, 0, step, seed=13, beta=BETA, **kw))
    dump(case, 'mcmc-b', net.mcmc_steps(like_id, z0, S, step, seed=13, beta=BETA, **kw))
    dump(case, 'mcmc-b-lp', net.mcmc_steps(like_id, z0, S, step, lp=t0['lp'], logl=t0['logl'], seed=14, beta=BETA, **kw))
    for tag, moves in mixes:
        dump(case, 'ens-%s' % tag, net.ensemble_steps(like_id, z0, S, seed=21, moves=moves, **kw))
        dump(case, 'ens-%s-c' % tag, net.ensemble_steps(like_id, z0, S, seed=22, moves=moves, loglstar=star, **kw))
    dump(case, 'ens-s0', net.ensemble_steps(like_id, z0, 0, seed=21, **kw))
    dump(case, 'imp', net.importance_evidence(like_id, M, seed=31, sample_offset=OFFSET, want_samples=True, **kw))
    dump(case, 'imp-sums', net.importance_evidence(like_id, M, seed=32, **kw))
    walk_case(dump, case, net, like_id, z0, step, **kw)
    return star


def walk_case(dump, case, net, like_id, z0, step, **kw):
    """the mixed and the adaptive walk on one target (kw: T, the box, and like_params or a data likelihood's descriptors)"""
    C = z0.shape[0]
    step_in = torch.as_tensor(step * np.linspace(0.5, 2.0, C), dtype=torch.float64, device=z0.device)
    runs = (('mixed', dict(global_every=EVERY, beta=BETA)),
            ('adapt-lo', dict(global_every=EVERY, adapt_steps=S - 2)),
            ('adapt-hi-in', dict(global_every=EVERY, beta=BETA, adapt_steps=S + 4, step_in=step_in)),
            ('adapt-in', dict(step_in=step_in)))
    for tag, opts in runs:
        dump(case, tag, net.mcmc_steps(like_id, z0, S, step, seed=51, walker_offset=5, **opts, **kw))
        # the same launch cut in two: the state handed on (the second half must be the first run's second half)
        a = dump(case, tag + '-cut1', net.mcmc_steps(like_id, z0, CUT, step, seed=51, walker_offset=5, **opts, **kw))
        rest = dict(opts, step_in=a['step']) if 'step' in a else opts
        dump(case, tag + '-cut2', net.mcmc_steps(like_id, a['z'], S - CUT, step, lp=a['lp'], logl=a['logl'], seed=51, walker_offset=5,
                                                 step0=CUT, **rest, **kw))


def data_cases(dump, case, net, D):
    """the walks on the data likelihoods at one shape, and their start evaluated (steps = 0)"""
    r = np.random.RandomState(D)
    sd, mu = r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)
    lo, hi = np.full(D, -4.0, np.float32), np.full(D, 4.0, np.float32)
    z0 = net.forward(start_x(D, sd, mu, lo, hi))[0].contiguous()
    step = 1.0 / np.sqrt(D)
    targets = [('gdata', dict(like_data=gd.replay_target(D)))]
    for n, family in GLMS:
        glm = gk.replay_target(D, n, family)
        targets.append(('glm-%s' % family, dict(like_glm=glm)))
        targets.append(('glmp-%s' % family, dict(like_glm=glm, prior_gauss=pk.replay_prior(D, 1.0).hip_gauss_prior)))
    for tag, like in targets:
        kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, **like)
        dump(case + '-' + tag, 's0', net.mcmc_steps(None, z0, 0, step, seed=51, **kw))
        walk_case(dump, case + '-' + tag, net, None, z0, step, **kw)


def alone_cases(dump):
    """the likelihoods and the prior alone, on rows that are already T(x)"""
    for D in ALONE_DIMS:
        t = (np.random.RandomState(D).normal(size=(C, D)) * 0.7).astype(np.float32)
        t[2, 0] = np.nan
        dump('alone-%d' % D, 'gdata', {'logl': flow.loglike_gdata(gd.replay_target(D), t)})
        for n, family in GLMS:
            dump('alone-%d' % D, 'glm-%s' % family, {'logl': flow.loglike_glm(gk.replay_target(D, n, family), t)})
        dump('alone-%d' % D, 'prior', {'logp': flow.logprior_gauss(pk.replay_prior(D, 1.0).hip_gauss_prior, t)})


def x_case(dump, case, like_id, params, D, sd, mu, lo, hi, star):
    x0 = start_x(D, sd, mu, lo, hi)
    for ttag, kw in (('T', dict(t_std=sd, t_mean=mu, lo=lo, hi=hi)), ('id', dict(lo=lo, hi=hi))):
        for tag, moves in (('st', None), ('mix', MIX)):
            dump(case, 'x%s-%s' % (ttag, tag), flow.ensemble_x_steps(like_id, x0, S, seed=41, moves=moves, like_params=params, **kw))
            dump(case, 'x%s-%s-c' % (ttag, tag), flow.ensemble_x_steps(like_id, x0, S, seed=42, moves=moves, loglstar=star, like_params=params, **kw))


def main():
    root = sys.argv[1]
    os.makedirs(root)
    torch.cuda.set_device(0)
    dump = Dump(root)
    for name, recipe, D in NVP_CASES:
        e = fl.LIKES[name]
        sd, mu = fl.affine(name, recipe, D, D)
        lo, hi = fl.box_for(sd, mu)
        case = 'nvp-%s-%s-%d' % (name, recipe, D)
        star = latent_case(dump, case, flow.HipNVP(D, 16, 3, 1, seed=D), e['id'], e['params'], D, sd, mu, lo, hi, (('st', None), ('mix', MIX)))
        x_case(dump, case, e['id'], e['params'], D, sd, mu, lo, hi, star)
    for D in (5, 50, 70, 100):   # (U = 1 .. 4)
        data_cases(dump, 'nvp-data-%d' % D, flow.HipNVP(D, 16, 3, 1, seed=D), D)
    for name, recipe, D, H in SPLINE_CASES:
        e = fl.LIKES[name]
        sd, mu = fl.affine(name, recipe, D, D)
        lo, hi = fl.box_for(sd, mu)
        sp = HipSpline(D, H, 3, seed=D + H)
        sp.forward((np.random.RandomState(D + H).normal(size=(40, D)) * 0.5).astype(np.float32))   # (sets the ActNorm layers)
        latent_case(dump, 'spl-%s-%s-%d-%d' % (name, recipe, D, H), sp, e['id'], e['params'], D, sd, mu, lo, hi, (('st', None),))
    for D, H in sorted(set((D, H) for _, _, D, H in SPLINE_CASES if D > 2)):   # (the six keys)
        sp = HipSpline(D, H, 3, seed=D + H)
        sp.forward((np.random.RandomState(D + H).normal(size=(40, D)) * 0.5).astype(np.float32))
        data_cases(dump, 'spl-data-%d-%d' % (D, H), sp, D)
    alone_cases(dump)
    print('%d arrays under %s' % (dump.n, root))


if __name__ == '__main__':
    main()
