#!/usr/bin/env python3
"""Dump what the front ends return on their fused routes (developer tool), so that two states of the Python layer can be compared
bit for bit against the same library -- the companion of tools/dump_latent_outputs.py one level up.

  python tools/dump_front_ends.py DIR          (NNEST_HIP_LIB selects the library, nnest_amd/_lib.py)
  python tools/compare_k4_outputs.py PARENT_DIR TREE_DIR [--out report.txt]

DIR receives one sub-directory of .npy files per case: every array the front end returns or leaves, and its counters.  The flows keep
their seed-initialised weights (trainer.train is a no-op here: the comparison does not rest on training), the seeds are fixed.
Flows: the NVP at x_dim 5 and 70 (a second NT), the spline at x_dim 5; a Gaussian likelihood in a box.  Per flow:
  mcmc        MCMCSampler.run(route='fused'): 37 chains x 7 steps, launches of 3 steps (ENSEMBLE_HISTORY_BYTES), output_interval 2
  ens-fused   EnsembleSampler.run(route='fused'), ens-rounds: route='rounds': 37 walkers x 7 steps, launches of 3 steps
  boot        EnsembleSampler.bootstrap's x-space run (`_ensemble_sample_x`, as bootstrap calls it: T = identity), launches of 3 steps
  imp         importance_evidence(100, chunk=37, return_samples=True, route='fused')
  smc         SMCSampler.run(route='fused'): 64 particles x 3 steps
37 walkers (141 for the ensemble at x_dim 70, which asks for two per dimension): a partial workgroup and a partial 16-tile; 7 steps
in launches of 3, and for the Metropolis run saves every 2: both cuts happen."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnest_amd  # noqa: E402
from nnest_amd import likelihoods  # noqa: E402
from nnest_amd.priors import UniformPrior  # noqa: E402
from nnest_amd.trainer import Trainer  # noqa: E402

N, S, CHUNK, M, PARTICLES = 37, 7, 3, 100, 64
FLOWS = (('nvp', 5), ('nvp', 70), ('spline', 5))


def sampler(cls, flow, D, tmp, walkers=N):
    """a front end on a flow with seed-initialised weights that no call trains"""
    np.random.seed(D)
    torch.manual_seed(D)
    trainer = Trainer(D, flow=flow, log_dir=tmp, log=False, seed=D, log_level=30)
    trainer.train = lambda *a, **kw: None
    s = cls(D, likelihoods.Gaussian(D, 0.5), prior=UniformPrior(D, -6.0, 6.0), trainer=trainer, log_dir=tmp, log_level=30)
    s.ENSEMBLE_HISTORY_BYTES = CHUNK * walkers * (8 * D + 8)   # (launches of CHUNK steps)
    trainer.netG.forward(np.random.RandomState(D).normal(size=(40, D)).astype(np.float32))   # (the spline: sets the ActNorm layers)
    return s


def dump(root, case, s, run):
    """run() -> the case's arrays; a route that refuses the case (ValueError) is recorded by its words"""
    d = os.path.join(root, case)
    os.makedirs(d)
    try:
        arrays = run()
    except ValueError as e:
        arrays = dict(refused=str(e))
    arrays['counters'] = np.array([s.total_calls, s.total_accepted, s.total_rejected], np.int64)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + '.npy'), np.asarray(v))
    return len(arrays)


def chains(s):
    return dict(samples=s.samples, latent=s.latent_samples, loglikes=s.loglikes)


def main():
    root = sys.argv[1]
    os.makedirs(root)
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp()
    n = 0
    for flow, D in FLOWS:
        tag = '%s-%d' % (flow, D)
        train = np.random.RandomState(1).normal(size=(200, D)) * 0.8 + 0.3
        W = N if N >= 2 * D else 2 * D + 1   # (the stretch move asks for two walkers per dimension: 141 at x_dim 70)
        s = sampler(nnest_amd.MCMCSampler, flow, D, tmp)
        n += dump(root, tag + '__mcmc', s, lambda: (s.run(S, N, train, output_interval=2, route='fused', seed=3), chains(s))[1])
        n += dump(root, tag + '__imp', s, lambda: {k: v for k, v in s.importance_evidence(
            M, seed=4, chunk=37, return_samples=True, route='fused').items() if k != 'route'})
        for route in ('fused', 'rounds'):
            s = sampler(nnest_amd.EnsembleSampler, flow, D, tmp, W)
            np.random.seed(5)
            torch.manual_seed(5)   # (`_next_seed`: the run's Philox seed)
            n += dump(root, tag + '__ens-' + route, s, lambda: (s.run(S, W, train, route=route), chains(s))[1])
            assert getattr(s, 'ensemble_route', route) == route
        s = sampler(nnest_amd.EnsembleSampler, flow, D, tmp, W)
        x0 = np.random.RandomState(2).uniform(-1, 1, size=(W, D))
        n += dump(root, tag + '__boot', s, lambda: dict(zip(('chain', 'loglikes', 'derived', 'ncall'),
                                                            s._ensemble_sample_x(S, x0, output_interval=2, seed=6, route='fused'))))
        s = sampler(nnest_amd.SMCSampler, flow, D, tmp)
        np.random.seed(7)   # (the prior's draws)
        n += dump(root, tag + '__smc', s, lambda: dict(
            logz=s.run(num_particles=PARTICLES, mcmc_steps=3, seed=8, route='fused'), samples=s.samples, loglikes=s.loglikes,
            latent=s.latent_samples, betas=s.betas, ess=s.ess, acceptance=s.acceptance, logz_steps=s.logz_steps))
    print('%d arrays under %s (nnest_amd: %s)' % (n, root, os.path.dirname(nnest_amd.__file__)))


if __name__ == '__main__':
    main()
