"""Protocol check at the reference's injection point (nnest/sampler.py:50, :196-212): a Trainer-shaped object exposing exactly
the surface of nnest_amd.Trainer(host_tensors=True) -- here the TEST-ONLY oracle-backed stand-in, since this check needs no
GPU -- drives a nested-sampling run.  The UNMODIFIED reference NestedSampler was driven with it by oracle/gen_nested_traj.py
(case rosen2_injection of tests/golden/nested_host_traj.json); the host driver, injected the same way on the same seeds, must
report what the reference reported."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nested_host_traj.json')


def test_reference_sampler_accepts_injected_trainer(tmp_path):
    from tests.oracle_trainer import OracleTrainer
    from nnest_amd.nested import NestedSampler
    from nnest_amd.likelihoods import Rosenbrock
    import nnest_amd.trainer as prod
    # the stand-in and the product expose the same protocol surface
    surface = ['forward', 'inverse', 'get_samples', 'get_latent_samples', 'get_prior_samples', 'train']
    for name in surface:
        assert callable(getattr(prod.Trainer, name)) and callable(getattr(OracleTrainer, name))
    with open(GOLDEN) as f:
        ref = json.load(f)['cases']['rosen2_injection']   # the reference's own run with the stand-in injected
    assert ref['run'] == dict(train_iters=30, mcmc_num_chains=5, max_iters=120, strategy=['mcmc'])
    assert np.isfinite(ref['logz']) and ref['num_trains'] >= 1 and ref['total_calls'] > 60
    np.random.seed(0)
    torch.manual_seed(0)
    tr = OracleTrainer(2, seed=0)
    # fused=False: the host protocol (the CPU stand-in has no kernel); checkpoint_min_seconds=0: the reference's dump cadence
    s = NestedSampler(2, Rosenbrock(2), transform=lambda x: 5 * x, log_dir=str(tmp_path), num_live_points=60,
                      flow='nvp', trainer=tr, log_level=40, fused=False, checkpoint_min_seconds=0)
    assert s.trainer is tr
    s.run(**ref['run'])
    assert np.isfinite(s.logz) and tr.num_trains >= 1 and s.total_calls > 60
    assert s.samples.shape[1] == 2
    assert float(s.logz) == ref['logz'] and int(s.total_calls) == ref['total_calls'] and tr.num_trains == ref['num_trains']
    assert np.array_equal(np.asarray(s.samples, dtype=np.float64), np.asarray(ref['samples']))
