"""A front-end run decides its device target once (Sampler._device_target): the user's host callable sees the 32-point probe that
checks the kernels' likelihood against it exactly once per run, whichever fused front end runs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 2


class _CountingGaussian(object):
    """likelihoods.Gaussian that counts the calls whose batch is the probe's 32 points"""

    def __init__(self):
        from nnest_amd.likelihoods import Gaussian
        self.like = Gaussian(D, 0.5)
        self.hip_like_id, self.hip_like_params = self.like.hip_like_id, self.like.hip_like_params
        self.probes = 0

    def __call__(self, x):
        self.probes += int(np.shape(x)[0] == 32)
        return self.like(x)


def _sampler(cls_name, tmp_path):
    import nnest_amd
    from nnest_amd.priors import UniformPrior
    np.random.seed(1)
    torch.manual_seed(1)
    like = _CountingGaussian()
    s = getattr(nnest_amd, cls_name)(D, like, prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, jitter=0.0, **kw: None   # the flow stays at its initialisation
    return s, like


def test_each_fused_front_end_probes_the_host_callable_once(tmp_path):
    train = np.random.RandomState(0).normal(size=(200, D)) * 1.5
    s, like = _sampler('MCMCSampler', tmp_path / 'mcmc')
    assert like.probes == 0   # (no K4 route for this prior: nothing probed at construction)
    s.run(3, 4, train, route='fused', seed=1)
    assert s.mcmc_route == 'fused' and like.probes == 1
    assert s.importance_evidence(64, route='fused', seed=2)['route'] == 'fused' and like.probes == 2
    s, like = _sampler('SMCSampler', tmp_path / 'smc')
    s.run(num_particles=16, mcmc_steps=2, route='fused', seed=3)
    assert s.smc_route == 'fused' and len(s.betas) >= 1 and like.probes == 1
