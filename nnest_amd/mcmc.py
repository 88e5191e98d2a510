"""MCMCSampler: the reference's flow-accelerated Metropolis front-end (nnest/mcmc.py:24-130) on this build's Sampler:
train the flow on a set of (normalised) training samples, then run `_mcmc_sample` with the likelihood and prior in the
proposal ratio (loglstar = None, sampler.py:371-410).  As in the reference, `mcmc_dynamic_step_size` is accepted and not
forwarded (mcmc.py:118-120): the chains run at the fixed step 2 / sqrt(x_dim).  With chain_stats=True the run logs the reference's
chain statistics (acceptance, ESS, jump distance: sampler.py:451-452 every `stats_interval` steps, mcmc.py:119-120 at the end),
computed on the GPU by nnest_amd.evaluation (plain numpy in the reference, nnest/utils/evaluation.py; no getdist involved).
`run(..., route='fused')` runs the chains inside one kernel per launch (Sampler._mcmc_sample_device) where the likelihood, the prior
and the flow allow it (Sampler._device_target decides, once per run); the default is the host step loop, draw for draw as before."""
import logging

import numpy as np

from .sampler import Sampler


class MCMCSampler(Sampler):

    def __init__(self, x_dim, loglike, prior=None, append_run_num=True, hidden_dim=16, num_slow=0, num_derived=0, batch_size=100,
                 flow='spline', num_blocks=3, num_layers=1, learning_rate=0.001, log_dir='logs/test', base_dist=None, scale='',
                 use_gpu=False, trainer=None, transform_prior=True, oversample_rate=-1, log_level=logging.INFO, param_names=None, chain_stats=False):
        super(MCMCSampler, self).__init__(x_dim, loglike, append_run_num=append_run_num, hidden_dim=hidden_dim, num_slow=num_slow,
                                          num_derived=num_derived, batch_size=batch_size, flow=flow, num_blocks=num_blocks,
                                          num_layers=num_layers, learning_rate=learning_rate, log_dir=log_dir, use_gpu=use_gpu,
                                          base_dist=base_dist, scale=scale, trainer=trainer, prior=prior,
                                          transform_prior=transform_prior, log_level=log_level, oversample_rate=oversample_rate,
                                          param_names=param_names, chain_stats=chain_stats)
        self.sampler = 'mcmc'

    def run(self, mcmc_steps, mcmc_num_chains, training_samples, mcmc_dynamic_step_size=True, stats_interval=100,
            output_interval=None, initial_jitter=0.01, final_jitter=0.01, init_samples=None, route=None, seed=None, global_every=0, adapt_steps=0,
            target_accept=0.234):
        """mcmc.py:79-130.  `route` and `seed` are not in the reference.  route: None or 'host' -- the reference's step loop with the
        flow passes on the GPU and the likelihood and the prior on the host (`_mcmc_sample_host`), draw for draw on torch's and
        numpy's streams; 'fused' -- every step inside the kernel (`_mcmc_sample_device`: nnest_mcmc_steps for the NVP,
        nnest_spline_mcmc_steps for the spline flow; build-defined stream, the reference's move), taken where the likelihood is one
        the kernels know and agrees with the host callable on T(x), there are no derived parameters, the prior is none or a
        UniformPrior on T(x), num_slow = 0 and the flow has such a kernel; ValueError, naming what is not taken, otherwise.  The
        route that ran is left in `mcmc_route`.  seed: the fused run's Philox seed (None: `_next_seed()`); the host route does not
        use it.  Both routes keep the fixed step 2 / sqrt(x_dim).
        global_every (not in the reference; build-defined): k > 0 makes every k-th step of the fused run a flow-independence
        ("global") step -- a draw of the flow's base as the proposal, accepted on the ratio of importance weights
        (`_mcmc_sample_device`, nnest_mcmc_mixed_steps) --, which lets a chain jump between the modes the flow has learnt.  It needs
        route='fused' (ValueError otherwise) and a N(0, I) base; the run leaves `global_proposed` and `global_accepted` and logs the
        global acceptance rate.  0: the run as it was.
        adapt_steps, target_accept (not in the reference, whose MCMCSampler never forwards mcmc_dynamic_step_size; build-defined):
        adapt_steps = A > 0 lets every chain of the fused run adapt its own step over the local steps t < A towards the acceptance
        `target_accept` and keep it from there on (`_mcmc_sample_device`, nnest_mcmc_adapt_steps): from step A on each chain is an
        ordinary Metropolis chain, so discard the first A steps where exactness matters.  It needs route='fused' (ValueError
        otherwise); the run leaves `step_sizes` [mcmc_num_chains], `adapt_acceptance` and `frozen_acceptance` and logs them.  0: the
        run as it was."""
        if route not in (None, 'host', 'fused'):
            raise ValueError("route=%r: None or 'host' (the reference's step loop) or 'fused' (build-defined stream)" % (route,))
        global_every = int(global_every)
        if global_every < 0:
            raise ValueError('MCMCSampler.run: global_every=%d (every how many steps a global step is taken: >= 0)' % global_every)
        if global_every and route != 'fused':
            raise ValueError("MCMCSampler.run: global_every=%d needs route='fused': the global step is built into the fused route's "
                             "kernels only" % global_every)
        adapt_steps = int(adapt_steps)
        if adapt_steps < 0:
            raise ValueError('MCMCSampler.run: adapt_steps=%d (over how many steps the chains adapt their step: >= 0)' % adapt_steps)
        if adapt_steps and route != 'fused':
            raise ValueError("MCMCSampler.run: adapt_steps=%d needs route='fused': the per-chain step adaptation is built into the fused "
                             "route's kernels only" % adapt_steps)
        if adapt_steps and not 0.0 < float(target_accept) < 1.0:
            raise ValueError('MCMCSampler.run: target_accept=%r (strictly inside (0, 1))' % (target_accept,))
        mean = np.mean(training_samples, axis=0)
        std = np.std(training_samples, axis=0)
        training_samples = (training_samples - mean) / std          # normalise
        self._install_transform(mean, std)                           # T(x) = x * std + mean (the K4 kernels only know x -> s * x)
        if route == 'fused':
            target, why = self._device_target(entry='mcmc_adapt' if adapt_steps else 'mcmc_mixed' if global_every else 'mcmc')
            if why is not None:
                raise ValueError('MCMCSampler.run: the fused route does not take %s' % why)
        self.trainer.train(training_samples, jitter=initial_jitter)
        if route == 'fused':
            samples, latent_samples, derived_samples, loglikes, scale, ncall = self._mcmc_sample_device(
                mcmc_steps, num_chains=mcmc_num_chains, init_samples=init_samples, output_interval=output_interval,
                stats_interval=stats_interval, seed=seed, target=target, **(dict(global_every=global_every) if global_every else {}),
                **(dict(adapt_steps=adapt_steps, target_accept=float(target_accept)) if adapt_steps else {}))
            if self.chain_stats:   # (the interval lines were logged by the run)
                self._log_chain_stats(samples, (std, mean), mcmc_steps, None, prefix_offset=1, min_step=0)
        else:
            samples, latent_samples, derived_samples, loglikes, scale, ncall = self._mcmc_sample(
                mcmc_steps, num_chains=mcmc_num_chains, stats_interval=stats_interval, output_interval=output_interval,
                init_samples=init_samples)   # mcmc.py:118-120 does not forward mcmc_dynamic_step_size: the chains keep a fixed step
            if self.chain_stats:
                self._log_chain_stats(samples, (std, mean), mcmc_steps, stats_interval, prefix_offset=1, min_step=0)
        self.mcmc_route = 'fused' if route == 'fused' else 'host'
        samples = self.transform(samples)
        self.samples = np.concatenate((samples, derived_samples), axis=2)
        self.latent_samples = latent_samples
        self.loglikes = loglikes
        self.logger.info('ncall: {:d}\n'.format(self.total_calls))
