"""EnsembleSampler: the reference's emcee front-end (nnest/ensemble.py:20-231) on this build's Sampler: train the flow on a set of
(normalised) training samples, then run emcee's default stretch move in its latent space (`Sampler._ensemble_sample`,
sampler.py:632-724).  emcee is not used: the move is restated (include/nnest_hip.h nnest_ensemble_steps) -- BUILD-DEFINED STREAM,
EMCEE'S MOVE, so parity with emcee is statistical.  With chain_stats=True the run logs the reference's chain statistics
(sampler.py:712-713 every `stats_interval` steps after the first, ensemble.py:224-225 at the end), computed on the GPU by
nnest_amd.evaluation; the trace plots are not drawn, and `bootstrap` needs emcee's x-space run, its autocorrelation time and
getdist."""
import logging

import numpy as np

from .sampler import Sampler


class EnsembleSampler(Sampler):

    def __init__(self, x_dim, loglike, prior=None, append_run_num=True, hidden_dim=16, num_slow=0, num_derived=0, batch_size=100,
                 flow='spline', num_blocks=3, num_layers=1, learning_rate=0.001, log_dir='logs/test', base_dist=None, scale='',
                 use_gpu=False, trainer=None, transform_prior=True, oversample_rate=-1, log_level=logging.INFO, param_names=None, chain_stats=False):
        super(EnsembleSampler, self).__init__(x_dim, loglike, append_run_num=append_run_num, hidden_dim=hidden_dim, num_slow=num_slow,
                                              num_derived=num_derived, batch_size=batch_size, flow=flow, num_blocks=num_blocks,
                                              num_layers=num_layers, learning_rate=learning_rate, log_dir=log_dir, use_gpu=use_gpu,
                                              base_dist=base_dist, scale=scale, trainer=trainer, prior=prior,
                                              transform_prior=transform_prior, log_level=log_level, oversample_rate=oversample_rate,
                                              param_names=param_names, chain_stats=chain_stats)
        self.sampler = 'ensemble'

    def bootstrap(self, mcmc_steps, num_walkers, iters=1, thin=10, stats_interval=10, output_interval=None, initial_jitter=0.01,
                  final_jitter=0.01, init_samples=None, moves=None):
        raise NotImplementedError('EnsembleSampler.bootstrap (nnest/ensemble.py:83-184) needs an emcee run in x space, its '
                                  'autocorrelation time and getdist: not built')

    def _install_transform(self, mean, std):
        """T(x) = x * std + mean, also as per-dimension float arrays for the device routes"""
        self.transform = lambda x: x * std + mean
        self._ensemble_transform = (np.asarray(std, np.float64), np.asarray(mean, np.float64))
        self._linear_scale = None   # (the Metropolis kernels only know x -> s * x)
        self._fused_like_id = None

    def run(self, mcmc_steps, num_walkers, training_samples, stats_interval=10, output_interval=None, initial_jitter=0.01,
            final_jitter=0.01, init_samples=None):
        """ensemble.py:186-231.  As in the reference, `init_samples` is accepted and not forwarded; `stats_interval` is used with
        chain_stats=True.  Sets samples [N, S, D + num_derived] (T(x), then the derived parameters: zeros, sampler.py:687),
        latent_samples [N, S, D] and loglikes [N, S] -- emcee's log_prob, the latent log target, not logL."""
        mean = np.mean(training_samples, axis=0)
        std = np.std(training_samples, axis=0)
        training_samples = (training_samples - mean) / std          # normalise
        self._install_transform(mean, std)
        self.trainer.train(training_samples, jitter=initial_jitter)
        samples, latent_samples, derived_samples, loglikes, ncall = self._ensemble_sample(
            mcmc_steps, num_walkers, stats_interval=stats_interval, output_interval=output_interval)
        if self.chain_stats:
            self._log_chain_stats(samples, (std, mean), mcmc_steps, stats_interval, prefix_offset=0, min_step=1)
        samples = self.transform(samples)
        self.samples = np.concatenate((samples, derived_samples), axis=2)
        self.latent_samples = latent_samples
        self.loglikes = loglikes
        self.logger.info('ncall: {:d}\n'.format(self.total_calls))
