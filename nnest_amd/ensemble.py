"""EnsembleSampler: the reference's emcee front-end (nnest/ensemble.py:20-231) on this build's Sampler: train the flow on a set of
(normalised) training samples, then run emcee's default stretch move in its latent space (`Sampler._ensemble_sample`,
sampler.py:632-724).  emcee is not used: the move is restated (include/nnest_hip.h nnest_ensemble_steps) -- BUILD-DEFINED STREAM,
EMCEE'S MOVE, so parity with emcee is statistical.  With chain_stats=True the run logs the reference's chain statistics
(sampler.py:712-713 every `stats_interval` steps after the first, ensemble.py:224-225 at the end), computed on the GPU by
nnest_amd.evaluation; the trace plots are not drawn.

`bootstrap` (ensemble.py:81-184) starts without training samples: the same stretch move in X space on logL(x) + prior(x)
(`Sampler._ensemble_sample_x`: the fused kernel nnest_ensemble_x_steps where `Sampler._device_target` gives a target, or the round
driver on an identity flow), emcee's integrated
autocorrelation time of that run (nnest_amd.evaluation.integrated_autocorr_time), emcee's discard / thin rule for the first
training samples, then rounds of train + latent-space run, each thinned into the next round's training samples by getdist's
makeSingleSamples rule.  Neither emcee nor getdist is used: both rules are restated (see `bootstrap`)."""
import logging

import numpy as np
import torch

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

    # emcee moves the reference's `moves` dict can name and bootstrap's x-space run refuses ('de' is built for the latent-space runs:
    # `latent_moves`)
    STRETCH_ONLY = ('kde', 'de', 'snooker')

    def bootstrap(self, mcmc_steps, num_walkers, iters=1, thin=10, stats_interval=10, output_interval=None, initial_jitter=0.01,
                  final_jitter=0.01, init_samples=None, moves=None, seed=None, route=None, latent_moves=None):
        """ensemble.py:81-184: from a likelihood and a prior to training samples and a trained flow, without emcee or getdist.

        1. The stretch move in x space from `init_samples` (else `num_walkers` draws of the prior) for `mcmc_steps` steps, on
           logL(x) + prior(x) (`_ensemble_sample_x`, T = identity; BUILD-DEFINED STREAM, EMCEE'S MOVE).  `moves`: None or
           {'stretch': w}; 'kde', 'de' and 'snooker' are not built (NotImplementedError).  As in the reference, `moves` is not
           forwarded to the latent runs.  The run is written to chains/emcee.txt (`_save_samples`) in place of emcee.h5; RESUMING
           from that file, which the reference's HDF backend does, is not built: every call starts a new run.
        2. tau = emcee's integrated autocorrelation time of that run (AutocorrError if it is shorter than 50 tau), discard =
           int(2 max tau), thin = max(1, int(0.5 min tau)) -- the clamp is a deviation: emcee divides by thin = 0 -- and the
           training samples are emcee's get_chain(discard, thin, flat=True): steps discard + thin - 1, discard + 2 thin - 1, ...
           of every walker, step-major.
        3. `iters` times: the reference's jitter schedule, mean / std normalisation, trainer.train, a fresh latent-space run of
           `mcmc_steps` steps (`_ensemble_sample`), the chain statistics line, then getdist's MCSamples.makeSingleSamples(
           single_thin=`thin`) for unit weights: every row of the concatenated chains is kept independently with probability
           1 / thin.  That rule is RESTATED FROM GETDIST'S DOCUMENTED BEHAVIOUR (getdist is not available to check against), on a
           BUILD-DEFINED STREAM: a torch generator seeded from `_next_seed()`.

        `seed` (not in the reference): the runs' and the thinning's seeds are seed, seed + 1, ...; None: `_next_seed()`.
        `route` (not in the reference): forwarded to the latent-space runs of step 3 only (`_ensemble_sample`: None | 'fused' |
        'rounds'); the x-space run of step 1 keeps its own choice.
        `latent_moves` (not in the reference): the moves of the latent-space runs of step 3, {'stretch': w, 'de': w}
        (`_ensemble_sample`: emcee's differential-evolution move beside the stretch move, one move per step by weight); the
        x-space run of step 1 keeps the stretch move, and `moves` its check above.
        Returns the last training samples [n, D]; leaves samples, latent_samples and loglikes of the last latent
        run, as `run` does."""
        if moves is not None:
            for k in moves:
                if str(k).lower() in self.STRETCH_ONLY:
                    raise NotImplementedError("EnsembleSampler.bootstrap: the '%s' move is not built (only emcee's default "
                                              "'stretch' move is)" % k)
                if str(k).lower() != 'stretch':
                    raise ValueError("EnsembleSampler.bootstrap: unknown move '%s'" % k)
        from . import _lib
        latent_moves = _lib.ens_moves(latent_moves, 'EnsembleSampler.bootstrap')   # (refused before the x-space run, not after it)
        if init_samples is None:
            if self.sample_prior is None:
                raise ValueError('Prior does not have sample method')
            init_samples = self.sample_prior(num_walkers)
        init_samples = np.asarray(init_samples)
        count = [0]

        def next_seed():
            count[0] += 1
            return self._next_seed() if seed is None else int(seed) + count[0] - 1

        D, nd = self.x_dim, self.num_derived
        self.transform = self._checked_transform if self._user_transform is not None else (lambda x: x)
        self._ensemble_transform = None
        self.logger.info('Performing initial emcee run with [%d] walkers' % (init_samples.shape[0]))
        acc0, rej0 = self.total_accepted, self.total_rejected
        chain, loglikes, derived, _ = self._ensemble_sample_x(mcmc_steps, init_samples, output_interval=output_interval,
                                                              seed=next_seed())
        N, S = chain.shape[:2]
        self.logger.info('Initial acceptance [%5.4f]' % ((self.total_accepted - acc0) / max(1, self.total_accepted - acc0 + self.total_rejected - rej0)))
        if S > 1:
            self._chain_stats(chain)
        self._save_samples(chain.reshape(-1, D), loglikes.reshape(-1), derived_samples=derived.reshape(N * S, nd), outfile='emcee')

        from .evaluation import integrated_autocorr_time
        tau = integrated_autocorr_time(chain)
        discard, single = int(2 * np.max(tau)), max(1, int(0.5 * np.min(tau)))
        self.logger.info('Autocorrelation time min [%5.4f] max [%5.4f]: discard [%d] thin [%d]' % (np.min(tau), np.max(tau), discard, single))
        # emcee's get_chain(discard, thin, flat=True) on [steps, walkers, D]
        training_samples = np.transpose(chain, (1, 0, 2))[discard + single - 1:S:single].reshape(-1, D).astype(np.float64)
        if len(training_samples) < 2:
            raise ValueError('bootstrap: %d steps leave %d training samples after discard %d' % (S, len(training_samples), discard))

        for it in range(1, iters + 1):
            if iters > 1:
                jitter = initial_jitter + (it - 1) * (final_jitter - initial_jitter) / (iters - 1)
            else:
                jitter = initial_jitter
            mean, std = np.mean(training_samples, axis=0), np.std(training_samples, axis=0)
            self._install_transform(mean, std)
            self.trainer.train((training_samples - mean) / std, jitter=jitter)
            samples, latent_samples, derived_samples, loglikes, ncall = self._ensemble_sample(
                mcmc_steps, num_walkers, stats_interval=stats_interval, output_interval=output_interval, seed=next_seed(), route=route,
                moves=latent_moves)
            self._chain_stats(samples, affine=(std, mean))
            samples = self.transform(samples)
            self.samples = np.concatenate((samples, derived_samples), axis=2)
            self.latent_samples = latent_samples
            self.loglikes = loglikes
            # getdist MCSamples(samples=[chain_0, chain_1, ...]).makeSingleSamples(single_thin=thin), unit weights
            gen = torch.Generator(device='cpu')
            gen.manual_seed(next_seed() & 0x7FFFFFFFFFFFFFFF)
            rows = samples.reshape(-1, D)   # (walker after walker, as getdist concatenates the chains)
            keep = torch.rand(len(rows), generator=gen, dtype=torch.float64).numpy() < 1.0 / thin
            training_samples = rows[keep].astype(np.float64)
        self.logger.info('ncall: {:d}\n'.format(self.total_calls))
        return training_samples

    def run(self, mcmc_steps, num_walkers, training_samples, stats_interval=10, output_interval=None, initial_jitter=0.01,
            final_jitter=0.01, init_samples=None, route=None, moves=None):
        """ensemble.py:186-231.  As in the reference, `init_samples` is accepted and not forwarded; `stats_interval` is used with
        chain_stats=True.  `route` (not in the reference) goes to the latent-space run (`_ensemble_sample`): None, or 'fused' /
        'rounds' to pin one -- with the default spline flow the fused kernel runs on route='fused' only.  `moves` (not in the
        reference's `run`) goes there too: {'stretch': w, 'de': w}, emcee's differential-evolution move beside the stretch move, one
        move per step by weight; with a DE step the spline flow runs the round route (route='fused': ValueError).  Sets samples [N, S, D + num_derived] (T(x), then the derived parameters: zeros, sampler.py:687),
        latent_samples [N, S, D] and loglikes [N, S] -- emcee's log_prob, the latent log target, not logL."""
        mean = np.mean(training_samples, axis=0)
        std = np.std(training_samples, axis=0)
        training_samples = (training_samples - mean) / std          # normalise
        self._install_transform(mean, std)
        self.trainer.train(training_samples, jitter=initial_jitter)
        samples, latent_samples, derived_samples, loglikes, ncall = self._ensemble_sample(
            mcmc_steps, num_walkers, stats_interval=stats_interval, output_interval=output_interval, route=route, moves=moves)
        if self.chain_stats:
            self._log_chain_stats(samples, (std, mean), mcmc_steps, stats_interval, prefix_offset=0, min_step=1)
        samples = self.transform(samples)
        self.samples = np.concatenate((samples, derived_samples), axis=2)
        self.latent_samples = latent_samples
        self.loglikes = loglikes
        self.logger.info('ncall: {:d}\n'.format(self.total_calls))
