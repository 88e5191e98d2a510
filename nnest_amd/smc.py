"""SMCSampler: a sequential Monte Carlo sampler on this build's Sampler (BUILD-DEFINED: the reference has no such sampler; DESIGN.md
3.12).  The population anneals L^beta pi from beta = 0 -- the prior, sampled exactly -- to beta = 1.  Between two temperatures it is
reweighted (the next beta is where the effective sample size of the incremental weights falls to `ess_fraction` of the population),
resampled (systematically, on integer weights), the flow is retrained on its distinct particles, and every particle takes `mcmc_steps`
Metropolis steps in the flow's latent space on the tempered target.  It needs no starting samples, returns the posterior sample and log Z from one run,
and carries separated modes from the prior instead of having to find them.

Routes.  'fused': the reweighting, the resampling and every step of a stage's moves run on the device (include/nnest_hip.h
nnest_smc_reweight, nnest_smc_resample, nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps), where
`Sampler._device_target(entry='mcmc_tempered')` gives a target: `_mcmc_sample_device`'s conditions and a family with a tempered
kernel.  'host': everything else -- a Python likelihood, the other flows, another prior -- a plain loop with the flow passes on the
GPU and the user's callables on the host, reweighted and resampled in numpy by the same rule (`reweight_host`, `resample_host`);
derived parameters are not carried by either route.

CONVENTION of `logz`: log of the integral of L(theta) pi(theta) d theta with the NORMALISED prior the particles were drawn from
(Z at beta = 0 is 1), as NestedSampler's `logz`.  For a UniformPrior on [lo, hi] this differs from `Sampler.importance_evidence`'s
convention -- the prior as its callable returns it, the unnormalised indicator -- by sum log(hi - lo):
logz_smc = logz_importance - sum log(hi - lo).  A priors.GaussianPrior's callable is the normalised density itself, and its
particles are drawn with `prior.sample`: `logz` under it carries no such term on either route (with a likelihoods.GLMData the fused
route takes it: DESIGN.md 3.17)."""
import functools
import logging
import math
import time

import numpy as np

from .sampler import Sampler

SMC_WEIGHT_ONE = 2147483648.0   # 2^31: the integer weight of the heaviest particle


def reweight_host(logl, beta, ess_fraction):
    """nnest_smc_reweight's rule in numpy (include/nnest_hip.h): (beta', log mean exp((beta' - beta) logL), ESS(beta'), max logL) and
    the integer weights m [N] int64"""
    logl = np.asarray(logl, np.float64)
    N = len(logl)
    mx = float(np.max(logl))
    d = logl - mx
    target = float(ess_fraction) * N

    def sums(b):
        w = np.exp((b - beta) * d)
        return float(w.sum()), float((w * w).sum()), w

    s1, s2, _ = sums(1.0)
    new = 1.0
    if s1 * s1 / s2 < target:
        lo, hi = float(beta), 1.0
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            s1, s2, _ = sums(mid)
            if s1 * s1 / s2 < target:
                hi = mid
            else:
                lo = mid
        new = hi if hi > beta else 1.0   # (the ladder always advances)
    s1, s2, w = sums(new)
    return (new, (new - beta) * mx + np.log(s1 / N), s1 * s1 / s2, mx), np.floor(w * SMC_WEIGHT_ONE).astype(np.int64)


def resample_host(m, u):
    """nnest_smc_resample's rule in numpy for the uniform u in [0, 1): anc [N], anc_j the smallest i whose inclusive prefix sum of m
    exceeds floor((j + u) sum(m) / N)"""
    m = np.asarray(m, np.int64)
    N = len(m)
    cum = np.cumsum(m)
    T = int(cum[-1])
    if T <= 0:
        raise ValueError('resample: the weights sum to 0')
    p = np.floor(((np.arange(N, dtype=np.float64) + float(u)) * float(T)) / float(N)).astype(np.int64)
    return np.searchsorted(cum, p, side='right')


def stage_seed(seed, stage):
    """the Philox seed of a stage's moves: a function of (seed, stage) only"""
    return (int(seed) + 0x9E3779B97F4A7C15 * (int(stage) + 1)) & 0xFFFFFFFFFFFFFFFF


class SMCSampler(Sampler):

    def __init__(self, x_dim, loglike, prior=None, append_run_num=True, hidden_dim=16, num_slow=0, num_derived=0, batch_size=100,
                 flow='spline', num_blocks=3, num_layers=1, learning_rate=0.001, log_dir='logs/test', base_dist=None, scale='',
                 use_gpu=False, trainer=None, transform_prior=True, oversample_rate=-1, log_level=logging.INFO, param_names=None, chain_stats=False):
        super(SMCSampler, self).__init__(x_dim, loglike, append_run_num=append_run_num, hidden_dim=hidden_dim, num_slow=num_slow,
                                         num_derived=num_derived, batch_size=batch_size, flow=flow, num_blocks=num_blocks,
                                         num_layers=num_layers, learning_rate=learning_rate, log_dir=log_dir, use_gpu=use_gpu,
                                         base_dist=base_dist, scale=scale, trainer=trainer, prior=prior,
                                         transform_prior=transform_prior, log_level=log_level, oversample_rate=oversample_rate,
                                         param_names=param_names, chain_stats=chain_stats)
        self.sampler = 'smc'

    # Every how many steps of a stage's moves a flow-independence ("global") step is taken; 0: never, the run as it was.  An
    # attribute of the sampler, set before `run` (sampler.global_every = 2), not an argument of `run`: tests/test_smc_check.py pins
    # run's argument list, and existing tests stay as they are.  `run` has the rest.
    global_every = 0
    # The share of a stage's moves over which every particle adapts its own step (include/nnest_hip.h nnest_mcmc_adapt_steps), and
    # the acceptance the rule aims at; 0.0: the fixed step, the run as it was.  Attributes for the same reason.  `run` has the rest.
    adapt_fraction = 0.0
    target_accept = 0.234

    def run(self, num_particles=1000, mcmc_steps=25, ess_fraction=0.5, step_size=0.0, jitter=0.01, seed=None, route=None, max_stages=1000):
        """Anneal `num_particles` draws of the prior to the posterior (the module docstring has the algorithm and the convention of
        `logz`).  mcmc_steps: Metropolis steps per particle and stage, at the fixed step `step_size` (<= 0: 2 / sqrt(x_dim), as
        `_mcmc_sample_device`); ess_fraction in (0, 1): the effective sample size, as a share of the population, at which the next
        temperature is placed; jitter: the training jitter; seed: the Philox seed of the resampling draws and the moves (None:
        `_next_seed()`) -- a stage's draws are a function of (seed, stage) only; the prior's draws and the training use numpy's
        and torch's global streams.  route: None -- 'fused' where it applies, else 'host'; an explicit 'fused' that does not apply
        raises ValueError naming why.  ValueError for a prior without a `sample` method; RuntimeError where beta = 1 is not reached
        within `max_stages` stages.
        Leaves: logz; betas, ess, acceptance, logz_steps (log Z's increments: they add up to logz) -- one entry per stage; samples
        [N, D] (theta at beta = 1), loglikes [N], latent_samples [N, D]; smc_route; stage_times (seconds per stage: reweight --
        with the resampling --, train, move); total_calls grows by N for the start and by N (1 + mcmc_steps) per stage (the start of
        a launch is evaluated, as the fused Metropolis route counts it).
        `self.global_every` = k > 0 (the attribute above) makes every k-th step of a stage's moves a flow-independence ("global")
        step at the stage's beta -- a draw of the freshly trained flow's base as the proposal, accepted on the ratio of importance
        weights (include/nnest_hip.h nnest_mcmc_mixed_steps) --, the step that decorrelates the copies a resampling leaves.  The
        fused route only: ValueError naming it where the host loop would run.  Leaves global_acceptance, one entry per stage beside
        `acceptance`.  0: the run as it was.
        `self.adapt_fraction` = f in (0, 1] (the attribute above) adapts the step: every particle enters a stage at the population's
        step (stage 0: `step_size`), adapts its own over the first ceil(f * mcmc_steps) steps of the stage towards the acceptance
        `self.target_accept` and keeps it for the rest; the next stage starts from the geometric mean exp(mean(log step_i)) of this
        stage's ends, so the step follows the ladder from the prior to the posterior.  The fused route only: ValueError naming it
        where the host loop would run.  Leaves step_sizes, the population's step at the end of each stage, one entry per stage, and
        logs it.  0.0: the run as it was, bit for bit."""
        if route not in (None, 'host', 'fused'):
            raise ValueError("route=%r: None, 'host' or 'fused'" % (route,))
        global_every = int(self.global_every)
        if global_every < 0:
            raise ValueError('SMCSampler.run: global_every=%d (every how many steps a global step is taken: >= 0)' % global_every)
        adapt_fraction, target_accept = float(self.adapt_fraction), float(self.target_accept)
        if not 0.0 <= adapt_fraction <= 1.0:
            raise ValueError('SMCSampler.run: adapt_fraction=%r (the share of a stage over which the step adapts: inside [0, 1])' % (
                self.adapt_fraction,))
        if adapt_fraction and not 0.0 < target_accept < 1.0:
            raise ValueError('SMCSampler.run: target_accept=%r (strictly inside (0, 1))' % (self.target_accept,))
        if self.sample_prior is None:
            raise ValueError('Prior does not have sample method')
        N, S, D = int(num_particles), int(mcmc_steps), self.x_dim
        if N < 2 or S < 1:
            raise ValueError('SMCSampler.run: num_particles=%d (>= 2) mcmc_steps=%d (>= 1)' % (N, S))
        if not 0.0 < float(ess_fraction) < 1.0:
            raise ValueError('SMCSampler.run: ess_fraction=%r (inside (0, 1))' % (ess_fraction,))
        self._install_transform(np.zeros(D), np.ones(D))   # (theta itself, until the first stage installs its own)
        # (likelihood and box do not depend on T: resolved here, once; every stage takes a copy under its own T)
        target, why = (None, None) if route == 'host' else self._device_target(
            entry='mcmc_adapt' if adapt_fraction else 'mcmc_mixed' if global_every else 'mcmc_tempered')
        if route == 'fused' and why is not None:
            raise ValueError('SMCSampler.run: the fused route does not take %s' % why)
        route = 'host' if target is None else 'fused'
        if global_every and route == 'host':
            raise ValueError("SMCSampler.run: global_every=%d needs the fused route, whose kernels alone take the global step%s" % (
                global_every, '' if why is None else ': the fused route does not take %s' % why))
        if adapt_fraction and route == 'host':
            raise ValueError("SMCSampler.run: adapt_fraction=%g needs the fused route, whose kernels alone adapt the step%s" % (
                adapt_fraction, '' if why is None else ': the fused route does not take %s' % why))
        if step_size <= 0.0:
            step_size = 2 / D ** 0.5
        seed = self._next_seed() if seed is None else int(seed)
        if route == 'fused':
            state = self._smc_start_fused(N, target)
            adapt = dict(adapt_steps=int(math.ceil(adapt_fraction * S)), target_accept=target_accept) if adapt_fraction else {}
            stage_fn = functools.partial(self._smc_stage_fused, target=target, **(dict(global_every=global_every) if global_every else {}),
                                         **adapt)
        else:
            state, stage_fn = self._smc_start_host(N), self._smc_stage_host
        beta, logz = 0.0, 0.0
        self.betas, self.ess, self.acceptance, self.logz_steps, self.stage_times = [], [], [], [], []
        self.global_acceptance = []   # (per stage, with global_every > 0)
        self.step_sizes = []          # (per stage, with adapt_fraction > 0: the population's step at the stage's end)
        stage = 0
        while beta < 1.0:
            if stage >= int(max_stages):
                raise RuntimeError('SMCSampler.run: beta=%g after %d stages (max_stages)' % (beta, stage))
            # (with adapt_fraction > 0 a stage enters at the step the stage before it left)
            stage_step = self.step_sizes[-1] if self.step_sizes else float(step_size)
            beta_new, inc, ess, acc, state, times = stage_fn(state, beta, float(ess_fraction), S, stage_step, float(jitter), seed, stage)
            if not beta_new > beta:
                raise RuntimeError('SMCSampler.run: the ladder did not advance (beta=%r -> %r)' % (beta, beta_new))
            beta = beta_new
            logz += inc
            self.betas.append(beta)
            self.ess.append(ess)
            self.acceptance.append(acc)
            self.logz_steps.append(inc)
            self.stage_times.append(times)
            stage += 1
            if self.single_or_primary_process:
                self.logger.info('smc stage [%d] beta [%.6g] ESS [%.1f of %d] acceptance [%5.4f] log Z [%5.4f]' % (stage, beta, ess, N, acc, logz))
                if global_every:
                    self.logger.info('smc stage [%d] global steps every [%d] global acceptance [%5.4f]' % (
                        stage, global_every, self.global_acceptance[-1]))
                if adapt_fraction:
                    self.logger.info('smc stage [%d] entered at step [%.6g] adapted over [%d] steps: population step [%.6g]' % (
                        stage, stage_step, int(math.ceil(adapt_fraction * S)), self.step_sizes[-1]))
        self.logz = logz
        self.smc_route = route
        theta, logl, z = state
        to_np = lambda t: t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)
        self.samples = to_np(theta).astype(np.float64)
        self.loglikes = to_np(logl).astype(np.float64)
        self.latent_samples = None if z is None else to_np(z)
        if self.single_or_primary_process:
            self.logger.info('smc: log Z [%5.4f] stages [%d] route [%s] ncall: %d\n' % (logz, stage, route, self.total_calls))
        return logz

    def _smc_train(self, theta_np, jitter):
        """install T(x) = x * std + mean of the population and train the flow on the normalised population's DISTINCT rows; returns
        the whole normalised population.  A resampling leaves every particle of weight above the mean in several exact copies (a
        third of the rows at ess_fraction 0.5).  Trained on with a jitter of 0.01 they are spikes that a spline flow fits: latent
        volume concentrates at them, accepted latent moves change theta little, the copies stay close and log Z comes out low
        (0.33 nats at x_dim 4, 5 at x_dim 20).  The preconditioner needs the population's shape, not its
        multiplicities, which the particles themselves carry"""
        mean, std = np.mean(theta_np, axis=0), np.std(theta_np, axis=0)
        std = np.where(std > 0.0, std, 1.0)   # (a population that has collapsed in a dimension)
        self._install_transform(mean, std)
        normalised = (theta_np - mean) / std
        self.trainer.train(np.unique(normalised, axis=0), jitter=jitter)
        return normalised, mean, std

    # ---- the fused route: theta [N, D] float32, logL [N] float64 and z on the device ------------------------------------------------
    def _smc_start_fused(self, N, target):
        import torch
        from . import flow
        if N > flow.SMC_MAX_PARTICLES:
            raise ValueError('SMCSampler.run: num_particles=%d: the fused route takes up to %d' % (N, flow.SMC_MAX_PARTICLES))
        netG = self.trainer.netG
        theta = torch.as_tensor(np.asarray(self.sample_prior(N), np.float32)).to(netG.device).contiguous()
        if target.like_data is not None:   # (a Gaussian likelihood from user data: no id, its own evaluator)
            logl = flow.loglike_gdata(target.launch_kwargs(netG.device)['like_data'], theta, device=netG.device)
        elif target.like_glm is not None:   # (a regression likelihood of user data, likewise)
            logl = flow.loglike_glm(target.launch_kwargs(netG.device)['like_glm'], theta, device=netG.device)
        else:
            logl = flow.loglike(target.like_id, theta, 1.0, device=netG.device, like_params=target.like_params)
        self.total_calls += N
        return theta, logl, None

    def _smc_stage_fused(self, state, beta, ess_fraction, S, step_size, jitter, seed, stage, target, global_every=0, adapt_steps=0, target_accept=0.234):
        import torch
        from . import flow
        theta, logl, _ = state
        netG = self.trainer.netG
        N = theta.shape[0]
        t0 = time.perf_counter()
        out, m = flow.smc_reweight(logl, beta, ess_fraction)
        _, theta, logl = flow.smc_resample(m, theta, logl, seed, stage)
        beta_new, inc, ess, _ = (float(v) for v in out.cpu().numpy())
        t1 = time.perf_counter()
        normalised, mean, std = self._smc_train(theta.cpu().numpy().astype(np.float64), jitter)
        torch.cuda.synchronize(netG.device)
        t2 = time.perf_counter()
        z, _ = netG.forward(normalised.astype(np.float32))
        target = target.with_transform(std, mean)   # (this stage's T)
        res = netG.mcmc_steps(target.like_id, z.contiguous(), S, step_size, seed=stage_seed(seed, stage), history=False, beta=beta_new,
                              **(dict(global_every=global_every) if global_every else {}),
                              **(dict(adapt_steps=adapt_steps, target_accept=target_accept) if adapt_steps else {}),
                              **target.launch_kwargs(netG.device))
        if adapt_steps:   # (the population's step: the geometric mean of the particles' ends, one reduction)
            self.step_sizes.append(float(torch.exp(torch.log(res['step']).mean()).item()))
        theta = target.transform(res['x'])
        n_acc = int(res['n_accept'].sum().item())
        if global_every:   # (steps t = k - 1, 2k - 1, ... of the stage's 0 .. S - 1)
            self.global_acceptance.append(int(res['n_accept_global'].sum().item()) / float(max(1, N * (S // global_every))))
        t3 = time.perf_counter()
        self.total_calls += N * (1 + S)
        self.total_accepted += n_acc
        self.total_rejected += N * S - n_acc
        return beta_new, inc, ess, n_acc / float(N * S), (theta, res['logl'], res['z']), dict(reweight=t1 - t0, train=t2 - t1, move=t3 - t2)

    # ---- the host route: theta [N, D] float64 and logL [N] in numpy, the flow passes on the GPU --------------------------------------
    def _smc_start_host(self, N):
        theta = np.asarray(self.sample_prior(N), np.float64)
        logl, _ = self.loglike(theta)   # (T = identity here; counts the calls)
        return theta, logl, None

    def _smc_lp_host(self, q, beta):
        """x = f^-1(q), lp_beta = ((beta logL) + log|det|) + log prior, and logL, with the user's callables on T(x)"""
        x_t, ld = self.trainer.netG.inverse(q)
        x = x_t.cpu().numpy().astype(np.float64)
        logl, _ = self.loglike(x)
        return x, ((beta * logl) + ld.double().cpu().numpy()) + np.asarray(self.prior(x), np.float64), logl

    def _smc_stage_host(self, state, beta, ess_fraction, S, step_size, jitter, seed, stage):
        theta, logl, _ = state
        N, D = theta.shape
        rng = np.random.RandomState(stage_seed(seed, stage) & 0xFFFFFFFF)
        t0 = time.perf_counter()
        (beta_new, inc, ess, _), m = reweight_host(logl, beta, ess_fraction)
        anc = resample_host(m, np.floor(rng.uniform() * (1 << 24)) / (1 << 24))
        theta, logl = theta[anc], logl[anc]
        t1 = time.perf_counter()
        normalised, mean, std = self._smc_train(theta, jitter)
        t2 = time.perf_counter()
        z_t, _ = self.trainer.netG.forward(normalised.astype(np.float32))
        z = z_t.cpu().numpy().astype(np.float32)
        x, lp, logl = self._smc_lp_host(z, beta_new)
        n_acc = 0
        for _ in range(S):
            q = z + np.float32(step_size) * rng.standard_normal((N, D)).astype(np.float32)
            xq, lpq, loglq = self._smc_lp_host(q, beta_new)
            with np.errstate(invalid='ignore', divide='ignore'):   # (-inf - -inf: NaN, never accepted)
                acc = lpq - lp > np.log(rng.uniform(size=N))
            z[acc], x[acc], lp[acc], logl[acc] = q[acc], xq[acc], lpq[acc], loglq[acc]
            n_acc += int(acc.sum())
        t3 = time.perf_counter()
        self.total_accepted += n_acc
        self.total_rejected += N * S - n_acc
        return beta_new, inc, ess, n_acc / float(N * S), (np.asarray(self.transform(x), np.float64), logl, z), dict(
            reweight=t1 - t0, train=t2 - t1, move=t3 - t2)
