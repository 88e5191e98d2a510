"""Sampler base: the reference's nnest.sampler.Sampler contract (nnest/sampler.py:29-222) with the batched
latent-space Metropolis proposal `_mcmc_sample` (nnest/sampler.py:229-463) running as ONE persistent HIP
kernel launch per batch when the likelihood is one of the analytic ones the kernels know
(nnest_mh_constrained_steps, include/nnest_hip.h), and as GPU flow passes + host likelihood callbacks
otherwise (any user `loglike`, the reference's plugin protocol).

Multi-GPU: one process per GPU (torch.distributed, backend nccl = RCCL).  State is replicated, the chains of
a batch are sharded over ranks, and the only data-path collective is one all-gather of the chain endpoints
per batch (the reference's mpi4py gather+bcast of full histories, nnest/nested.py:416-427, shrunk to what is
consumed).
"""
import itertools
import json
import logging
import os

import numpy as np
import torch

from . import _lib
from .device_target import DeviceTarget
from .priors import GaussianPrior, UniformPrior
from .utils import create_logger, get_or_create_run_dir, write_rows_e5


def detect_linear_scale(transform, x_dim):
    """transform(x) == s * x for a scalar s?  (examples/nested/run.py:25-42 only uses such transforms.)
    Returns s or None.  Probing is on a few random rows; the fused path is additionally verified against the
    host callable before it is enabled (Sampler._verify_fused)."""
    if transform is None:
        return 1.0
    x = np.random.RandomState(12345).uniform(-1, 1, size=(4, x_dim))
    try:
        y = np.asarray(transform(x.copy()), dtype=np.float64)
    except Exception:
        return None
    if y.shape != x.shape:
        return None
    s = float(np.asarray(transform(np.ones((1, x_dim))), dtype=np.float64)[0, 0])  # exact, no division
    return s if np.allclose(y, s * x, rtol=1e-12, atol=0) else None


class Sampler(object):

    def __init__(self,
                 x_dim,
                 loglike,
                 transform=None,
                 prior=None,
                 append_run_num=True,
                 hidden_dim=16,
                 num_slow=0,
                 num_derived=0,
                 batch_size=100,
                 flow='spline',
                 num_blocks=3,
                 num_layers=1,
                 learning_rate=0.001,
                 log_dir='logs/test',
                 resume=True,
                 use_gpu=True,
                 base_dist=None,
                 scale='',
                 trainer=None,
                 transform_prior=True,
                 oversample_rate=-1,
                 log_level=logging.INFO,
                 param_names=None,
                 fused=True,
                 mcmc_history=False,
                 mcmc_proposal='mh',
                 chain_stats=False):
        # mcmc_proposal (not in the reference, whose _mcmc_sample proposes random-walk Metropolis moves only, sampler.py:310-316):
        # 'mh' = that step; 'slice' = the build-defined slice proposal in latent space (BASELINE north_star; include/nnest_hip.h,
        # parity unpinned) under the hard constraint logL > L*, with every flow and every likelihood: the fused kernels
        # (nnest_slice_steps, nnest_spline_slice_steps) where they take the flow and the likelihood is a known id, the round driver
        # nnest_amd.slice_rounds otherwise (other flows and shapes; a user likelihood, derived parameters or another prior).  A
        # likelihoods.GLMData under the unit box on x and x -> s * x runs on the device too: the fused kernels of that likelihood
        # (nnest_slice_glm_steps, nnest_spline_slice_glm_steps) where they take the flow, slice_rounds(like_glm=...) otherwise
        if mcmc_proposal not in ('mh', 'slice'):
            raise ValueError("mcmc_proposal=%r: 'mh' (the reference's step) or 'slice' (build-defined)" % (mcmc_proposal,))
        self.mcmc_proposal = mcmc_proposal
        self.x_dim = x_dim
        self.num_derived = num_derived
        self.num_params = x_dim + num_derived
        assert x_dim > num_slow                       # sampler.py:87
        self.num_slow = num_slow
        self.num_fast = x_dim - num_slow
        self.param_names = param_names
        if self.param_names is not None:
            assert len(param_names) == self.num_params
        self.oversample_rate = oversample_rate if oversample_rate > 0 else self.num_fast / self.x_dim   # sampler.py:95
        self.mcmc_history = mcmc_history
        # chain_stats: log the reference's chain statistics (acceptance, ESS, jump distance: sampler.py:474-492), computed on the
        # GPU (nnest_amd.evaluation); off by default, which leaves every run as it was
        self.chain_stats = bool(chain_stats)
        self._chain_hist = None   # chain_stats: the history [C, steps + 1, D] of the last batch of chains (this rank's)
        self._user_loglike = loglike
        self._user_prior = prior
        self._transform_prior = transform_prior

        self._user_transform = transform
        self.transform = self._checked_transform if transform is not None else (lambda x: x)
        self._linear_scale = detect_linear_scale(transform, x_dim)
        self.loglike = self._checked_loglike
        sample_prior = getattr(prior, 'sample', None)
        self.sample_prior = sample_prior if callable(sample_prior) else None
        self.prior = self._checked_prior

        # process group (the reference: mpi4py, sampler.py:165-177)
        self.use_mpi = False
        self.mpi_size, self.mpi_rank = 1, 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.mpi_size = torch.distributed.get_world_size()
            self.mpi_rank = torch.distributed.get_rank()
            # an initialised process group selects the distributed code path, also with ONE rank (the degenerate case runs
            # the same collectives; it is how the RCCL branch is exercised on a one-GPU box)
            self.use_mpi = True
        self.single_or_primary_process = (not self.use_mpi) or self.mpi_rank == 0

        # only the primary process owns a run directory: the others neither write it nor read checkpoints from it (the
        # reference lets every MPI rank read the checkpoint files, sampler.py:179-185; here rank 0 broadcasts the resumed state)
        if self.single_or_primary_process:
            self.logs = get_or_create_run_dir(log_dir, append_run_num=append_run_num)
            self.log_dir = self.logs['run_dir']
        else:
            self.logs = None
            self.log_dir = None
        if self.single_or_primary_process:
            args = {k: str(v) for k, v in dict(x_dim=x_dim, num_derived=num_derived, hidden_dim=hidden_dim, flow=flow,
                                               num_blocks=num_blocks, num_layers=num_layers, batch_size=batch_size,
                                               learning_rate=learning_rate, log_dir=self.log_dir, scale=scale,
                                               transform_prior=transform_prior, param_names=param_names).items()}
            with open(os.path.join(self.logs['info'], 'params.txt'), 'w') as f:
                json.dump(args, f, indent=4)

        self.resume = resume
        self.logger = create_logger(__name__, level=log_level)

        if trainer is None:
            from .trainer import Trainer
            self.trainer = Trainer(x_dim, hidden_dim=hidden_dim, num_slow=num_slow, batch_size=batch_size, flow=flow,
                                   num_blocks=num_blocks, num_layers=num_layers, learning_rate=learning_rate,
                                   log_dir=self.log_dir if self.single_or_primary_process else None,
                                   log=self.single_or_primary_process, use_gpu=use_gpu,
                                   base_dist=base_dist, scale=scale, log_level=log_level)
        else:
            self.trainer = trainer

        if self.single_or_primary_process:
            self.logger.info('Num base params [%d]' % self.x_dim)
            self.logger.info('Num derived params [%d]' % self.num_derived)
            self.logger.info('Total params [%d]' % self.num_params)

        self.total_accepted = 0
        self.total_rejected = 0
        self.total_calls = 0
        self.total_fast_calls = 0

        # can the whole proposal loop run inside the HIP kernel?
        self._fused_like_id = None
        self._fused_like_params = ()
        if fused:
            self._fused_like_id = self._fused_eligibility()
        # the slice proposal on a regression likelihood of user data (likelihoods.GLMData): its device target, resolved once, or None
        self._slice_glm = None
        self.slice_route = None   # 'fused-glm' | 'rounds-glm' | 'fused' | 'rounds' | 'host': what the last slice batch ran, logged once
        if fused and mcmc_proposal == 'slice' and self._fused_like_id is None and getattr(self.trainer, 'netG', None) is not None:
            self._slice_glm, _ = self._device_target(unit_box_on_x=True, entry='slice_glm')
        # the Metropolis proposal on such a likelihood (nnest_mh_glm_steps, nnest_spline_mh_glm_steps): its device target, or None
        self._mh_glm = None
        self.mh_route = None   # 'fused-glm' | 'fused' | 'host': what the last Metropolis batch ran, logged once
        if (fused and mcmc_proposal == 'mh' and self._fused_like_id is None and getattr(self.trainer, 'netG', None) is not None
                and getattr(self, 'mpi_size', 1) <= 1):
            self._mh_glm, _ = self._device_target(unit_box_on_x=True, entry='mh_glm')

    # ---- the user's callables behind shape checks (sampler.py:97-163) ----------------------------------------------
    def _rows(self, x):
        """[D] or [N, D] (array or list) -> [N, D]"""
        x = np.asarray(x) if isinstance(x, list) else x
        if x.ndim == 1:
            assert x.shape[0] == self.x_dim
            x = x[None, :]
        return x

    def _checked_transform(self, x):
        return self._user_transform(self._rows(x))

    def _checked_loglike(self, x):
        """loglike(transform(x)) -> (logl float64 [N], derived [N, num_derived]); counts the rows as likelihood calls;
        non-finite values become -1e100 (sampler.py:110-133)"""
        x = self._rows(x)
        n = x.shape[0]
        out = self._user_loglike(self.transform(x))
        self.total_calls += n
        logl, derived = out if isinstance(out, tuple) else (out, None)
        logl = np.array(logl, dtype=np.float64, ndmin=1)   # a copy, float64: -1e100 is not representable in float32
        logl[~np.isfinite(logl)] = -1e100
        if derived is None:
            derived = np.empty((n, 0))
        elif np.ndim(derived) == 1:
            raise ValueError('Derived should have dimensions (batch size, num derived params)')
        derived = np.asarray(derived)
        if derived.shape[1] != self.num_derived:
            raise ValueError('Is the number of derived parameters correct?')
        return logl, derived

    def _checked_prior(self, x):
        """log prior density of every row (sampler.py:137-163): the prior protocol is one row -> one number"""
        x = self._rows(x)
        prior = self._user_prior
        if prior is None:
            return np.zeros(x.shape[0])
        rows = getattr(prior, 'log_prob_rows', None)   # whole-batch form of the same rule, when the prior has one
        if callable(rows):
            return rows(self.transform(x) if self._transform_prior else x)
        if self._transform_prior:   # one row at a time through the transform, as the reference calls it (sampler.py:159)
            return np.array([prior(self.transform(r)) for r in x])
        return np.array([prior(r) for r in x])

    # ---- fused-path eligibility -----------------------------------------------------------------------
    def _fused_eligibility(self):
        like = self._user_loglike
        like_id = getattr(like, 'hip_like_id', None)
        netG = getattr(self.trainer, 'netG', None)
        if like_id is None or getattr(netG, 'mh_steps', None) is None or self._linear_scale is None or self.num_derived != 0:
            return None
        if not self._unit_box_on_x():
            return None
        # verify the kernel's likelihood against the host callable on a few points before trusting it
        self._fused_like_params = tuple(getattr(like, 'hip_like_params', ()) or ())
        if not self._probe_agrees(like_id, self._fused_like_params, self._linear_scale, warn='fused '):
            return None
        return like_id

    def _probe_agrees(self, like_id, params, scale=1.0, affine=None, warn=''):
        """does the kernels' likelihood `like_id` agree with the host callable?  On 32 fixed points of the unit box, handed to the
        kernel as each caller hands it its x: raw, with like_scale = `scale` (the K4 routes), or as T(x) = x * std + mean computed
        here in float32, with scale 1 (the device targets: `affine` = (std, mean)).  Warns (`warn` opens the line) where it does not"""
        from . import flow
        x = np.random.RandomState(4321).uniform(-1, 1, size=(32, self.x_dim)).astype(np.float32)
        if affine is not None:
            x = x * np.asarray(affine[0], np.float32) + np.asarray(affine[1], np.float32)
        dev = flow.loglike(like_id, x, scale, device=self.trainer.netG.device, like_params=params).cpu().numpy()
        host = np.asarray(self._user_loglike(scale * x.astype(np.float64)), dtype=np.float64)
        ok = bool(np.allclose(dev, host, rtol=1e-5, atol=1e-4))
        if not ok:
            self.logger.warning('%slikelihood id %d disagrees with the host callable; using the host protocol' % (warn, like_id))
        return ok

    def _probe_agrees_gdata(self, data, affine, warn=''):
        """`_probe_agrees` for a Gaussian likelihood from user data: does the kernels' evaluation of the descriptor `data`
        (flow.loglike_gdata) agree with the host callable, on the same 32 points under the same tolerances?  Warns where it does not"""
        from . import flow
        x = np.random.RandomState(4321).uniform(-1, 1, size=(32, self.x_dim)).astype(np.float32)
        x = x * np.asarray(affine[0], np.float32) + np.asarray(affine[1], np.float32)
        dev = flow.loglike_gdata(data, x, device=self.trainer.netG.device).cpu().numpy()
        host = np.asarray(self._user_loglike(x.astype(np.float64)), dtype=np.float64)
        ok = bool(np.allclose(dev, host, rtol=1e-5, atol=1e-4))
        if not ok:
            self.logger.warning('%sthe likelihood\'s hip_like_data disagrees with the host callable; using the host protocol' % warn)
        return ok

    def _probe_agrees_glm(self, data, affine, warn=''):
        """`_probe_agrees_gdata` for a regression likelihood of user data: the kernels' evaluation of the descriptor `data`
        (flow.loglike_glm) against the host callable, on the same 32 points under the same tolerances.  Warns where it does not"""
        from . import flow
        x = np.random.RandomState(4321).uniform(-1, 1, size=(32, self.x_dim)).astype(np.float32)
        x = x * np.asarray(affine[0], np.float32) + np.asarray(affine[1], np.float32)
        dev = flow.loglike_glm(data, x, device=self.trainer.netG.device).cpu().numpy()
        host = np.asarray(self._user_loglike(x.astype(np.float64)), dtype=np.float64)
        ok = bool(np.allclose(dev, host, rtol=1e-5, atol=1e-4))
        if not ok:
            self.logger.warning('%sthe likelihood\'s hip_like_glm disagrees with the host callable; using the host protocol' % warn)
        return ok

    def _probe_agrees_gauss_prior(self, data, affine, warn=''):
        """`_probe_agrees_glm` for the prior: the kernels' evaluation of the descriptor `data` (flow.logprior_gauss) against the prior's
        host callable, on the same 32 points under the same tolerances.  Warns where it does not"""
        from . import flow
        x = np.random.RandomState(4321).uniform(-1, 1, size=(32, self.x_dim)).astype(np.float32)
        x = x * np.asarray(affine[0], np.float32) + np.asarray(affine[1], np.float32)
        dev = flow.logprior_gauss(data, x, device=self.trainer.netG.device).cpu().numpy()
        host = np.array([self._user_prior(r) for r in x.astype(np.float64)], dtype=np.float64)
        ok = bool(np.allclose(dev, host, rtol=1e-5, atol=1e-4))
        if not ok:
            self.logger.warning('%sthe prior\'s hip_gauss_prior disagrees with the host callable; using the host protocol' % warn)
        return ok

    def _next_seed(self):
        """64-bit seed for the in-kernel Philox streams.  Drawn from a PRIVATE generator seeded once from the seed of torch's
        CPU generator (torch.manual_seed): the global generator is never advanced by the build's own bookkeeping, so the
        host protocol consumes torch / numpy randomness draw for draw as the reference's loop does (nested.py:398-456;
        tests/test_reference_trajectory.py holds the two drivers to the same trajectory)."""
        gen = getattr(self, '_seed_gen', None)
        if gen is None:
            gen = self._seed_gen = torch.Generator(device='cpu')
            gen.manual_seed(torch.initial_seed())
        return int(torch.empty((), dtype=torch.int64).random_(generator=gen).item())

    # ---- the batched proposal ---------------------------------------------------------------------------
    def _mcmc_sample(self,
                     mcmc_steps,
                     step_size=0.0,
                     dynamic_step_size=False,
                     num_chains=1,
                     init_samples=None,
                     init_loglikes=None,
                     init_derived=None,
                     loglstar=None,
                     show_progress=False,
                     max_start_tries=100,
                     output_interval=None,
                     stats_interval=None,
                     plot_trace=False,
                     prior_volume_steps=1,
                     walker_offset=0,
                     seed=None,
                     form=None):
        """Returns (samples, latent_samples, derived_samples, loglikes, scale, ncall) shaped as the reference
        (chain, step, dim), sampler.py:455-463.  On the fused path the step axis holds only the first and the
        last state unless the sampler was built with mcmc_history=True (nested.py:432-437 reads only those)."""
        if step_size <= 0.0:
            step_size = 2 / self.x_dim ** 0.5
        if self.mcmc_proposal == 'slice':
            return self._mcmc_sample_slice(mcmc_steps, step_size, init_samples, init_loglikes, init_derived, loglstar, walker_offset,
                                           seed)
        fused = (self._fused_like_id is not None and init_samples is not None and init_loglikes is not None
                 and prior_volume_steps == 1)   # loglstar None = the unconstrained branch, also in the kernel
        if fused:
            return self._mcmc_sample_fused(mcmc_steps, step_size, dynamic_step_size, init_samples, init_loglikes,
                                           loglstar, walker_offset, seed, form)
        return self._mcmc_sample_host(mcmc_steps, step_size, dynamic_step_size, num_chains, init_samples,
                                      init_loglikes, init_derived, loglstar, max_start_tries, prior_volume_steps)

    def _unit_box_on_x(self):
        """the NestedSampler's prior: the unit box on x, not on T(x) (`transform_prior=False`)"""
        p = self._user_prior
        return p is not None and not self._transform_prior and bool(getattr(p, 'is_unit_box', lambda: False)())

    def _slice_batch(self, z, logl, loglstar, step_size, mcmc_steps, walker_offset, seed, history=False, init_derived=None, rounds=False):
        """One batch of the slice proposal from (z, logl), both updated in place: the fused kernel where the flow has one for this
        population and the kernels know the likelihood (netG.slice_steps), else -- or with rounds=True, for a caller that needs
        hist_z / hist_logl -- nnest_amd.slice_rounds: the device likelihood when the kernels know it, else the host protocol
        (self.loglike on the rows whose likelihood decides, so it counts exactly sum n_call calls itself; the prior in place of the
        box unless it is the unit box).  With a device target for a regression likelihood of user data (`_slice_glm`): the fused
        kernel of that likelihood where the flow's `slice_glm_refusal` is None, else slice_rounds(like_glm=...); either way the rows
        stay on the device.  `slice_route` names what ran.  Initial bracket: twice the Metropolis step.  Books total_calls / total_accepted /
        total_rejected; returns (res, ncall).  One small device-to-host copy for the counts."""
        netG = self.trainer.netG
        C = z.shape[0]
        kw = dict(seed=self._next_seed() if seed is None else seed, walker_offset=walker_offset, history=history)
        args = (z, logl, float(loglstar), 2.0 * float(step_size), int(mcmc_steps))
        fused_slice = getattr(netG, 'supports_fused_slice', None)
        glm = self._slice_glm if self._fused_like_id is None else None
        if glm is not None:
            tk = glm.launch_kwargs(netG.device)
            tk = dict(like_glm=tk['like_glm'], t_std=tk['t_std'], t_mean=tk['t_mean'])
            refusal = getattr(netG, 'slice_glm_refusal', None)
            try:
                fused_glm = not rounds and refusal is not None and refusal(self.x_dim) is None
            except NotImplementedError:   # (a family without such a kernel)
                fused_glm = False
            if fused_glm:
                route = 'fused-glm'
                res = netG.slice_steps(None, 1.0, *args, **tk, **kw)
            else:
                from .slice_rounds import slice_rounds
                route = 'rounds-glm'
                res = slice_rounds(netG, *args, **tk, **kw)
        elif self._fused_like_id is None:
            from .slice_rounds import slice_rounds
            route = 'host'
            prior = None if self._unit_box_on_x() else (lambda x: self.prior(x) > -1e30)
            res = slice_rounds(netG, *args, loglike=self.loglike, prior=prior, num_derived=self.num_derived, init_derived=init_derived, **kw)
        elif rounds or (fused_slice is not None and not fused_slice(C)):
            from .slice_rounds import slice_rounds
            route = 'rounds'
            res = slice_rounds(netG, *args, like_id=self._fused_like_id, like_scale=self._linear_scale, like_params=self._fused_like_params, **kw)
        else:
            route = 'fused'
            res = netG.slice_steps(self._fused_like_id, self._linear_scale, *args, like_params=self._fused_like_params, **kw)
        if route != self.slice_route:
            self.slice_route = route
            if self.single_or_primary_process:
                self.logger.info('slice proposal route [%s]' % route)
        counts = torch.stack([res['n_call'].sum(), res['n_move'].sum()]).cpu()
        ncall, nmove = int(counts[0]), int(counts[1])
        if self._fused_like_id is not None or glm is not None:   # (a device likelihood: the host callable did not count these)
            self.total_calls += ncall
        self.total_accepted += nmove
        self.total_rejected += C * int(mcmc_steps) - nmove
        return res, ncall

    def _mcmc_sample_slice(self, mcmc_steps, step_size, init_samples, init_loglikes, init_derived, loglstar, walker_offset, seed):
        """_mcmc_sample with mcmc_proposal='slice': (samples, latent, derived, loglikes, scale, ncall) as _mcmc_sample_host returns
        them, with the step axis steps + 1.  BUILD-DEFINED (the reference has no slice proposal)."""
        if loglstar is None:
            raise NotImplementedError("mcmc_proposal='slice' samples under the hard constraint logL > loglstar only")
        if init_samples is None:
            raise NotImplementedError("mcmc_proposal='slice' starts from given points (init_samples)")
        netG = self.trainer.netG
        ncall0 = 0
        if init_loglikes is None or (self.num_derived > 0 and init_derived is None):
            init_loglikes, init_derived = self.loglike(init_samples)
            ncall0 = init_samples.shape[0]
        z, _ = netG.forward(init_samples)
        logl = torch.as_tensor(np.asarray(init_loglikes, dtype=np.float64)).to(z.device).contiguous()
        res, ncall = self._slice_batch(z, logl, loglstar, step_size, mcmc_steps, walker_offset, seed, history=True,
                                       init_derived=init_derived, rounds=True)
        C = z.shape[0]
        derived = res['hist_derived'] if res['hist_derived'] is not None else np.empty((C, int(mcmc_steps) + 1, 0))
        return (res['hist_x'].cpu().numpy(), res['hist_z'].cpu().numpy(), derived, res['hist_logl'].cpu().numpy(), float(step_size),
                ncall + ncall0)

    def _note_mh_route(self, route):
        """`mh_route`: what the last Metropolis batch ran; logged when it changes"""
        if route != self.mh_route:
            self.mh_route = route
            if self.single_or_primary_process:
                self.logger.info('Metropolis proposal route [%s]' % route)

    def _fused_launch(self, mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar, walker_offset, seed,
                      form=None, target=None):
        """One K4 launch from live points: returns (res, z0, z, logl) device-side (no host copies).  target: None -- the known
        likelihood (`_fused_like_id`, `_linear_scale`, `_fused_like_params`); a DeviceTarget with a like_glm (`_mh_glm`) -- the
        kernels of that likelihood (netG.mh_steps(like_glm=...)), with the same lag choice and the same fallback ladder; where the
        batch rule is refused and the flow has no per-tile rule (the NVP: one walker per wave) the result is None: the caller's
        batches go back to the host protocol."""
        netG = self.trainer.netG
        z, _ = netG.forward(init_samples)                               # sampler.py:264
        logl = torch.as_tensor(np.ascontiguousarray(init_loglikes, dtype=np.float64)).to(netG.device)
        z0 = z.clone()
        kw = dict(seed=self._next_seed() if seed is None else seed, walker_offset=walker_offset,
                  history=self.mcmc_history or self.chain_stats, like_params=self._fused_like_params, form=form)
        star = None if loglstar is None else float(loglstar)
        args = (self._fused_like_id, self._linear_scale, z, logl, star, float(step_size), int(mcmc_steps))
        if target is not None:
            tk = target.launch_kwargs(netG.device)
            kw = dict(seed=kw['seed'], walker_offset=walker_offset, history=kw['history'], like_glm=tk['like_glm'], t_std=tk['t_std'],
                      t_mean=tk['t_mean'])
            args = (None, 1.0) + args[2:]
        # dynamic: the reference's rule over the whole batch (sampler.py:422-431), `mcmc_step_lag` steps behind (0 = exactly
        # the reference; the default keeps the grid-wide wait off the step); populations too large for a
        # resident grid fall back to the per-16-walker rule
        mode = 'batch' if dynamic and getattr(self, '_batch_rule_ok', True) else ('group' if dynamic else False)
        lag = getattr(self, 'mcmc_step_lag', None)
        if lag is None and int(mcmc_steps) < 100:
            lag = 0   # short chains: the lag would be a sizeable part of the launch, and the exact rule costs microseconds here
        if getattr(self, 'mcmc_step_warm', None) is not None and target is None:
            kw['warm'] = int(self.mcmc_step_warm)
        if target is not None:
            # the same ladder in the `mh_glm` entries' terms: the `_check` entry is asked, nothing is launched and refused.  The spline
            # flow falls back to the per-tile rule; the NVP has none (one walker per wave): its batches go back to the host protocol
            if mode == 'batch':
                why = netG.mh_glm_refusal(self.x_dim, z.shape[0], 'batch', lag)
                if why is not None:
                    self._batch_rule_ok = False
                    mode = 'group'
                    per_tile = netG.mh_glm_refusal(self.x_dim, z.shape[0], 'group', None) is None
                    self.logger.warning('batch-wide step rule not available for %d walkers (%s); using %s' % (
                        z.shape[0], why, 'the per-group rule' if per_tile else 'the host protocol'))
            if mode == 'group' and netG.mh_glm_refusal(self.x_dim, z.shape[0], 'group', None) is not None:
                self._mh_glm = None
                return None, z0, z, logl
            return netG.mh_steps(*args, dynamic=mode, lag=lag, **kw), z0, z, logl
        try:
            res = netG.mh_steps(*args, dynamic=mode, lag=lag, **kw)
        except _lib.NnestHipError as e:
            if e.code != _lib.NNEST_E_UNSUPPORTED or (mode != 'batch' and form is None):
                raise
            # refused: the batch-wide rule on a grid that may not be resident, or a pinned form that does not apply to this
            # shape / rule, or exact warm-up steps asked of a form that has none (they belong to the solo form).
            res = None
            if mode == 'batch' and kw.get('warm', 0) > 0:
                # first the same rule WITHOUT the warm-up (the batch rule itself may well be available)
                try:
                    res = netG.mh_steps(*args, dynamic=mode, lag=lag, **dict(kw, warm=0))
                    if not getattr(self, '_warned_warm', False):
                        self.logger.warning('mcmc_step_warm=%d dropped: the kernel form for %d walkers has no exact warm-up steps' % (kw['warm'], z.shape[0]))
                        self._warned_warm = True
                    self.mcmc_step_warm = 0
                except _lib.NnestHipError as e2:
                    if e2.code != _lib.NNEST_E_UNSUPPORTED:
                        raise
            if res is not None:
                return res, z0, z, logl
            # Next: the per-group rule, with the form the library picks for it.
            if mode == 'batch':
                self.logger.warning('batch-wide step rule not available for %d walkers (%s); using the per-group rule' % (z.shape[0], e))
                self._batch_rule_ok = False
                mode = 'group'
            kw['form'] = None
            res = netG.mh_steps(*args, dynamic=mode, lag=lag, **kw)
        return res, z0, z, logl

    def _mcmc_sample_fused(self, mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar, walker_offset,
                           seed, form=None):
        netG = self.trainer.netG
        C = init_samples.shape[0]
        res, z0, z, logl = self._fused_launch(mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar,
                                              walker_offset, seed, form)
        ncall = int(res['n_call'].sum().item())
        nacc = int(res['n_accept'].sum().item())
        self._note_mh_route('fused')
        netG.check_sync(res)
        self.total_calls += ncall
        self.total_accepted += nacc
        self.total_rejected += C * int(mcmc_steps) - nacc
        if self.mcmc_history:
            samples = res['hist_x'].cpu().numpy()
            loglikes = res['hist_logl'].cpu().numpy()
            latent = np.stack([z0.cpu().numpy(), z.cpu().numpy()], axis=1)
        else:
            x0, _ = netG.inverse(z0)                                    # sampler.py:266
            samples = torch.stack([x0, res['x']], dim=1).cpu().numpy()
            loglikes = np.stack([np.asarray(init_loglikes, dtype=np.float64), logl.cpu().numpy()], axis=1)
            latent = torch.stack([z0, z], dim=1).cpu().numpy()
        derived = np.empty((C, samples.shape[1], 0))
        scale = float(res['scale'].mean().item()) if dynamic else float(step_size)
        return samples, latent, derived, loglikes, scale, ncall

    def _mcmc_endpoints_fused(self, mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar, walker_offset, seed,
                              form=None):
        """What the nested-sampling loop consumes of a batch (nested.py:432-437) -- per chain its end x, its end logL and whether
        every coordinate moved (the reference's test of a usable chain, evaluated here, where the start x exists) -- as ONE
        device tensor [C, D + 2] float64, so that the per-batch all-gather (C2) runs on device memory and carries no start
        points (round 2 gathered [C, 2 D + 1])."""
        netG = self.trainer.netG
        C = init_samples.shape[0]
        if self.mcmc_proposal == 'slice':
            # BUILD-DEFINED (the reference has no slice proposal): `mcmc_steps` slice-sampling updates per chain along random
            # directions of latent space.  Initial bracket: twice the Metropolis step (z + t * 2 step_size * eps, |eps| ~ sqrt(D): with
            # the default step_size = 1 / sqrt(D) a bracket of length ~2, the chord of a latent ball of radius sqrt(D) through a point
            # near its surface in a random direction); every update moves (no rejection), so the scale is not adapted -- stepping
            # out and shrinkage find the slice's extent
            if loglstar is None:
                raise NotImplementedError("mcmc_proposal='slice' samples under the hard constraint logL > loglstar only")
            z, _ = netG.forward(init_samples)
            logl = torch.as_tensor(np.asarray(init_loglikes, dtype=np.float64), device=z.device).contiguous()
            res, ncall = self._slice_batch(z, logl, loglstar, step_size, mcmc_steps, walker_offset, seed, history=self.chain_stats)
            self._chain_hist = res['hist_x'] if self.chain_stats else None
            ends = torch.cat([res['x'].double(), logl[:, None], res['moved'][:, None].double()], dim=1)
            return ends, float(step_size), ncall
        target = self._mh_glm if self._fused_like_id is None else None
        res, z0, z, logl = self._fused_launch(mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar,
                                              walker_offset, seed, None if target is not None else form, target=target)
        if res is None:   # (a regression likelihood of user data whose batch rule was refused, on a flow without a per-tile rule)
            return self._mcmc_endpoints_host(mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar)
        self._note_mh_route('fused-glm' if target is not None else 'fused')
        # "every coordinate moved" (nested.py:432: samples[:, 0] != samples[:, -1] in every dimension): the kernel's own test of the
        # chain's last x against its first x = f^-1(z_0), coordinate by coordinate (NNEST_MH_ALL_MOVED; round 4 took "accepted at
        # least once" for it, which differs once a proposal is so small that a coordinate of x does not change in float32)
        moved = res['moved']
        self._chain_hist = res['hist_x'] if self.chain_stats else None   # [C, steps + 1, D] on the device, read in place
        ends = torch.cat([res['x'].double(), logl[:, None], moved[:, None].double()], dim=1)
        counts = torch.stack([res['n_call'].sum(), res['n_accept'].sum()]).cpu()   # one small copy; orders the stream too
        netG.check_sync(res)
        ncall, nacc = int(counts[0]), int(counts[1])
        self.total_calls += ncall
        self.total_accepted += nacc
        self.total_rejected += C * int(mcmc_steps) - nacc
        scale = float(res['scale'].mean().item()) if dynamic else float(step_size)
        return ends, scale, ncall

    def _mcmc_endpoints_host(self, mcmc_steps, step_size, dynamic, init_samples, init_loglikes, loglstar):
        """`_mcmc_endpoints_fused`'s return from the host protocol (`_mcmc_sample_host`), for a batch the kernels refused: ends
        [C, D + 2] float64 on the flow's device -- the last x, the last logL, every coordinate moved (nested.py:432)"""
        s_x, _lat, _d, s_l, scale, nc = self._mcmc_sample_host(mcmc_steps, step_size, dynamic, init_samples.shape[0], init_samples,
                                                               init_loglikes, None, loglstar, 100, 1)
        moved = np.all(s_x[:, 0, :] != s_x[:, -1, :], axis=1)
        ends = np.concatenate([s_x[:, -1, :].astype(np.float64), s_l[:, -1, None], moved[:, None].astype(np.float64)], axis=1)
        return torch.as_tensor(ends, device=self.trainer.netG.device), scale, nc

    class _StepScale(object):
        """the proposal scale under the reference's adaptation rule (sampler.py:422-431): a step in which more than half of
        the chains moved votes up, any other step votes down; the scale follows whichever side leads"""

        def __init__(self, value):
            self.value, self.up, self.down = value, 0, 0

        def vote(self, moved, chains):
            if 2 * moved > chains:
                self.up += 1
            else:
                self.down += 1
            if self.up > self.down:
                self.value *= np.exp(1. / (1 + self.up))
            elif self.up < self.down:
                self.value /= np.exp(1. / (1 + self.down))

    def _propose(self, z, scale):
        """z + scale * N(0, I); with a fast/slow hierarchy a fraction `oversample_rate` of the proposals leaves the slow
        block alone (sampler.py:310-316, :377-382).  Returns (z', fast?)"""
        dz = torch.randn_like(z) * scale
        fast = self.num_slow > 0 and np.random.uniform() < self.oversample_rate
        if fast:
            dz[:, 0:self.num_slow] = 0.0
        return z + dz, fast

    @staticmethod
    def _metropolis_mask(log_ratio):
        """u < min(1, e^log_ratio) row by row (sampler.py:334-336): bool numpy array"""
        log_ratio = log_ratio if torch.is_tensor(log_ratio) else torch.as_tensor(log_ratio)
        return (torch.rand(log_ratio.shape) < log_ratio.exp().clamp(max=1)).numpy().astype(bool)

    def _mcmc_sample_host(self, mcmc_steps, step_size, dynamic, num_chains, init_samples, init_loglikes, init_derived,
                          loglstar, max_start_tries, prior_volume_steps):
        """The reference's step loop (sampler.py:246-463) with the flow passes on the GPU and the user's
        likelihood / prior callables on the host: the path for likelihoods the kernels do not know."""
        self._note_mh_route('host')
        tr = self.trainer
        tr.netG.eval()
        ncall = 0
        if init_samples is not None:
            num_chains = init_samples.shape[0]
            z, _ = tr.forward(init_samples)
            x = tr.get_samples(z, to_numpy=True)
            if init_loglikes is None or init_derived is None:
                logl, derived = self.loglike(x)
                ncall += num_chains
            else:
                logl, derived = np.array(init_loglikes, dtype=np.float64), init_derived
            logl_prior = self.prior(x)
        else:   # sampler.py:270-284: draw from the flow's base until every chain starts at finite density
            for attempt in range(max_start_tries):
                z = tr.get_prior_samples(num_chains)
                x = tr.get_samples(z, to_numpy=True)
                logl, derived = self.loglike(x)
                ncall += num_chains
                logl_prior = self.prior(x)
                if np.all(logl > -1e30) and np.all(logl_prior > -1e30):
                    break
            else:
                raise Exception('Could not find starting value')
        z = z if torch.is_tensor(z) else torch.as_tensor(z)
        hist = dict(x=[x], z=[z.cpu().numpy()], derived=[derived], logl=[logl])
        step = self._StepScale(step_size)
        for it in range(mcmc_steps):
            _, log_det_J = tr.inverse(z)                 # sampler.py:295 (x itself is carried: value-identical)
            fast = False
            if loglstar is not None:
                # hard constraint logl > loglstar.  Up to prior_volume_steps proposals from the CURRENT z; a chain keeps the
                # last one that passed the prior box and the Jacobian test (sampler.py:300-345), then its likelihood decides.
                z_prime, x_prime = z, x
                moved = np.zeros(num_chains, dtype=bool)
                for _ in range(prior_volume_steps):
                    z_try, fast = self._propose(z, step.value)
                    try:
                        x_try_t, log_det_J_try = tr.inverse(z_try)
                    except ValueError:           # a flow may refuse an inverse (sampler.py:322-324): proposal skipped
                        continue
                    x_try = x_try_t.cpu().numpy()
                    log_ratio = (log_det_J_try - log_det_J).cpu()
                    log_ratio[torch.as_tensor(self.prior(x_try) < -1e30)] = -np.inf
                    ok = self._metropolis_mask(log_ratio)
                    z_prime = torch.where(torch.as_tensor(ok, device=z.device)[:, None], z_try, z_prime)
                    x_prime = np.where(ok[:, None], x_try, x_prime)
                    moved |= ok
                mask = moved
                logl_prior_prime = self.prior(x_prime)
                logl_prime = np.array(logl, dtype=np.float64, copy=True)
                derived_prime = np.copy(derived)
                cand = np.flatnonzero(mask)
                if cand.size:                    # the likelihood is evaluated only where the cheap tests passed (:358-368)
                    lp, der = self.loglike(x_prime[cand])
                    ncall += cand.size
                    if fast:
                        self.total_fast_calls += cand.size
                    good = np.isfinite(lp) & (lp > loglstar)
                    logl_prime[cand[good]] = lp[good]
                    derived_prime[cand[good]] = der[good]
                    mask[cand[~good]] = False
            else:
                # no constraint: likelihood and prior enter the Metropolis ratio (sampler.py:372-413)
                z_prime, fast = self._propose(z, step.value)
                try:
                    x_prime_t, log_det_J_prime = tr.inverse(z_prime)
                except ValueError:
                    continue
                x_prime = x_prime_t.cpu().numpy()
                ncall += num_chains
                if fast:
                    self.total_fast_calls += num_chains
                logl_prime, derived_prime = self.loglike(x_prime)
                logl_prior_prime = self.prior(x_prime)
                mask = self._metropolis_mask((log_det_J_prime - log_det_J).cpu() + torch.as_tensor(logl_prime - logl)
                                             + torch.as_tensor(logl_prior_prime - logl_prior))
            n_moved = int(mask.sum())
            self.total_accepted += n_moved
            self.total_rejected += num_chains - n_moved
            if dynamic:
                step.vote(n_moved, num_chains)
            sel = mask[:, None]
            logl = np.where(mask, logl_prime, logl)
            logl_prior = np.where(mask, logl_prior_prime, logl_prior)
            z = torch.where(torch.as_tensor(sel, device=z.device), z_prime, z)
            x = np.where(sel, x_prime, x)
            derived = np.where(sel, derived_prime, derived)
            for k, v in (('x', x), ('z', z.cpu().numpy()), ('derived', derived), ('logl', logl)):
                hist[k].append(v)
        chain_major = lambda a: np.moveaxis(np.array(a), 0, 1)   # (step, chain, ...) -> (chain, step, ...)  sampler.py:455-459
        return (chain_major(hist['x']), chain_major(hist['z']), chain_major(hist['derived']), chain_major(hist['logl']),
                step.value, ncall)

    # ---- prior rejection (sampler.py:529-543) ---------------------------------------------------------------
    def _rejection_prior_sample(self, loglstar, num_trials=None):
        if num_trials is None and self._fused_like_id is not None:
            # The reference draws one prior sample per likelihood call until one passes (sampler.py:531-538).  The
            # draws are independent, so the same rule is applied to a block per launch of the likelihood kernel: the
            # first candidate above loglstar is returned and ncall counts the candidates examined up to and including it.
            # Round 4: candidates a launch evaluated but the caller did not reach (they lie behind the accepted one) are independent
            # prior draws like any other, so they are KEPT and examined first by the next call (against its higher loglstar), each
            # exactly once and in order: one launch + one read-back now serves several iterations of the outer loop instead of one
            # (5 264 calls of 0.11 ms in a config-2 run, latency-bound).
            # Each block keeps the (sorted) indices of its candidates above the threshold AT ITS CREATION with their float64 likelihoods
            # from one vectorised host call: the threshold only rises, so every later hit is among them, and a call walks a pointer
            # instead of searching the block (config 3: 8 371 calls, 0.59 s of a 1.9 s run before).
            from . import flow
            ncall = 0
            cache = getattr(self, '_prior_cache', None)
            while True:
                if cache is None or cache['pos'] >= len(cache['logl']) or loglstar < cache['star0']:   # (a LOWER threshold than the block was indexed for: start afresh)
                    block = getattr(self, '_prior_block', 256)
                    x = self.sample_prior(block)
                    logl = flow.loglike(self._fused_like_id, x, self._linear_scale, device=self.trainer.netG.device,
                                        like_params=self._fused_like_params).cpu().numpy()
                    cand = np.flatnonzero(logl > loglstar)
                    l64 = d64 = None
                    if len(cand):   # the kernel works on float32(x); the stored value is the reference's float64 one
                        calls = self.total_calls
                        l64, d64 = self.loglike(x[cand])
                        self.total_calls = calls
                    cache = self._prior_cache = dict(x=x, logl=logl, pos=0, hits=0, cand=cand, k=0, l64=l64, d64=d64, star0=loglstar)
                x, logl, pos, cand, k = cache['x'], cache['logl'], cache['pos'], cache['cand'], cache['k']
                found = None
                while k < len(cand):
                    j = int(cand[k])
                    if j >= pos and logl[j] > loglstar and cache['l64'][k] > loglstar:
                        found = (j, k)
                        break
                    k += 1
                if found is not None:
                    j, k = found
                    self.total_calls += j + 1 - pos
                    cache['pos'], cache['k'] = j + 1, k + 1
                    cache['hits'] += 1
                    # the next block: ~ 16 acceptances' worth of candidates at the rate seen, bounded
                    self._prior_block = int(min(65536, max(256, 16 * (j + 1) / cache['hits'])))
                    return x[j:j + 1], cache['l64'][k:k + 1], cache['d64'][k:k + 1], ncall + j + 1 - pos
                self.total_calls += len(logl) - pos
                ncall += len(logl) - pos
                if cache['hits'] == 0:
                    self._prior_block = int(min(65536, 4 * len(logl)))
                cache = self._prior_cache = None
        if num_trials is not None:   # a fixed block of prior draws; ncall = expected draws per success (sampler.py:540-542)
            x = self.sample_prior(num_trials)
            logl, derived = self.loglike(x)
            return x, logl, derived, num_trials / np.sum(logl > loglstar)
        for ncall in itertools.count(1):   # one prior draw per likelihood call until one lies above loglstar (:531-538)
            x = self.sample_prior(1)
            logl, derived = self.loglike(x)
            if logl > loglstar:
                return x, logl, derived, ncall

    # ---- flow rejection (sampler.py:545-605) and density sampling (sampler.py:607-628) ----------------------------
    # The reference draws one candidate, inverts it, tests it, and loops.  Candidates are independent, so the same
    # chain of decisions is taken here over a block of candidates per launch: candidates are examined in order, the
    # first that passes every test is returned, and `ncall` counts -- as the reference does -- the candidates that
    # reached the likelihood test (box prior and Jacobian envelope passed) up to and including the accepted one.
    def _candidate_block(self, z):
        """x, log|dx/dz|, logl for a block of latent candidates; logl is None when the likelihood is a host callable."""
        netG = self.trainer.netG
        if self._fused_like_id is not None:
            x, ld, logl, inbox = netG.inverse_loglike(self._fused_like_id, self._linear_scale, z,
                                                      like_params=self._fused_like_params)
            return x.cpu().numpy().astype(np.float64), ld.cpu().numpy().astype(np.float64), logl.cpu().numpy(), \
                inbox.cpu().numpy().astype(bool)
        x, ld = netG.inverse(z)
        x = x.cpu().numpy().astype(np.float64)
        return x, ld.cpu().numpy().astype(np.float64), None, self.prior(x) > -1e30

    def _first_accepted(self, x, passed, logl, loglstar, strict):
        """Walk the candidates that passed the cheap tests in order; returns (index or None, likelihood calls made)."""
        idx = np.where(passed)[0]
        if logl is not None:                       # likelihood already evaluated in the launch
            good = logl[idx] > loglstar if strict else ~(np.isfinite(logl[idx]) & (logl[idx] < loglstar))
            hit = np.where(good)[0]
            if len(hit) == 0:
                self.total_calls += len(idx)
                return None, len(idx), None, None
            self.total_calls += int(hit[0]) + 1
            j = idx[hit[0]]
            return j, int(hit[0]) + 1, logl[j:j + 1], np.empty((1, 0))
        calls = 0
        for lo in range(0, len(idx), 16):          # host callable: evaluate in small groups, stop at the first hit
            grp = idx[lo:lo + 16]
            before = self.total_calls
            lg, dg = self.loglike(x[grp])
            good = lg > loglstar if strict else ~(np.isfinite(lg) & (lg < loglstar))
            hit = np.where(good)[0]
            if len(hit) > 0:
                # the reference evaluates one candidate per call and stops at the accepted one: the rest of the group is
                # not counted, neither in the returned ncall nor in total_calls
                self.total_calls = before + int(hit[0]) + 1
                return grp[hit[0]], calls + int(hit[0]) + 1, lg[hit[0]:hit[0] + 1], dg[hit[0]:hit[0] + 1]
            calls += len(grp)
        return None, calls, None, None

    def _rejection_flow_sample(self, init_samples, loglstar, enlargement_factor=1.1, constant_efficiency_factor=None,
                               cache=False, block=256):
        netG = self.trainer.netG

        def get_cache():
            z, log_det_J = netG.forward(init_samples)
            # envelope for the rejection step: max log|dx/dz| over the live points (sampler.py:556-561)
            self.max_log_det_J = enlargement_factor * float(torch.max(-log_det_J).item())
            self.max_r = float(np.max(np.linalg.norm(z.cpu().numpy(), axis=1)))

        if not cache or not hasattr(self, 'max_log_det_J'):
            get_cache()
        if constant_efficiency_factor is not None:
            enlargement_factor = (1 / constant_efficiency_factor) ** (1 / self.x_dim)
        ncall = 0
        while True:
            prior = getattr(netG, 'prior', None)
            if hasattr(prior, 'usample'):   # sampler.py:575-576: uniform box of the generalised-normal base
                z = np.asarray(prior.usample(sample_shape=(block,))).reshape(block, self.x_dim) * enlargement_factor
            else:                           # uniform in the ball of radius enlargement * max_r (sampler.py:579-583)
                z = np.random.randn(block, self.x_dim)
                r = enlargement_factor * self.max_r * np.random.rand(block) ** (1. / self.x_dim)
                z = z * (r / np.sqrt(np.sum(z ** 2, axis=1)))[:, None]
            rnd_u = np.random.rand(block)
            x, ld, logl, inbox = self._candidate_block(z)
            with np.errstate(over='ignore', invalid='ignore'):
                ratio = np.minimum(np.exp(ld - self.max_log_det_J), 1.0)
            # first test (sampler.py:593-597): Jacobian envelope; the second (sampler.py:599-604) zeroes the ratio
            # where logl is finite and below loglstar and repeats rnd_u < ratio
            passed = inbox & (rnd_u < ratio)
            j, calls, lj, dj = self._first_accepted(x, passed, logl, loglstar, strict=False)
            ncall += calls
            if j is not None:
                return x[j:j + 1], lj, dj, ncall
            block = min(4 * block, 65536)

    def _density_sample(self, loglstar, block=256):
        ncall = 0
        while True:
            z = self.trainer.get_prior_samples(block)
            x, ld, logl, inbox = self._candidate_block(z)
            j, calls, lj, dj = self._first_accepted(x, inbox, logl, loglstar, strict=True)
            ncall += calls
            if j is not None:
                return x[j:j + 1], lj, dj, ncall
            block = min(4 * block, 65536)

    # ---- ensemble sampling (sampler.py:632-724): emcee's stretch move in latent space, build-defined stream -----------------
    ENSEMBLE_HISTORY_BYTES = 256 << 20   # device history per launch; longer runs are cut into launches of fewer steps

    def _ensemble_affine(self):
        """T as (std, mean) per dimension when the transform is x * std + mean (EnsembleSampler.run installs one), else None"""
        aff = getattr(self, '_ensemble_transform', None)
        if aff is not None:
            return aff
        if self._user_transform is None:
            return np.ones(self.x_dim), np.zeros(self.x_dim)
        if self._linear_scale is not None:
            return np.full(self.x_dim, self._linear_scale), np.zeros(self.x_dim)
        return None

    ENTRY_NEEDS = {'mcmc': ('mcmc',), 'mcmc_tempered': ('mcmc', 'mcmc_tempered'), 'importance': ('importance',),
                   'mcmc_mixed': ('mcmc', 'mcmc_mixed'), 'mcmc_adapt': ('mcmc', 'mcmc_adapt')}
    ENTRY_KERNEL = {'mcmc': 'random-walk Metropolis', 'mcmc_tempered': 'tempered random-walk Metropolis', 'importance': 'importance-sampling',
                    'mcmc_mixed': 'mixed (local and global step) Metropolis', 'mcmc_adapt': 'adaptive-step Metropolis'}

    GDATA_ENTRIES = ('mcmc', 'mcmc_tempered', 'mcmc_mixed', 'mcmc_adapt')   # what the `mcmc_gdata` entry of a flow stands in for

    def _device_target(self, affine=None, entry=None, unit_box_on_x=False):
        """(target, None) where the likelihood and the prior run on the device under the transform `affine` = (std, mean) (None:
        `_ensemble_affine()`), else (None, what is not taken: the words the front ends put after 'the fused route does not take').
        A DeviceTarget: no derived parameters, a likelihood the kernels know that agrees with the host callable on T(x), and no prior
        or a UniformPrior on T(x) -- with `unit_box_on_x` (the evidence) also the NestedSampler's prior, the unit box on x under
        x -> s * x (`_linear_scale`): the box on T(x) is +-|s|.  `entry` names the flow entry a front end needs bound ('mcmc',
        'mcmc_tempered', 'mcmc_mixed' and 'mcmc_adapt' -- which need 'mcmc' too --, 'importance'): every parameter must then be fast
        and, for 'importance', 'mcmc_mixed' and 'mcmc_adapt', the library must take the flow's shape and base (`importance_refusal`,
        `mcmc_mixed_refusal`, `mcmc_adapt_refusal`: nothing is launched).  The ensemble routes name none:
        they fall back to rounds.  One probe of the host callable (`_probe_agrees`) per call: a run resolves once and hands the
        target down.  A likelihood without an id but with a `hip_like_data` (likelihoods.GaussianData) is taken for the Metropolis
        entries (GDATA_ENTRIES) where the flow's `mcmc_gdata` entry is bound and takes the flow (`mcmc_gdata_refusal`) and the
        descriptor agrees with the host callable (`_probe_agrees_gdata`): the target then has like_id None and the data.  Likewise
        a likelihood with a `hip_like_glm` (likelihoods.GLMData): the flow's `mcmc_glm` entry, `mcmc_glm_refusal`,
        `_probe_agrees_glm`.  Entry 'mh_glm' (the NestedSampler's Metropolis proposal) takes such a likelihood under mcmc_proposal='mh',
        the unit box on x and x -> s * x where the flow binds `mh_glm` and takes the shape (`mh_glm_refusal`).  Entry 'slice_glm' (the NestedSampler's slice proposal; `unit_box_on_x` goes with it) takes such a
        likelihood, and nothing else, under mcmc_proposal='slice', the unit box on x and x -> s * x, with any flow and fast/slow
        parameters too: `_slice_batch` chooses between the fused kernel and the round driver.  Beside such a likelihood, and only there, a priors.GaussianPrior on T(x) whose `__call__` is its own
        is taken where the flow binds `mcmc_glm_prior` and takes the shape (`mcmc_glm_prior_refusal`) and the prior's
        `hip_gauss_prior` agrees with its callable (`_probe_agrees_gauss_prior`): the target then carries `prior_gauss` and no box.
        With any other likelihood, entry or flow a GaussianPrior stays a Python prior: refused here, the host route's.
        For entry 'importance' a `hip_like_glm` is taken where the flow binds `importance_glm` and takes the shape and base
        (`importance_glm_refusal`), the descriptor agrees with the host callable and there is a PROPER prior: a UniformPrior on T(x)
        whose rule is its own or the unit box on x (the box), or a GaussianPrior on T(x) whose `__call__` is its own (`prior_gauss`
        through the same entry, no box).  A GLMData with NO prior is not taken, in the words a Python callable gets: the integral of
        a regression likelihood over R^D is not an evidence, and is infinite for separable classes"""
        affine = self._ensemble_affine() if affine is None else affine
        netG = self.trainer.netG
        if self.num_derived != 0:
            return None, 'derived parameters (num_derived=%d)' % self.num_derived
        if entry not in (None, 'slice_glm') and self.num_slow != 0:   # (the slice proposal's round driver takes any flow)
            return None, 'the fast/slow proposal (num_slow=%d)' % self.num_slow
        for need in self.ENTRY_NEEDS.get(entry, ()):
            if need not in getattr(netG, '_sym', ()):
                return None, 'the flow %s (no fused %s kernel)' % (type(netG).__name__, self.ENTRY_KERNEL[need])
        like = self._user_loglike
        like_id = getattr(like, 'hip_like_id', None)
        like_data = getattr(like, 'hip_like_data', None) if like_id is None else None
        if like_data is not None and not (entry in self.GDATA_ENTRIES and 'mcmc_gdata' in getattr(netG, '_sym', ())):
            like_data = None
        like_glm = getattr(like, 'hip_like_glm', None) if like_id is None and like_data is None else None
        prior = self._user_prior
        gauss_own = self._transform_prior and isinstance(prior, GaussianPrior) and type(prior).__call__ is GaussianPrior.__call__
        glm_evidence = False   # (the evidence of a regression: the flow's `importance_glm` entry, and a PROPER prior)
        if like_glm is not None and entry == 'importance':
            proper = (gauss_own or (unit_box_on_x and self._unit_box_on_x() and self._linear_scale is not None)
                      or (self._transform_prior and isinstance(prior, UniformPrior) and type(prior).__call__ is UniformPrior.__call__))
            glm_evidence = proper and 'importance_glm' in getattr(netG, '_sym', ())
        # (the slice proposal on a regression: the NestedSampler's prior, the unit box on x under x -> s * x.  Any flow: the fused kernel
        # or the round driver is `_slice_batch`'s choice, batch by batch)
        # (entry 'mh_glm': the same under mcmc_proposal='mh', with a flow that binds the `mh_glm` entry and whose shape it takes --
        # there is no round driver behind the Metropolis proposal; population and step rule are `_fused_launch`'s, batch by batch)
        nested_glm = {'slice_glm': 'slice', 'mh_glm': 'mh'}.get(entry)
        glm_slice = (nested_glm is not None and like_glm is not None and self.mcmc_proposal == nested_glm and self._unit_box_on_x()
                     and self._linear_scale is not None)
        if nested_glm is not None and not glm_slice:
            return None, ("anything but mcmc_proposal='%s' on a likelihood with a hip_like_glm (likelihoods.GLMData) under the unit box on x and "
                          "x -> s * x" % nested_glm)
        if entry == 'mh_glm':
            if 'mh_glm' not in getattr(netG, '_sym', ()):
                return None, 'the flow %s (no fused Metropolis kernel on a regression likelihood of user data)' % type(netG).__name__
            why = netG.mh_glm_refusal(np.shape(like_glm['at'])[0])
            if why is not None:
                return None, 'the flow %s: %s' % (type(netG).__name__, why)
        if like_glm is not None and not glm_evidence and not glm_slice and not (entry in self.GDATA_ENTRIES and 'mcmc_glm' in getattr(netG, '_sym', ())):
            like_glm = None
        if like_id is None and like_data is None and like_glm is None:
            return None, 'a likelihood the kernels do not know (a Python callable)'
        prior_gauss = None   # (normal priors: beside a regression likelihood of user data only)
        if like_glm is not None and gauss_own and (glm_evidence or 'mcmc_glm_prior' in getattr(netG, '_sym', ())):
            prior_gauss = prior.hip_gauss_prior
        if glm_slice:
            entry = None
        elif like_glm is not None:   # (as below for like_data: one kernel per flow and family serves the four entries)
            ask = netG.importance_glm_refusal if glm_evidence else netG.mcmc_glm_refusal if prior_gauss is None else netG.mcmc_glm_prior_refusal
            why = ask(np.shape(like_glm['at'])[0])
            if why is not None:
                return None, 'the flow %s: %s' % (type(netG).__name__, why)
            entry = None
        if like_data is not None:   # (one kernel per family serves the four entries: its shapes and base, in the library's words)
            why = netG.mcmc_gdata_refusal(len(like_data['mu']))
            if why is not None:
                return None, 'the flow %s: %s' % (type(netG).__name__, why)
            entry = None   # (the checks by id below are not this likelihood's)
        if entry == 'importance':
            why = netG.importance_refusal(like_id)
            if why is not None:
                return None, 'the flow %s: %s' % (type(netG).__name__, why)
        if entry == 'mcmc_mixed':   # (the global step draws from the base: its shape and N(0, I), in the library's words)
            why = netG.mcmc_mixed_refusal(like_id)
            if why is not None:
                return None, 'the flow %s: %s' % (type(netG).__name__, why)
        if entry == 'mcmc_adapt':   # (the adaptive kernels are the mixed walk's: the same shapes and base, in the library's words)
            why = netG.mcmc_adapt_refusal(like_id)
            if why is not None:
                return None, 'the flow %s: %s' % (type(netG).__name__, why)
        refused ='this transform, likelihood or prior (an affine transform, a likelihood that agrees with the kernel\'s, and no prior%s)' % (
            ', a UniformPrior on T(x) or the unit box on x' if unit_box_on_x else ' or a UniformPrior on T(x)')
        refused = refused[:-1] + ', or a GaussianPrior with a GLMData)'
        box = (None, None)
        if unit_box_on_x and self._unit_box_on_x() and self._linear_scale is not None:
            s = np.full(self.x_dim, abs(float(self._linear_scale)), np.float32)
            box = (-s, s)
        elif prior_gauss is not None:   # (no box beside it)
            pass
        elif prior is not None:   # (a UniformPrior on T(x) whose rule is its own, or refused)
            ok = self._transform_prior and isinstance(prior, UniformPrior) and type(prior).__call__ is UniformPrior.__call__
            box = (prior.minimum, prior.maximum) if ok else None
        params = tuple(getattr(like, 'hip_like_params', ()) or ())
        if like_glm is not None:
            if affine is None or box is None or not self._probe_agrees_glm(like_glm, affine, warn=('%s: ' % nested_glm) if glm_slice else 'mcmc: '):
                return None, refused
            if prior_gauss is not None and (box != (None, None) or not self._probe_agrees_gauss_prior(prior_gauss, affine, warn='mcmc: ')):
                return None, refused
            return DeviceTarget(None, (), affine[0], affine[1], *box, like_glm=like_glm, prior_gauss=prior_gauss), None
        if like_data is not None:
            if affine is None or box is None or not self._probe_agrees_gdata(like_data, affine, warn='mcmc: '):
                return None, refused
            return DeviceTarget(None, (), affine[0], affine[1], *box, like_data=like_data), None
        if affine is None or box is None or not self._probe_agrees(like_id, params, affine=affine, warn='ensemble: '):
            return None, refused
        return DeviceTarget(like_id, params, affine[0], affine[1], *box), None

    def _install_transform(self, mean, std):
        """T(x) = x * std + mean, also as per-dimension float arrays for the device routes"""
        self.transform = lambda x: x * std + mean
        self._ensemble_transform = (np.asarray(std, np.float64), np.asarray(mean, np.float64))
        self._linear_scale = None   # (the Metropolis kernels only know x -> s * x)
        self._fused_like_id = None
        self._slice_glm = None
        self._mh_glm = None

    # ---- importance-sampled evidence from the trained flow (build-defined: the reference has none) ---------------------------------
    IMPORTANCE_CHUNK = 1 << 22   # samples per launch when nothing per sample comes back

    def _importance_constant(self, affine):
        """what turns the weights' log Z over x into `importance_evidence`'s logz (its docstring has the convention)"""
        if self._user_prior is not None and not self._transform_prior:   # a prior on x: Z over x is the evidence already
            return -self.x_dim * np.log(2.0) if self._unit_box_on_x() else 0.0   # (the unit box, normalised: 2^-D)
        if affine is None:
            return 0.0
        return float(np.sum(np.log(np.abs(np.asarray(affine[0], np.float64)))))

    def _importance_host_sums(self, n):
        """the sums (a, S1, S2, n_live) of n samples of the flow with the user's callables on the host, and (T(x), logw)"""
        netG = self.trainer.netG
        x_t = netG.sample(int(n))
        logq = netG.log_probs(x_t).double().cpu().numpy()
        x = x_t.cpu().numpy()
        logl, _ = self.loglike(x)                  # (safe: non-finite -> -1e100; counts the calls)
        logw = logl + np.asarray(self.prior(x), np.float64) - logq
        live = ~(np.isnan(logw) | (logw == -np.inf))
        if not live.any():
            return (-np.inf, 0.0, 0.0, 0.0), x, logw
        a = float(np.max(logw[live]))
        e = np.exp(logw[live] - a)
        return (a, float(e.sum()), float((e * e).sum()), float(live.sum())), x, logw

    def importance_evidence(self, num_samples, seed=None, route=None, chunk=None, return_samples=False):
        """The evidence by importance sampling with the trained flow as the proposal (build-defined; the reference has none):
        Z = E_q[L(T(x)) pi(T(x)) / q(x)] over `num_samples` exact draws of the flow -- an estimate that does not depend on how well
        any chain has mixed, with an error bar and an effective sample size.  For every front end, once a flow has been trained.
        route: 'fused' -- drawn, evaluated and reduced inside the kernel (include/nnest_hip.h nnest_importance_evidence,
        nnest_spline_importance_evidence; for a likelihoods.GLMData under a proper prior -- a UniformPrior, the unit box or a
        priors.GaussianPrior -- nnest_importance_glm_evidence, nnest_spline_importance_glm_evidence; a GLMData with no prior is
        not taken: the integral of a regression likelihood over R^D is not an evidence, and is infinite for separable classes),
        in launches of `chunk` samples addressed by their global index (the cut does not change
        a sample; chunk defaults to 2^22, or by ENSEMBLE_HISTORY_BYTES when samples come back); taken where `_device_target`
        gives a target (a likelihood the kernels know, no derived or slow parameters, an affine transform, no prior or a
        UniformPrior on T(x), HipNVP in the default shape or HipSpline) or the prior is the NestedSampler's unit box on x, and the
        base is N(0, I); ValueError, naming what is not taken, otherwise.  'host' -- netG.sample / netG.log_probs with the
        likelihood and the prior as the host Metropolis route evaluates them: every flow, base, prior and Python likelihood.
        None -- 'fused' where it is taken, 'host' otherwise.  seed: the fused route's Philox seed (None: `_next_seed()`).
        CONVENTION of logz: the weights estimate Z over x.  With no prior, or a prior evaluated on T(x) (`transform_prior`, the
        default), and an affine transform, sum log|t_std| is added: the result is log of the integral of L(theta) pi(theta) d theta
        with pi as the prior callable returns it (the UniformPrior is the UNNORMALISED indicator of its box); under a transform that
        is not affine (host route only) nothing is added and Z stays over x.  With a prior evaluated on x (`transform_prior=False`)
        Z over x is the evidence already and nothing is added, whatever the transform; where that prior is the unit box on x
        (NestedSampler) it is taken as the normalised 2^-D and the result is logz_x - D log 2: directly comparable with
        NestedSampler's `logz`.
        Returns a dict: logz, logzerr (the delta-method standard error of log Z), ess, n_samples, n_live, max_weight_share, route;
        with return_samples also samples (T(x), as `self.transform` gives it) [n, D] and logw [n] (the log weights over x:
        logsumexp(logw) - log n is logz less the convention's constant).  Leaves the route in `importance_route`, logs one line."""
        if route not in (None, 'host', 'fused'):
            raise ValueError("route=%r: None, 'host' or 'fused'" % (route,))
        M = int(num_samples)
        if M < 1:
            raise ValueError('importance_evidence: num_samples=%d' % M)
        target, why = (None, None) if route == 'host' else self._device_target(entry='importance', unit_box_on_x=True)
        if route == 'fused' and why is not None:
            raise ValueError('importance_evidence: the fused route does not take %s' % why)
        route = 'host' if target is None else 'fused'
        D = self.x_dim
        parts, xs, lws = [], [], []
        if route == 'fused':
            netG = self.trainer.netG
            kw = target.launch_kwargs(netG.device)
            seed = self._next_seed() if seed is None else int(seed)
            if chunk is None:
                chunk = max(1, self.ENSEMBLE_HISTORY_BYTES // (8 * D + 16)) if return_samples else self.IMPORTANCE_CHUNK
            chunk = max(1, min(int(chunk), 1 << 30))
            sums = []
            for first in range(0, M, chunk):
                k = min(chunk, M - first)
                res = netG.importance_evidence(target.like_id, k, seed=seed, sample_offset=first, want_samples=return_samples, **kw)
                sums.append(res['sums'])
                if return_samples:
                    xs.append(res['x'].cpu().numpy())
                    lws.append(res['logw'].cpu().numpy())
            parts = [tuple(t.cpu().numpy()) for t in sums]
            self.total_calls += M
        else:
            if chunk is None:
                chunk = 1 << 16
            chunk = max(1, int(chunk))
            for first in range(0, M, chunk):
                p, x, lw = self._importance_host_sums(min(chunk, M - first))
                parts.append(p)
                if return_samples:
                    xs.append(x)
                    lws.append(lw)
        const = self._importance_constant(self._ensemble_affine())
        a, s1, s2, n_live = _lib.merge_importance(parts)
        r = _lib.importance_result(a, s1, s2, n_live, M)
        out = dict(logz=r['logz_x'] + const if r['logz_x'] > -np.inf else -np.inf, logzerr=r['logzerr'], ess=r['ess'], n_samples=M,
                   n_live=r['n_live'], max_weight_share=r['max_weight_share'], route=route)
        if return_samples:
            out['samples'] = np.asarray(self.transform(np.concatenate(xs, axis=0)))
            out['logw'] = np.concatenate(lws, axis=0)
        self.importance_route = route
        if self.single_or_primary_process:
            self.logger.info('importance: log Z [%5.4f +- %5.4f] ESS [%.1f of %d] live [%d] max weight share [%.3g] route [%s]' % (
                out['logz'], out['logzerr'], out['ess'], M, out['n_live'], out['max_weight_share'], route))
        return out

    def _mcmc_sample_device(self, mcmc_steps, step_size=0.0, num_chains=1, init_samples=None, max_start_tries=100, output_interval=None,
                            stats_interval=None, seed=None, chunk_steps=None, target=None, global_every=0, adapt_steps=0,
                            target_accept=0.234):
        """`_mcmc_sample` with loglstar = None (sampler.py:372-416: the likelihood, the prior and the Jacobian in the ratio) with every
        step of a launch inside the kernel (include/nnest_hip.h nnest_mcmc_steps, nnest_spline_mcmc_steps).  BUILD-DEFINED STREAM,
        THE REFERENCE'S MOVE: parity with the host route's torch stream is statistical.  The step is fixed (`step_size`, <= 0: the
        reference's 2 / sqrt(x_dim)).  Starts: forward(init_samples), or draws of the flow's base, the whole batch redrawn while any
        chain's target is <= -1e30, up to `max_start_tries` times (sampler.py:275-284).  The run is cut into launches of `chunk_steps`
        steps (default: by device memory, ENSEMBLE_HISTORY_BYTES) and at `output_interval`; the cut does not change it.  Returns the
        reference's tuple (samples [N, S + 1, D] (x, before the transform: the start, then every step), latent_samples [N, S + 1, D],
        derived_samples [N, S + 1, 0], loglikes [N, S + 1] (logL), scale, ncall).  `target`: the run's DeviceTarget where the caller
        has resolved it (`_device_target(entry='mcmc')`); None: resolved here, ValueError naming what is not taken.
        global_every = k > 0 (build-defined; include/nnest_hip.h nnest_mcmc_mixed_steps): every k-th step of the run -- step t where
        (t + 1) % k == 0 -- is a flow-independence ("global") step: the proposal is a draw of the flow's base, accepted on the ratio
        of importance weights, through the family's mixed kernel (`_device_target(entry='mcmc_mixed')`: the base must be N(0, I)).
        The run leaves `global_proposed` and `global_accepted` on the sampler and logs the global acceptance rate -- the figure
        that says how good the flow is as a proposal.  0: the run as it was.
        adapt_steps = A > 0 (build-defined; include/nnest_hip.h nnest_mcmc_adapt_steps): every chain adapts its own step over the
        local steps t < A of the run -- a Robbins-Monro rule on its own decisions towards the acceptance `target_accept` -- and keeps
        it from there on, through the family's adaptive kernel (`_device_target(entry='mcmc_adapt')`); the chains' steps are handed
        from launch to launch, so the cut still does not change the run.  The run leaves `step_sizes` [N] (the chains' steps at its
        end), `adapt_acceptance` (of the local steps t < A) and `frozen_acceptance` (of the local steps t >= A; nan where there are
        none) on the sampler and logs the three.  0: the run as it was."""
        global_every, adapt_steps = int(global_every), int(adapt_steps)
        if global_every < 0:
            raise ValueError('mcmc: global_every=%d (every how many steps a global step is taken: >= 0)' % global_every)
        if adapt_steps < 0:
            raise ValueError('mcmc: adapt_steps=%d (over how many steps of the run the chains adapt their step: >= 0)' % adapt_steps)
        if target is None:
            target, why = self._device_target(entry='mcmc_adapt' if adapt_steps else 'mcmc_mixed' if global_every else 'mcmc')
            if why is not None:
                raise ValueError('mcmc: the fused route does not take %s' % why)
        S = int(mcmc_steps)
        if step_size <= 0.0:
            step_size = 2 / self.x_dim ** 0.5
        D = self.x_dim
        netG = self.trainer.netG
        seed = self._next_seed() if seed is None else int(seed)
        kw = dict(target.launch_kwargs(netG.device), seed=seed)
        if init_samples is not None:
            z, _ = netG.forward(init_samples)
            z = z.contiguous()
            start, tries = netG.mcmc_steps(target.like_id, z, 0, step_size, **kw), 1
        else:
            for tries in range(1, int(max_start_tries) + 1):
                z = netG.prior_sample(int(num_chains)).contiguous()
                start = netG.mcmc_steps(target.like_id, z, 0, step_size, **kw)
                if bool((start['lp'] > -1e30).all().item()):
                    break
            else:
                raise Exception('Could not find starting value')
        N = z.shape[0]
        samples = np.empty((N, S + 1, D), np.float32)
        latent = np.empty((N, S + 1, D), np.float32)
        loglikes = np.empty((N, S + 1))
        derived = np.zeros((N, S + 1, 0))
        samples[:, 0], latent[:, 0], loglikes[:, 0] = start['x'].cpu().numpy(), z.cpu().numpy(), start['logl'].cpu().numpy()

        mixed = dict(global_every=global_every) if global_every else {}   # (0: the call as it was)
        n_global = [0]

        def launch(k, done, state):
            res = netG.mcmc_steps(target.like_id, state[0], k, step_size, lp=state[1], logl=state[2], step0=done, **mixed, **kw)
            if global_every:
                n_global[0] += int(res['n_accept_global'].sum().item())
            return ((res['z'], res['lp'], res['logl']), dict(x=res['hist_x'], z=res['hist_z'], logl=res['hist_logl']),
                    int(res['n_accept'].sum().item()))

        n_local = [0, 0]   # (the accepted local steps: adapting, frozen)

        def piece(k, done, state):   # (steps done .. done + k - 1, all on one side of adapt_steps; state: z, lp, logl, step)
            res = netG.mcmc_steps(target.like_id, state[0], k, step_size, lp=state[1], logl=state[2], step0=done, step_in=state[3],
                                  adapt_steps=adapt_steps, target_accept=target_accept, **mixed, **kw)
            accepted, glob = int(res['n_accept'].sum().item()), 0
            if global_every:
                glob = int(res['n_accept_global'].sum().item())
                n_global[0] += glob
            n_local[0 if done < adapt_steps else 1] += accepted - glob
            return (res['z'], res['lp'], res['logl'], res['step']), dict(x=res['hist_x'], z=res['hist_z'], logl=res['hist_logl']), accepted

        def launch_adapt(k, done, state):   # (a launch across adapt_steps runs as two: the cut does not change the run)
            k0 = adapt_steps - done if done < adapt_steps < done + k else k
            state, chunk, accepted = piece(k0, done, state)
            if k0 < k:
                state, rest, more = piece(k - k0, done + k0, state)
                chunk, accepted = dict((key, torch.cat([rows, rest[key]], dim=1)) for key, rows in chunk.items()), accepted + more
            return state, chunk, accepted

        ncall = N * (tries + S)
        hist = dict(x=samples, z=latent, logl=loglikes, derived=derived)
        if adapt_steps:
            state = self._run_in_launches(launch_adapt, (z, start['lp'], start['logl'], None), hist, S, chunk_steps, output_interval,
                                          first=1, ncall=ncall)
            A = min(adapt_steps, S)
            g = (lambda n: n // global_every) if global_every else (lambda n: 0)   # (the global steps among steps 0 .. n - 1)
            n_adapting, n_frozen = N * (A - g(A)), N * ((S - A) - (g(S) - g(A)))
            self.step_sizes = (state[3].cpu().numpy() if state[3] is not None else np.full(N, float(np.float32(step_size))))
            self.adapt_acceptance = n_local[0] / n_adapting if n_adapting else float('nan')
            self.frozen_acceptance = n_local[1] / n_frozen if n_frozen else float('nan')
            if self.single_or_primary_process:
                self.logger.info('mcmc: step adapted over [%d] steps towards acceptance [%5.4f]: step mean [%5.4f] min [%5.4f] max [%5.4f] '
                                 'adapting acceptance [%5.4f] frozen acceptance [%5.4f]' % (
                                     adapt_steps, target_accept, self.step_sizes.mean(), self.step_sizes.min(), self.step_sizes.max(),
                                     self.adapt_acceptance, self.frozen_acceptance))
        else:
            self._run_in_launches(launch, (z, start['lp'], start['logl']), hist, S, chunk_steps, output_interval, first=1, ncall=ncall)
        if global_every:   # (steps t = k - 1, 2k - 1, ... of 0 .. S - 1)
            self.global_proposed, self.global_accepted = N * (S // global_every), n_global[0]
            if self.single_or_primary_process:
                self.logger.info('mcmc: global steps every [%d] accepted [%d of %d] global acceptance [%5.4f]' % (
                    global_every, self.global_accepted, self.global_proposed, self.global_accepted / max(1, self.global_proposed)))
        if self.chain_stats and stats_interval is not None:   # sampler.py:451-452: the transformed chains up to step `it`
            self._log_chain_stats(samples, self._ensemble_affine(), S, stats_interval, prefix_offset=1, min_step=0, final=False)
        return samples, latent, derived, loglikes, step_size, ncall

    def _run_in_launches(self, launch, state, hist, S, chunk_steps, output_interval, first=0, save=True, ncall=0):
        """A run of S steps cut into launches: of `chunk_steps` steps (None: what ENSEMBLE_HISTORY_BYTES of device history hold) and at
        `output_interval`; the cut does not change the run.  launch(k, done, state) runs steps done .. done + k - 1 from `state` and
        returns (the state the next launch starts from, the chunk's history {key: [N, k, ...] tensor or array}, its accept count).
        hist: {'x', 'logl', 'derived', ...: [N, first + S, ...] numpy}, filled under the chunk's keys from column `first` on; with
        `save` the chain file is rewritten from it whenever `done` reaches a multiple of output_interval.  Books total_accepted and
        total_rejected, and `ncall` as total_calls (0 where the host protocol has counted its own)"""
        N, D = hist['x'].shape[0], self.x_dim
        if chunk_steps is None:
            chunk_steps = max(1, self.ENSEMBLE_HISTORY_BYTES // (N * (8 * D + 8)))
        chunk_steps = max(1, min(int(chunk_steps), S if S > 0 else 1))
        if output_interval:
            chunk_steps = min(chunk_steps, int(output_interval))
        n_acc, done = 0, 0
        while done < S:
            k = min(chunk_steps, S - done)
            state, chunk, accepted = launch(k, done, state)
            n_acc += accepted
            for key, rows in chunk.items():
                hist[key][:, first + done:first + done + k] = rows.cpu().numpy() if torch.is_tensor(rows) else rows
            done += k
            if save and output_interval is not None and done % int(output_interval) == 0:
                n = first + done
                self._save_samples(self.transform(hist['x'][:, :n].reshape(-1, D)), hist['logl'][:, :n].reshape(-1),
                                   derived_samples=hist['derived'][:, :n].reshape(N * n, hist['derived'].shape[2]))
        self.total_calls += ncall
        self.total_accepted += n_acc
        self.total_rejected += N * S - n_acc
        return state

    def _ensemble_sample(self, mcmc_steps, num_walkers, init_samples=None, init_loglikes=None, init_derived=None, loglstar=None,
                         show_progress=False, max_start_tries=100, output_interval=None, stats_interval=None, plot_trace=True,
                         moves=None, seed=None, chunk_steps=None, route=None):
        """emcee's EnsembleSampler with its default stretch move in latent space (sampler.py:632-724).  BUILD-DEFINED STREAM, EMCEE'S
        MOVE: include/nnest_hip.h nnest_ensemble_steps has the definition; parity with emcee is statistical.  The fused kernel runs
        where it takes the flow, the likelihood and the population (route 'fused'), the round driver otherwise (route 'rounds').
        `route` pins one; None chooses 'fused' for the NVP where it is taken and 'rounds' for every other flow -- the spline flow's
        fused kernel (nnest_spline_ensemble_steps) runs on route='fused' only, which raises ValueError where it is not taken.  The run is cut into launches of `chunk_steps` steps (default: by device memory); the cut does
        not change it.  Returns (samples [N, S, D] (x, before the transform), latent_samples [N, S, D], derived_samples [N, S, nd],
        loglikes [N, S] (the latent log target, emcee's log_prob), ncall).
        `moves`: None, or the reference's dict (sampler.py:693-707) with 'stretch' and 'de' (_lib.ens_moves: 'kde' and 'snooker' are
        not built, NotImplementedError): one move per step by weight (include/nnest_hip.h nnest_ensemble_moves_steps).  With a DE
        step in the run the NVP's fused route is taken where its population fits the kernel that knows the move; the spline flow's
        fused kernel does not know it: rounds at route=None, ValueError at route='fused'."""
        mv = _lib.ens_moves(moves)
        S = int(mcmc_steps)
        if init_samples is not None:
            num_walkers = init_samples.shape[0]
        N, D, nd = int(num_walkers), self.x_dim, self.num_derived
        if N < 2 * D:   # emcee/moves/red_blue.py
            raise RuntimeError('It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions.')
        mix = _lib.ens_moves_mix(mv, N)
        mkw = {} if mv is None else {'moves': mv}
        netG = self.trainer.netG
        if init_samples is not None:
            z, _ = netG.forward(init_samples)
        else:   # sampler.py:662-672 (its retry loop tests np.all(...) > -1e30, which always holds: one draw)
            z = netG.prior_sample(N)
        z = z.contiguous()
        lp0 = None if init_loglikes is None else torch.as_tensor(np.asarray(init_loglikes, np.float64)).to(z.device)
        seed = self._next_seed() if seed is None else int(seed)
        target, _ = self._device_target()
        # the fused kernel takes the flow (its family binds an `ensemble` entry: HipNVP, HipSpline), the likelihood and the population
        # (with a DE step in the run: an `ensemble_moves` entry, and the population of the kernel that knows the move)
        fused_ok = (target is not None and ('ensemble_moves' if mix else 'ensemble') in getattr(netG, '_sym', ())
                    and N <= (netG.ensemble_max_walkers(target.like_id, moves=mv) if mix else netG.ensemble_max_walkers(target.like_id)))
        if route is None:   # (the spline's fused kernel is opt-in, route='fused': DESIGN.md 3.7)
            route = 'fused' if fused_ok and getattr(netG, 'ensemble_fused_by_default', False) else 'rounds'
        elif route == 'fused' and not fused_ok:
            raise ValueError('ensemble: the fused route does not take this flow, likelihood, population or move')
        samples = np.empty((N, S, D), np.float32)
        latent = np.empty((N, S, D), np.float32)
        loglikes = np.empty((N, S))
        derived = np.zeros((N, S, nd))
        ncall = (0 if init_loglikes is not None else N) + N * S
        from .ensemble_rounds import ensemble_rounds
        kw = dict(loglstar=loglstar, seed=seed, **mkw)
        if target is not None:
            kw.update(target.launch_kwargs(netG.device))
        else:
            host = dict(loglike=self.loglike, prior=self.prior if self._user_prior is not None else None, num_derived=nd,
                        init_derived=init_derived)

        def launch(k, done, state):
            z, lp, rounds = state
            if route == 'fused':
                res = netG.ensemble_steps(target.like_id, z, k, lp=lp, step0=done, **kw)
                return ((res['z'], res['lp'], None), dict(z=res['hist_z'], x=res['hist_x'], logl=res['hist_lp']),
                        int(res['n_accept'].sum().item()))
            acc0 = 0 if rounds is None else int(rounds.n_accept.sum().item())
            rounds, h = ensemble_rounds(netG, z, k, state=rounds, lp=lp, step0=done, **kw,
                                        **(host if target is None else dict(like_id=target.like_id)))
            return ((z, lp, rounds), dict(z=h['hist_z'], x=h['hist_x'], logl=h['hist_lp'], derived=h['hist_derived']),
                    int(rounds.n_accept.sum().item()) - acc0)

        # (the host protocol counts its own calls in self.loglike)
        self._run_in_launches(launch, (z, lp0, None), dict(x=samples, z=latent, logl=loglikes, derived=derived), S, chunk_steps,
                              output_interval, ncall=0 if target is None else ncall)
        self.ensemble_route = route
        return samples, latent, derived, loglikes, ncall

    def _ensemble_sample_x(self, mcmc_steps, init_samples, init_loglikes=None, loglstar=None, affine=None, output_interval=None,
                           seed=None, chunk_steps=None, route=None, moves=None):
        """The stretch move in X space: `_ensemble_sample`'s run with the identity for the flow, so the walkers are x and the target
        is logL(T(x)) + prior -- the emcee run EnsembleSampler.bootstrap starts from (ensemble.py:111-147).  BUILD-DEFINED STREAM,
        EMCEE'S MOVE (include/nnest_hip.h nnest_ensemble_x_steps).  T is `affine` = (std, mean), None: the identity.  Route 'fused'
        (nnest_ensemble_x_steps) where the likelihood and the prior run on the device and the population is resident, 'rounds'
        (ensemble_rounds on an IdentityFlow) otherwise: a Python likelihood, another prior, derived parameters, a larger
        population; `route` pins one, for tests.  Cut into launches like `_ensemble_sample`.  Returns (samples [N, S, D],
        loglikes [N, S] (the log target), derived [N, S, nd], ncall).  `moves`: as `_ensemble_sample` (nnest_ensemble_x_moves_steps)."""
        from . import flow as _flow
        mv = _lib.ens_moves(moves)
        from .ensemble_rounds import IdentityFlow, ensemble_rounds
        S = int(mcmc_steps)
        init_samples = np.asarray(init_samples)
        N, D, nd = init_samples.shape[0], self.x_dim, self.num_derived
        if init_samples.shape != (N, D):
            raise ValueError('init_samples must be shaped [num_walkers, %d], got %s' % (D, init_samples.shape))
        if N < 2 * D:   # emcee/moves/red_blue.py
            raise RuntimeError('It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions.')
        _lib.ens_moves_mix(mv, N)
        mkw = {} if mv is None else {'moves': mv}
        dev = self.trainer.netG.device
        if affine is None:
            affine = (np.ones(D), np.zeros(D))
        x = _flow._as_dev_f32(init_samples, dev).contiguous()
        lp0 = None if init_loglikes is None else torch.as_tensor(np.asarray(init_loglikes, np.float64)).to(dev)
        seed = self._next_seed() if seed is None else int(seed)
        target, _ = self._device_target(affine)
        fused_ok = target is not None and D <= 128 and N <= _flow.ensemble_x_max_walkers(D, target.like_id, device=dev, **mkw)
        if route is None:
            route = 'fused' if fused_ok else 'rounds'
        elif route == 'fused' and not fused_ok:
            raise ValueError('ensemble: the fused x-space route does not take this likelihood, prior or population')
        samples = np.empty((N, S, D), np.float32)
        loglikes = np.empty((N, S))
        derived = np.zeros((N, S, nd))
        ncall = (0 if init_loglikes is not None else N) + N * S
        ident = IdentityFlow(dev)
        kw = dict(loglstar=loglstar, seed=seed, **mkw)
        if target is not None:
            kw.update(target.launch_kwargs(dev))
        else:
            host = dict(loglike=self.loglike, prior=self.prior if self._user_prior is not None else None, num_derived=nd)

        def launch(k, done, state):
            x, lp, rounds = state
            if route == 'fused':
                res = _flow.ensemble_x_steps(target.like_id, x, k, lp=lp, step0=done, device=dev, **kw)
                return (res['x'], res['lp'], None), dict(x=res['hist_x'], logl=res['hist_lp']), int(res['n_accept'].sum().item())
            acc0 = 0 if rounds is None else int(rounds.n_accept.sum().item())
            rounds, h = ensemble_rounds(ident, x, k, state=rounds, lp=lp, step0=done, **kw,
                                        **(host if target is None else dict(like_id=target.like_id)))
            return ((x, lp, rounds), dict(x=h['hist_z'], logl=h['hist_lp'], derived=h['hist_derived']),
                    int(rounds.n_accept.sum().item()) - acc0)

        # (bootstrap writes the whole run itself; the host protocol counts its own calls in self.loglike)
        self._run_in_launches(launch, (x, lp0, None), dict(x=samples, logl=loglikes, derived=derived), S, chunk_steps, output_interval,
                              save=False, ncall=0 if target is None else ncall)
        self.ensemble_route = route
        return samples, loglikes, derived, ncall

    # ---- chain statistics (sampler.py:474-492) ---------------------------------------------------------------------
    def _chain_stats(self, samples, mean=None, std=None, step=None, affine=None):
        """acceptance rate, ESS [D] and mean jump distance of chains samples [C, T, D] (numpy, or a CUDA tensor read in place), and
        the reference's log line, as Sampler._chain_stats (the Gelman-Rubin R-hat, which the reference computes and discards, is in
        nnest_amd.evaluation.chain_stats).  affine = (a, b): the statistics of samples * a + b, without a transformed copy."""
        from .evaluation import chain_stats
        r = chain_stats(samples, mean=mean, std=std, affine=affine)
        acceptance, ess, jump_distance = r['acceptance'], r['ess'], r['jump_distance']
        self._log_chain_stats_line(acceptance, ess, jump_distance, step)
        return acceptance, ess, jump_distance

    def _log_chain_stats_line(self, acceptance, ess, jump_distance, step=None):
        if step is None:
            self.logger.info('Acceptance [%5.4f] min ESS [%5.4f] max ESS [%5.4f] average jump [%5.4f]' %
                             (acceptance, np.min(ess), np.max(ess), jump_distance))
        else:
            self.logger.info('Step [%d] acceptance [%5.4f] min ESS [%5.4f] max ESS [%5.4f] average jump [%5.4f]' %
                             (step, acceptance, np.min(ess), np.max(ess), jump_distance))

    def _log_chain_stats(self, samples, affine, mcmc_steps, stats_interval, prefix_offset, min_step, final=True):
        """MCMCSampler / EnsembleSampler with chain_stats=True: the lines the reference logs while it samples (step `it` of
        stats_interval, on the transformed chains up to that step: prefix_offset + it states, sampler.py:451-452 and :712-713,
        steps > min_step), then once on the whole run (mcmc.py:119-120, ensemble.py:224-225).  One upload of the history; every
        prefix is read in place through its strides, the transform applied on load.  final=False: the interval lines alone."""
        h = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(self.trainer.netG.device)
        if stats_interval is not None:
            for it in range(int(stats_interval), int(mcmc_steps) + 1, int(stats_interval)):
                if it > min_step and prefix_offset + it >= 2:
                    self._chain_stats(h[:, :prefix_offset + it], step=it, affine=affine)
        if final and mcmc_steps > 1:
            self._chain_stats(h, affine=affine)

    # ---- chain files (sampler.py:494-527): getdist text format "weight -logL params..." ------------------------
    def _save_samples(self, samples, loglikes, weights=None, derived_samples=None, min_weight=1e-30, outfile='chain'):
        if self.logs is None:
            return
        if weights is None:
            weights = np.ones_like(loglikes)
        cols = [np.maximum(weights, min_weight)[:, None], -np.asarray(loglikes)[:, None], samples]
        if derived_samples is not None:
            cols.append(derived_samples)
        header = ''
        if self.param_names is not None:
            header = 'weight minusloglike ' + ' '.join(self.param_names)
        write_rows_e5(os.path.join(self.logs['chains'], outfile + '.txt'), np.concatenate(cols, axis=1), header=header)

    # ---- collectives -------------------------------------------------------------------------------------------------
    # One process per GPU, torch.distributed ('nccl' = RCCL over xGMI; 'gloo' on CPU for the tests).  A tensor argument stays
    # a tensor on the communication device (no host round trip under RCCL); a numpy argument comes back as numpy.
    def _comm_device(self):
        if torch.distributed.get_backend() == 'nccl':
            return torch.device('cuda', torch.cuda.current_device())
        return torch.device('cpu')

    def _all_gather_rows(self, arr):
        """concatenate equally-shaped per-rank arrays along axis 0 on every rank (C2)"""
        if not self.use_mpi:
            return arr
        as_numpy = not torch.is_tensor(arr)
        t = (torch.as_tensor(np.ascontiguousarray(arr)) if as_numpy else arr).to(self._comm_device()).contiguous()
        out = torch.empty((self.mpi_size * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        torch.distributed.all_gather_into_tensor(out, t)
        return out.cpu().numpy() if as_numpy else out

    def _broadcast(self, arr, src=0):
        if not self.use_mpi:
            return arr
        as_numpy = not torch.is_tensor(arr)
        t = (torch.as_tensor(np.ascontiguousarray(arr)) if as_numpy else arr).to(self._comm_device()).contiguous()
        torch.distributed.broadcast(t, src=src)
        return t.cpu().numpy() if as_numpy else t

    def _all_reduce_(self, t):
        """sum a tensor over the ranks in place (on the communication device, copied back)"""
        if self.use_mpi:
            c = t.to(self._comm_device())
            torch.distributed.all_reduce(c)
            t.copy_(c)
        return t

    def _all_sum(self, value):
        if not self.use_mpi:
            return value
        t = torch.tensor([float(value)], dtype=torch.float64, device=self._comm_device())
        torch.distributed.all_reduce(t)
        return float(t.item())
