"""HipNVP: the RealNVP coupling stack resident on one MI355X, driven through the C ABI.

Mirrors SingleSpeedNVP / NormalizingFlowModel (reference nnest/networks.py:17-84, :328-347):
forward, inverse, log_probs, sample -- all on torch CUDA (ROCm) float32 tensors, computed by the HIP
kernels in libnnest_hip.so.  No PyTorch arithmetic is used for the flow itself.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib


_STAGING = {}


def _staging_f32(n, device):
    """a pinned float32 staging buffer per (device, stream), grown on demand: callers on different streams (threads) never
    share one"""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _STAGING.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(int(n), 1 << 16), dtype=torch.float32).pin_memory()
        _STAGING[key] = buf
    return buf[:n]


def _as_dev_f32(x, device):
    """host array -> float32 device tensor [rows, D].  Host arrays are cast on the host (the same rounding as the device
    cast) with numpy and go through one pinned staging buffer; torch's own host-side cast/copy goes through its CPU thread
    pool, which on a many-core host measured 3-6 ms per call inside a run (tools/run_timing.py) against 0.1 ms here."""
    device = torch.device(device)
    if torch.is_tensor(x) and x.device.type == 'cpu' and device.type == 'cuda':
        x = x.detach().numpy()
    if not torch.is_tensor(x) and device.type == 'cuda':
        a = np.asarray(x)
        if a.ndim == 1:
            a = a[None, :]
        out = torch.empty(a.shape, dtype=torch.float32, device=device)
        if a.size:
            stage = _staging_f32(a.size, device)
            # cast and copy in ONE pass, straight into the pinned buffer (numpy, not Tensor.copy_: torch's CPU copy wakes its whole
            # thread pool -- 5.7 ms per call on a 256-core host, tools/run_timing.py)
            np.copyto(stage.numpy().reshape(a.shape), a, casting='unsafe')
            out.view(-1).copy_(stage, non_blocking=True)
            torch.cuda.current_stream(device).synchronize()  # the staging buffer is free for the next call
        return out
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    x = x.to(device=device, dtype=torch.float32)
    if x.dim() == 1:
        x = x[None, :]
    return x.contiguous()


def target_vectors(who, device, t_std, t_mean, lo, hi, D=None, identity=False):
    """a device target's per-dimension vectors as the C entries take them: (t_std, t_mean, lo, hi), each a float32 [D] tensor on
    `device` or None.  Each comes as an array (cast on the host, staged), as None, or as a float32 tensor already on the device, which
    passes through untouched (DeviceTarget.launch_kwargs stages a run's once).  t_std and t_mean: both or neither, and so lo and hi;
    identity=True fills a missing T with (1, 0), for the entries that require one"""
    if (t_std is None) != (t_mean is None):
        raise ValueError('%s: t_std and t_mean: both or neither' % who)
    if (lo is None) != (hi is None):
        raise ValueError('%s: lo and hi: both or neither' % who)
    device = torch.device(device)

    def vec(v, fill):
        if v is None:
            return torch.full((D,), fill, dtype=torch.float32, device=device) if identity and fill is not None else None
        if torch.is_tensor(v) and v.dtype == torch.float32 and v.device == device and v.is_contiguous():
            return v
        if not torch.is_tensor(v):
            v = np.array(v, np.float32)   # (cast on the host; a copy, so a read-only array stages too)
        return _as_dev_f32(v.reshape(1, -1 if D is None else D), device).reshape(-1)
    return vec(t_std, 1.0), vec(t_mean, 0.0), vec(lo, None), vec(hi, None)


SCALE_MODES = {'': 0, 'translate': 1, 'constant': 2}
TRAIN_KERNEL_MAX_BATCH = 128   # row slots of the one-launch training kernels (nnest_train.hip TRAIN_MAX_ROWS; nnest_spline_train.hip)


class _HipFlow(object):
    """What the flow families share: the pass, proposal, gradient and optimiser entry points differ only in the C symbol
    (`self._sym[...]`, filled in by the subclass through `_bind`) -- same tensors in, same tensors out."""

    base_beta = 0.0   # 0: N(0, I); > 0: GeneralisedNormal(0, 1, beta)
    base_dist = None  # the distribution object handed to Trainer(base_dist=...), if any

    _IMPORTANCE_TILE = 4   # samples per workgroup and pass of the family's `importance` kernel (nnest_importance_groups)
    _FAMILY_ENTRIES = ('forward', 'inverse', 'log_probs', 'inverse_loglike', 'set_base', 'loss_grad', 'vjp', 'adam_step', 'destroy')

    def _bind(self, family, **named):
        """self._sym: the entry points `<family>_<name>` that the library declares for this family (nnest_chol has neither
        inverse_loglike nor vjp: those names stay out), and the ones whose symbol does not follow the pattern, by name
        (mh='nnest_mh_constrained_steps', slice='nnest_slice_steps', ensemble='nnest_ensemble_steps'); a name left out is an entry point the family does not have"""
        family_syms = [(n, '%s_%s' % (family, n)) for n in self._FAMILY_ENTRIES]
        self._sym = {n: getattr(self._lib, sym) for n, sym in family_syms if sym in _lib.SIGNATURES}
        self._sym.update((n, getattr(self._lib, sym)) for n, sym in named.items())

    def __del__(self):
        try:
            if getattr(self, '_h', None) is not None and self._h.value:
                self._sym['destroy'](self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    def set_base(self, base_dist):
        """NormalizingFlowModel(prior=...) (networks.py:47-59): None / MultivariateNormal(0, I) or GeneralisedNormal(0, 1, beta)"""
        beta = 0.0
        if base_dist is not None and hasattr(base_dist, 'beta'):
            loc = torch.as_tensor(base_dist.loc, dtype=torch.float32).detach().cpu()
            scale = torch.as_tensor(base_dist.scale, dtype=torch.float32).detach().cpu()
            if not (bool(torch.all(loc == 0)) and bool(torch.all(scale == 1))):
                raise NotImplementedError('GeneralisedNormal base: only loc = 0, scale = 1 (what the reference constructs)')
            beta = float(base_dist.beta.item()) if torch.is_tensor(base_dist.beta) else float(base_dist.beta)
            if not beta > 0:
                raise ValueError('beta must be > 0')
            self.base_dist = base_dist
        with torch.cuda.device(self.device):
            _lib.check(self._sym['set_base'](self._h, ctypes.c_float(beta)))
        self.base_beta = beta

    def prior_sample(self, num_samples):
        """self.prior.sample((n,)) (networks.py:80): N(0, I) draws, or scipy gennorm draws for the generalised normal"""
        if self.base_dist is not None:
            return _as_dev_f32(self.base_dist.sample((int(num_samples),)).reshape(int(num_samples), self.D), self.device)
        return torch.randn(int(num_samples), self.D, device=self.device)

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def parameters(self):
        return list(self.state_dict().values())

    def _pass(self, fn, x, want_logdet=True):
        x = _as_dev_f32(x, self.device)
        N = x.shape[0]
        if x.shape[1] != self.D:
            raise ValueError('expected [N, %d], got %s' % (self.D, tuple(x.shape)))
        out = torch.empty_like(x)
        ld = torch.empty(N, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(fn(self._h, _lib.ptr(x), _lib.ptr(out), _lib.ptr(ld), N, _lib.current_stream(self.device)))
        return out, ld

    def forward(self, x):
        """NormalizingFlow.forward (networks.py:24-32): (z, log_det)"""
        return self._pass(self._sym['forward'], x)

    def inverse(self, z):
        """NormalizingFlow.inverse (networks.py:34-42): (x, log_det)"""
        return self._pass(self._sym['inverse'], z)

    def log_probs(self, x):
        """NormalizingFlowModel.log_probs (networks.py:71-76)"""
        x = _as_dev_f32(x, self.device)
        out = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._sym['log_probs'](self._h, _lib.ptr(x), _lib.ptr(out), x.shape[0],
                                              _lib.current_stream(self.device)))
        return out

    def sample(self, num_samples=None, noise=None):
        """NormalizingFlowModel.sample (networks.py:78-84)"""
        if noise is None:
            noise = self.prior_sample(num_samples)
        x, _ = self.inverse(noise)
        return x

    def inverse_loglike(self, like_id, like_scale, z, want_x=True, like_params=None):
        """K3: x = f^-1(z), logdet, box-prior flag, logl = loglike(like_scale * x) in one launch."""
        z = _as_dev_f32(z, self.device)
        N = z.shape[0]
        x = torch.empty_like(z) if want_x else None
        ld = torch.empty(N, dtype=torch.float32, device=self.device)
        logl = torch.empty(N, dtype=torch.float64, device=self.device)
        inbox = torch.empty(N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            lk = _lib.like_spec(like_id, like_scale, like_params)
            _lib.check(self._sym['inverse_loglike'](self._h, ctypes.byref(lk), _lib.ptr(z),
                                                    _lib.ptr(x), _lib.ptr(ld), _lib.ptr(logl), _lib.ptr(inbox), N,
                                                    _lib.current_stream(self.device)))
        return x, ld, logl, inbox

    # ---- gradient, chain-rule stage and optimiser step: one argument list in every family (_lib.SIGNATURES).  The library's vectors
    # are the native ones (`_native_params` long; _PaddedVectors reorders, HipCholesky's are the packed ones as they are).
    def loss_grad(self, x):
        """loss = -mean(log_probs(x)) and dloss/dw (packed order) for one minibatch (loss.backward(), trainer.py:394-400), no weight
        update.  The NVP's takes <= 128 rows."""
        x = _as_dev_f32(x, self.device)
        grad = torch.empty(self._native_params, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._sym['loss_grad'](self._h, _lib.ptr(x), x.shape[0], _lib.ptr(grad), _lib.ptr(loss),
                                              _lib.current_stream(self.device)))
        return loss, self._from_native_dev(grad)

    def vjp(self, x, gz, gld):
        """the flow as one stage of a composite model (nnest_{nvp,spline}_vjp): upstream gradient gz [M,D] and dL/d(logdet) in,
        dL/dw (packed order) and dL/dx out"""
        fn = self._sym.get('vjp')
        if fn is None:   # (a family without one: the handle must not reach another family's)
            raise NotImplementedError('%s has no vjp entry point' % type(self).__name__)
        M = x.shape[0]
        grad = torch.empty(self._native_params, dtype=torch.float32, device=self.device)
        gx = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _lib.check(fn(self._h, _lib.ptr(x), _lib.ptr(gz.contiguous()), ctypes.c_float(gld), M, _lib.ptr(grad), _lib.ptr(gx),
                          _lib.current_stream(self.device)))
        return self._from_native_dev(grad), gx

    def adam_step(self, grad, lr, weight_decay):
        """one torch.optim.Adam step (coupled weight decay, trainer.py:121-122) from a gradient in packed order"""
        grad = self._to_native_dev(grad)
        with torch.cuda.device(self.device):
            _lib.check(self._sym['adam_step'](self._h, _lib.ptr(grad), ctypes.c_float(lr), ctypes.c_float(weight_decay),
                                              _lib.current_stream(self.device)))

    def mh_steps(self, like_id, like_scale, z, logl, loglstar, step_size, steps, dynamic=False, noise=None, seed=0,
                 walker_offset=0, history=False, like_params=None, lag=None, form=None, warm=None, like_glm=None, t_std=None,
                 t_mean=None):
        """K4: `steps` constrained Metropolis steps for all walkers in one launch (Sampler._mcmc_sample,
        sampler.py:229-463).  z [C,D] float32 and logl [C] float64 are updated in place.
        noise = (dz [steps,C,D], u [steps,C]) replays recorded draws; None = in-kernel Philox.
        loglstar None / NaN = the unconstrained branch (sampler.py:371-410): likelihood and box prior in the ratio.
        dynamic: False | True or 'batch' (sampler.py:422-431 over all C walkers; `lag` steps between a step and the
        scale that reflects its count, 0 = the reference exactly) | 'group' (per 16 walkers, shard-invariant).
        warm: with a lagged batch rule, the first `warm` steps apply it exactly (NNEST_MH_WARM); None = default_warm().
        form: None (by population) | 'solo' | 'quad' | 'team' | 'reg' | 'image' (include/nnest_hip.h NNEST_MH_FORM_*).
        like_glm: None -- the entry above, as it was; the descriptor of a regression likelihood of user data
        (likelihoods.GLMData.hip_like_glm, as `slice_steps` takes it) -- `like_id` must then be None (ValueError otherwise;
        like_scale and like_params are not read) and the launch goes through the family's `mh_glm` entry (nnest_mh_glm_steps,
        nnest_spline_mh_glm_steps): the same step with logL(x) = GLM(T(x)), T(x) = x * t_std + t_mean per dimension (t_std / t_mean
        [D], both or neither; None: the identity), the box on x, Philox draws per (seed, walker, step).  That entry has the hard
        constraint only (a loglstar), one form and no warm-up steps; dynamic 'group' is the spline flow's alone.  The result is
        the same dict.  `mh_glm_refusal` says beforehand whether shape, population and rule are taken."""
        if like_glm is not None:
            return self._mh_glm_steps(like_id, like_glm, t_std, t_mean, z, logl, loglstar, step_size, steps, dynamic, noise, seed,
                                      walker_offset, history, lag, form, warm)
        if t_std is not None or t_mean is not None:
            raise ValueError('mh_steps: t_std and t_mean go only with a like_glm (the analytic likelihoods take like_scale)')
        free = loglstar is None or loglstar != loglstar
        loglstar = 0.0 if free else loglstar
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()
        assert logl.is_cuda and logl.dtype == torch.float64 and logl.is_contiguous()
        C = z.shape[0]
        dev = self.device
        x = torch.empty_like(z)
        n_acc = torch.empty(C, dtype=torch.int32, device=dev)    # (every form writes both counters of every walker: no fill launches
        n_call = torch.empty(C, dtype=torch.int32, device=dev)   # in front of the kernel)
        ngroups = (C + 15) // 16
        scale_out = torch.empty(max(ngroups, 1), dtype=torch.float32, device=dev)
        hx = torch.empty(C, steps + 1, self.D, dtype=torch.float32, device=dev) if history else None
        hl = torch.empty(C, steps + 1, dtype=torch.float64, device=dev) if history else None
        dz = u = None
        if noise is not None:
            dz = _as_dev_f32(noise[0].reshape(-1, self.D), dev)
            u = noise[1].to(device=dev, dtype=torch.float32).contiguous()
            assert dz.shape[0] == steps * C and u.numel() == steps * C
        if lag is None and dynamic in (True, 'batch'):
            lag = self.default_lag(C, form)
        if warm is None:
            warm = self.default_warm(C, dynamic, lag, form)
        flags = _lib.mh_flags(dynamic, free, lag, form, warm)
        sync = None
        if flags & _lib.MH_DYNAMIC_BATCH:   # per-step batch counters, zero at every launch; last word = error flag
            # a double buffer per step count, zeroed ONCE: each launch zeroes the half the next launch will use (in-kernel where the
            # solo form runs: the fill launch in front of every K4 launch -- 3 % of a config-2 launch -- is gone)
            W = int(self._lib.nnest_mh_sync_words(int(steps)))
            pool = self.__dict__.setdefault('_sync_pool', {})
            ent = pool.get(int(steps))
            if ent is None:
                ent = pool[int(steps)] = [torch.zeros(2 * W, dtype=torch.int64, device=dev), 0]
            half = ent[1]
            sync = ent[0][half * W:(half + 1) * W]
            flags |= _lib.MH_SYNC_ZERO_PREV if half else _lib.MH_SYNC_ZERO_NEXT
        with torch.cuda.device(dev):
            lk = _lib.like_spec(like_id, like_scale, like_params)
            try:
                _lib.check(self._sym['mh'](
                    self._h, ctypes.byref(lk), _lib.ptr(z), _lib.ptr(x), _lib.ptr(logl), float(loglstar),
                    float(step_size), int(steps), C, flags, _lib.ptr(dz), _lib.ptr(u),
                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), _lib.ptr(hx), _lib.ptr(hl), _lib.ptr(n_acc),
                    _lib.ptr(n_call), _lib.ptr(scale_out), _lib.ptr(sync), _lib.current_stream(dev)))
            except Exception:
                # a refused launch ran nothing: the half it was given may or may not be the one the last launch zeroed for it,
                # and the other half was not zeroed for the launch after -- start the pair over from fresh zeros
                if sync is not None:
                    self._sync_pool.pop(int(steps), None)
                raise
        if sync is not None:
            ent[1] ^= 1   # the halves change roles only behind a launch that ran (it zeroed the other one)
        # the kernels report in the count's bit 30 whether EVERY coordinate of the chain's last x differs from its first
        # (include/nnest_hip.h NNEST_MH_ALL_MOVED): the reference's usable-chain test, nested.py:432
        # (split on first use: two element-wise launches that a caller who reads neither does not pay for)
        return _MhResult(x=x, n_accept_word=n_acc, n_call=n_call, scale=scale_out, hist_x=hx, hist_logl=hl, sync=sync)

    @staticmethod
    def _mh_glm_flags(dynamic, lag):
        """the flags word of the `mh_glm` entries: 0, the batch rule with its lag (None: MH_DEFAULT_LAG), or the per-tile rule"""
        return _lib.mh_flags(dynamic, False, lag, None, 0)

    def _mh_glm_steps(self, like_id, like_glm, t_std, t_mean, z, logl, loglstar, step_size, steps, dynamic, noise, seed, walker_offset,
                      history, lag, form, warm):
        """`mh_steps` with a like_glm: the family's `mh_glm` entry"""
        if like_id is not None:
            raise ValueError('mh_steps: like_glm goes with like_id=None, got like_id=%r' % (like_id,))
        if loglstar is None or loglstar != loglstar:
            raise ValueError('mh_steps: a like_glm runs under the hard constraint only (the unconstrained walk is mcmc_steps)')
        if form is not None or warm:
            raise ValueError('mh_steps: form=%r warm=%r: %s has one Metropolis kernel form on a regression likelihood of user data, '
                             'without warm-up steps' % (form, warm, type(self).__name__))
        fn = self._sym.get('mh_glm')
        if fn is None:
            raise NotImplementedError('no fused Metropolis kernel for %s on a regression likelihood of user data' % type(self).__name__)
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()
        assert logl.is_cuda and logl.dtype == torch.float64 and logl.is_contiguous()
        C, dev, steps = z.shape[0], self.device, int(steps)
        x = torch.empty_like(z)
        n_acc = torch.empty(C, dtype=torch.int32, device=dev)
        n_call = torch.empty(C, dtype=torch.int32, device=dev)
        scale_out = torch.empty(max((C + self.MH_GLM_WALKERS_PER_WORKGROUP - 1) // self.MH_GLM_WALKERS_PER_WORKGROUP, 1),
                                dtype=torch.float32, device=dev)
        hx = torch.empty(C, steps + 1, self.D, dtype=torch.float32, device=dev) if history else None
        hl = torch.empty(C, steps + 1, dtype=torch.float64, device=dev) if history else None
        dz = u = None
        if noise is not None:
            dz = _as_dev_f32(noise[0].reshape(-1, self.D), dev)
            u = noise[1].to(device=dev, dtype=torch.float32).contiguous()
            assert dz.shape[0] == steps * C and u.numel() == steps * C
        flags = self._mh_glm_flags(dynamic, lag)
        sync = None
        if flags & _lib.MH_DYNAMIC_BATCH:   # per-step batch counters, zero at the launch; last word = error flag
            sync = torch.zeros(int(self._lib.nnest_mh_sync_words(steps)), dtype=torch.int64, device=dev)
        t_std, t_mean, _, _ = target_vectors('mh_steps', dev, t_std, t_mean, None, None, D=self.D)
        with torch.cuda.device(dev):
            lk, keep = glm_spec(like_glm, dev)   # (`keep`: the staged arrays, alive until the call has been enqueued)
            _lib.check(fn(self._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(z), _lib.ptr(x), _lib.ptr(logl),
                          float(loglstar), float(step_size), steps, C, flags, _lib.ptr(dz), _lib.ptr(u), int(seed) & 0xFFFFFFFFFFFFFFFF,
                          int(walker_offset), _lib.ptr(hx), _lib.ptr(hl), _lib.ptr(n_acc), _lib.ptr(n_call), _lib.ptr(scale_out),
                          _lib.ptr(sync), _lib.current_stream(dev)))
        return _MhResult(x=x, n_accept_word=n_acc, n_call=n_call, scale=scale_out, hist_x=hx, hist_logl=hl, sync=sync)

    MH_GLM_WALKERS_PER_WORKGROUP = 4   # (scale_out_dev of the `mh_glm` entry: one float per workgroup)

    def mh_glm_refusal(self, D=None, C=0, dynamic=False, lag=None):
        """why `mh_steps` with a like_glm of dimension D (None: the flow's own) would refuse this flow (its shape), C walkers or this
        step rule (the batch rule on a grid that is not proven resident) -- the library's own words (the family's `mh_glm_check`
        entry; nothing is launched) --, or None where it is taken.  NotImplementedError for a family without such a kernel"""
        fn = self._sym.get('mh_glm_check')
        if fn is None or 'mh_glm' not in self._sym:
            raise NotImplementedError('no fused Metropolis kernel for %s on a regression likelihood of user data' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, self.D if D is None else int(D), int(C), self._mh_glm_flags(dynamic, lag))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def slice_steps(self, like_id, like_scale, z, logl, loglstar, width, steps, max_stepout=8, max_shrink=32, noise=None, seed=0,
                    walker_offset=0, history=False, like_params=None, form=None, like_glm=None, t_std=None, t_mean=None):
        """SLICE proposal in latent space (the family's `slice` entry point: nnest_slice_steps, nnest_spline_slice_steps; BUILD-DEFINED:
        the reference has none, nnest/sampler.py:310-316 is random-walk Metropolis): `steps` slice-sampling updates (stepping out +
        shrinkage along a random direction) of every walker under the hard constraint logL > loglstar, the target the reference's
        Metropolis step leaves invariant.  z [C,D] float32 and logl [C] float64 are updated in place.  noise = dz [steps,C,D] replays
        recorded directions (fill_slice_noise exports the in-kernel ones).  form: the kernel form, where the family has several
        (HipSpline: None = by population | 'wave' | 'team' | 'pair').  Returns x, n_call (candidates whose likelihood decided),
        n_move, moved (nested.py:432), n_eval (flow evaluations), hist_x.  A family without a fused slice kernel raises
        NotImplementedError (its handle must not reach another family's): the slice proposal runs it through nnest_amd.slice_rounds.
        like_glm: None -- the entries above, as they were; the descriptor of a regression likelihood of user data
        (likelihoods.GLMData.hip_like_glm, as `mcmc_steps` takes it) -- `like_id` must then be None (ValueError otherwise; like_scale
        and like_params are not read) and the launch goes through the family's `slice_glm` entry (nnest_slice_glm_steps,
        nnest_spline_slice_glm_steps): the same update with logL(x) = GLM(T(x)), T(x) = x * t_std + t_mean per dimension (t_std /
        t_mean [D], both or neither; None: the identity).  The box stays on x.  The spline's `slice_glm` kernel has the team form only:
        form None or 'team' (ValueError otherwise).  `slice_glm_refusal` says beforehand whether the flow's shape is taken."""
        glm = like_glm is not None
        if glm and like_id is not None:
            raise ValueError('slice_steps: like_glm goes with like_id=None, got like_id=%r' % (like_id,))
        if not glm and (t_std is not None or t_mean is not None):
            raise ValueError('slice_steps: t_std and t_mean go only with a like_glm (the analytic likelihoods take like_scale)')
        fn = self._sym.get('slice_glm' if glm else 'slice')
        if fn is None:
            raise NotImplementedError('no fused slice kernel for %s%s: use nnest_amd.slice_rounds' % (
                type(self).__name__, ' on a regression likelihood of user data' if glm else ''))
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()
        assert logl.is_cuda and logl.dtype == torch.float64 and logl.is_contiguous()
        form_args = self._slice_glm_form_args(form) if glm else self._slice_form_args(form)
        C, dev = z.shape[0], self.device
        x = torch.empty_like(z)
        n_call = torch.empty(C, dtype=torch.int32, device=dev)
        n_move = torch.empty(C, dtype=torch.int32, device=dev)
        n_eval = torch.empty(C, dtype=torch.int32, device=dev)
        hx = torch.empty(C, steps + 1, self.D, dtype=torch.float32, device=dev) if history else None
        dz = None
        if noise is not None:
            dz = _as_dev_f32(noise.reshape(-1, self.D), dev)
            assert dz.shape[0] == steps * C
        t_args = ()
        if glm:
            t_std, t_mean, _, _ = target_vectors('slice_steps', dev, t_std, t_mean, None, None, D=self.D)
            t_args = (_lib.ptr(t_std), _lib.ptr(t_mean))
        with torch.cuda.device(dev):
            if glm:
                lk, keep = glm_spec(like_glm, dev)   # (`keep`: the staged arrays, alive until the call has been enqueued)
            else:
                lk = _lib.like_spec(like_id, like_scale, like_params)
            _lib.check(fn(self._h, ctypes.byref(lk), *t_args, _lib.ptr(z), _lib.ptr(x), _lib.ptr(logl), float(loglstar), float(width),
                          int(steps), C, int(max_stepout), int(max_shrink), *form_args, _lib.ptr(dz), int(seed) & 0xFFFFFFFFFFFFFFFF,
                          int(walker_offset), _lib.ptr(hx), _lib.ptr(n_call), _lib.ptr(n_move), _lib.ptr(n_eval), _lib.current_stream(dev)))
        n_move, moved = split_move_word(n_move)
        return dict(x=x, n_call=n_call, n_move=n_move, moved=moved, n_eval=n_eval, hist_x=hx)

    def slice_glm_refusal(self, D=None):
        """why `slice_steps` with a like_glm of dimension D (None: the flow's own) would refuse this flow (its shape) -- the library's
        own words (the family's `slice_glm_check` entry; nothing is launched) --, or None where it is taken.  NotImplementedError
        for a family without such a kernel"""
        fn = self._sym.get('slice_glm_check')
        if fn is None or 'slice_glm' not in self._sym:
            raise NotImplementedError('no fused slice kernel for %s on a regression likelihood of user data' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, self.D if D is None else int(D))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def _slice_glm_form_args(self, form):
        """`_slice_form_args` for the family's `slice_glm` entry point: nothing, and one form"""
        if form is not None:
            raise ValueError('form=%r: %s has one slice kernel form on a regression likelihood of user data' % (form, type(self).__name__))
        return ()

    def _slice_form_args(self, form):
        """what the family's slice entry point takes between max_shrink and noise_dz_dev: nothing, for a kernel with one form"""
        if form is not None:
            raise ValueError('form=%r: %s has one slice kernel form' % (form, type(self).__name__))
        return ()

    def supports_fused_slice(self, C):
        """whether `slice_steps` (a fused slice kernel) takes this flow for C walkers; where it does not, the slice proposal runs
        through nnest_amd.slice_rounds (any flow)"""
        return 'slice' in self._sym

    def fill_slice_noise(self, steps, C, seed=0, walker_offset=0):
        """the directions nnest_slice_steps draws (Philox normals), exported for the checker: dz [steps, C, D]"""
        dz = torch.empty(steps, C, self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_slice_fill_noise(_lib.ptr(dz), steps, C, self.D, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                        int(walker_offset), _lib.current_stream(self.device)))
        return dz

    # whether Sampler._ensemble_sample takes the fused ensemble route for this family when the caller names none (route=None).  The
    # spline's fused kernel is opt-in (route='fused'): DESIGN.md 3.7
    ensemble_fused_by_default = False

    def ensemble_max_walkers(self, like_id, moves=None):
        """the population the family's fused ensemble entry (nnest_ensemble_steps, nnest_spline_ensemble_steps) takes for this flow and
        likelihood (every workgroup resident); 0 if its shape is not the fused route's, or the family has no such entry.  moves
        (_lib.ens_moves): with a DE step in the run, the population of the entry that knows the move (nnest_ensemble_moves_steps:
        another kernel instantiation); 0 for a family without one"""
        mv = _lib.ens_moves(moves)
        mix = _lib.ens_moves_mix(mv)
        fn = self._sym.get('ensemble_moves_max_walkers' if mix else 'ensemble_max_walkers')
        if fn is None:
            return 0
        with torch.cuda.device(self.device):
            return max(0, int(fn(self._h, int(like_id), _lib.moves_ref(mv)) if mix else fn(self._h, int(like_id))))

    def ensemble_steps(self, like_id, z, steps, t_std=None, t_mean=None, lo=None, hi=None, lp=None, loglstar=None, seed=0, step0=0,
                       like_params=None, moves=None):
        """`steps` steps of emcee's stretch move in latent space, in ONE launch (the family's `ensemble` entry point:
        nnest_ensemble_steps, nnest_spline_ensemble_steps; build-defined stream, emcee's move: include/nnest_hip.h has the definition).  z [C, D] float32 on the device: the walkers' start (read only); lp [C]
        float64 or None (evaluated); the likelihood `like_id` sees T(x) = x * t_std + t_mean (per dimension; None: identity); lo / hi
        [D]: the prior box on T(x) (None: no prior); loglstar: None = logL + log|det| + prior, else the hard constraint.  step0: the
        global index of the first step (the draws depend on it, so a run cut into launches is the same run).  Returns z, x, lp (the
        last state), hist_z, hist_x [C, steps, D], hist_lp [C, steps] and n_accept [C].  Raises NnestHipError (code
        NNEST_E_UNSUPPORTED) when C exceeds ensemble_max_walkers, NotImplementedError for a family without a fused ensemble kernel
        (its handle must not reach another family's): nnest_amd.ensemble_rounds runs those.  moves: None (the stretch move alone, the
        family's `ensemble` entry), or {'stretch': w, 'de': w} (_lib.ens_moves): a mixture with emcee's DE move, one move per step by
        weight, through the family's `ensemble_moves` entry (nnest_ensemble_moves_steps; with a DE step in the run
        NotImplementedError for a family without one: the spline flow)."""
        mv = _lib.ens_moves(moves, 'ensemble_steps')
        mix = _lib.ens_moves_mix(mv)
        fn = None if mv is None else self._sym.get('ensemble_moves')
        if fn is None and not mix:   # (weights on the stretch move alone are that run: the family's `ensemble` entry takes it)
            fn, mv = self._sym.get('ensemble'), None
        if fn is None:
            raise NotImplementedError('no fused ensemble kernel for %s%s: use nnest_amd.ensemble_rounds' % (
                type(self).__name__, ' with a move other than the stretch move' if mix else ''))
        dev = self.device
        z = _as_dev_f32(z, dev).contiguous()
        C, D, steps = z.shape[0], self.D, int(steps)
        _lib.ens_moves_mix(mv, C, 'ensemble_steps')
        f32 = dict(dtype=torch.float32, device=dev)
        t_std, t_mean, lo_t, hi_t = target_vectors('ensemble_steps', dev, t_std, t_mean, lo, hi, D=D, identity=True)
        if lp is not None:
            lp = torch.as_tensor(lp, dtype=torch.float64).to(dev).contiguous()
        out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, dtype=torch.float64, device=dev),
                   hist_z=torch.empty(C, steps, D, **f32), hist_x=torch.empty(C, steps, D, **f32),
                   hist_lp=torch.empty(C, steps, dtype=torch.float64, device=dev), n_accept=torch.empty(C, dtype=torch.int32, device=dev))
        words = self._lib.nnest_ensemble_work_words(C, steps)
        if words < 0:
            raise ValueError('ensemble_steps: %d walkers x %d steps: the work buffer is too large; launch fewer steps' % (C, steps))
        work = torch.empty(words, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            lk = _lib.like_spec(like_id, 1.0, like_params)
            _lib.check(fn(
                self._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo_t), _lib.ptr(hi_t), _lib.ptr(z), _lib.ptr(lp),
                _lib.ptr(out['z']), _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['hist_z']), _lib.ptr(out['hist_x']),
                _lib.ptr(out['hist_lp']), _lib.ptr(out['n_accept']), _lib.ptr(work), C, steps, int(step0) & 0xFFFFFFFFFFFFFFFF,
                int(seed) & 0xFFFFFFFFFFFFFFFF, 0 if loglstar is None else 1, 0.0 if loglstar is None else float(loglstar),
                _lib.current_stream(dev), *(() if mv is None else (_lib.moves_ref(mv),))))
        return out

    def mcmc_steps(self, like_id, z, steps, step_size, t_std=None, t_mean=None, lo=None, hi=None, lp=None, logl=None, seed=0, step0=0,
                   walker_offset=0, like_params=None, history=True, beta=None, global_every=0, step_in=None, adapt_steps=0, adapt_rate=1.0,
                   target_accept=0.234, like_data=None, like_glm=None, prior_gauss=None):
        """`steps` steps of random-walk Metropolis in latent space with the likelihood, the prior and the Jacobian in the ratio, in ONE
        launch (the family's `mcmc` entry point: nnest_mcmc_steps, nnest_spline_mcmc_steps; build-defined stream, the reference's move:
        include/nnest_hip.h has the definition).  z [C, D] float32 on the device: the walkers' start; lp, logl [C] float64: the
        start's target and likelihood as a previous launch returned them, or both None (evaluated); the likelihood `like_id` sees
        T(x) = x * t_std + t_mean (per dimension; None: identity); lo / hi [D]: the prior box on T(x) (None: no prior).  step0: the
        global index of the first step, walker_offset: the global index of walker 0 -- the draws depend on (seed, walker, step)
        only, so a run cut into launches or into shards is the same run.  steps = 0 evaluates the start (x, lp, logl; z is the
        caller's).  Returns z, x, lp, logl (the last state), hist_z, hist_x [C, steps, D], hist_logl [C, steps] (the state after
        every step; None with history=False or steps = 0) and n_accept [C].  Asynchronous on the current stream.
        beta: None -- the entry above, as it was; a float -- the TEMPERED target lp_beta = ((beta * logL) + log|det|) + prior through
        the family's `mcmc_tempered` entry (nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps: the same draws, the same
        invariances; lp is lp_beta, logl stays the untempered logL; beta finite and >= 0, 1.0 is the untempered run bit for bit).
        global_every: 0 -- the entries above, as they were; k > 0 -- the MIXED walk through the family's `mcmc_mixed` entry
        (nnest_mcmc_mixed_steps, nnest_spline_mcmc_mixed_steps): step t is a flow-independence ("global") step where (t + 1) % k == 0
        -- the proposal is the draw eps itself, accepted on the ratio of importance weights lp - logb under the N(0, I) base --, a
        random-walk step otherwise; the same draws and invariances; beta None is 1.0.  The result then also carries n_accept_global
        [C] (n_accept counts both kinds).  ValueError for global_every < 0.
        step_in, adapt_steps, adapt_rate, target_accept: adapt_steps == 0 and step_in None -- the entries above, as they were;
        otherwise the ADAPTIVE walk through the family's `mcmc_adapt` entry (nnest_mcmc_adapt_steps, nnest_spline_mcmc_adapt_steps):
        the mixed walk (global_every 0 included, beta None is 1.0) in which every walker proposes its local steps at its own float64
        step -- step_in [C] float64 (clamped to [1e-8, 1e2]), or `step_size` for all -- and, after each local step t < adapt_steps,
        multiplies it by 1 + adapt_rate / sqrt(t + 1) * (accepted - target_accept); steps t >= adapt_steps and global steps leave
        it alone.  The same draws and invariances, with the step handed from launch to launch: the result then also carries step
        [C] float64 (the walkers' steps after the launch; step_in itself, or `step_size`, at steps = 0) and, with history=True,
        hist_step [C, steps] (after every step; None at steps = 0).  ValueError for adapt_steps < 0 or a misshapen step_in; the
        library refuses adapt_rate outside [0, 1] and target_accept outside (0, 1).
        like_data: None -- the entries above, as they were; the descriptor of a Gaussian likelihood from user data
        (likelihoods.GaussianData.hip_like_data: mu [D] and R [D, D] float32, logl0) -- `like_id` must then be None, and the run goes
        through the family's `mcmc_gdata` entry (nnest_mcmc_gdata_steps, nnest_spline_mcmc_gdata_steps: the adaptive walk with that
        likelihood compiled in) whatever beta, global_every, adapt_steps and step_in are; the result carries the keys the same
        arguments give above.
        like_glm: None -- the entries above, as they were; the descriptor of a regression likelihood of user data
        (likelihoods.GLMData.hip_like_glm: at [D, ld], y [ld], o [ld] float32, logl0, n, family) -- `like_id` and `like_data` must
        then be None, and the run goes through the family's `mcmc_glm` entry (nnest_mcmc_glm_steps, nnest_spline_mcmc_glm_steps)
        in the same way, with the same keys.
        prior_gauss: None -- the entries above, as they were, bit for bit; the descriptor of independent normal priors on T(x)
        (priors.GaussianPrior.hip_gauss_prior: m [D], r = 1 / sigma [D] float32, logc) -- only with a `like_glm` (ValueError naming
        prior_gauss otherwise), and the run goes through the family's `mcmc_glm_prior` entry (nnest_mcmc_glm_prior_steps,
        nnest_spline_mcmc_glm_prior_steps): lp = ((beta logL) + log|det|) + log pi, -inf outside lo / hi, with the same keys.
        NotImplementedError for a family without such a kernel (its handle must not reach another family's)."""
        global_every = int(global_every)
        if global_every < 0:
            raise ValueError('mcmc_steps: global_every=%d (>= 0)' % global_every)
        adapt_steps = int(adapt_steps)
        if adapt_steps < 0:
            raise ValueError('mcmc_steps: adapt_steps=%d (>= 0)' % adapt_steps)
        adapt = adapt_steps > 0 or step_in is not None
        mixed = global_every > 0
        glm = like_glm is not None
        if glm and (like_id is not None or like_data is not None):
            raise ValueError('mcmc_steps: like_glm goes with like_id=None and like_data=None')
        gprior = prior_gauss is not None
        if gprior and not glm:
            raise ValueError('mcmc_steps: prior_gauss goes only with a like_glm (a GaussianPrior beside a regression likelihood of user data)')
        gdata = like_data is not None or glm   # (either descriptor: the adaptive entry's arguments, whatever the options)
        if gdata and like_id is not None:
            raise ValueError('mcmc_steps: like_data goes with like_id=None, got like_id=%r' % (like_id,))
        fn = self._sym.get('mcmc_glm_prior' if gprior else 'mcmc_glm' if glm else 'mcmc_gdata' if gdata else 'mcmc_adapt' if adapt else 'mcmc_mixed' if mixed else 'mcmc' if beta is None
                           else 'mcmc_tempered')
        if fn is None:
            raise NotImplementedError('no fused %srandom-walk Metropolis kernel for %s%s' % (
                'adaptive ' if adapt else 'mixed ' if mixed else '' if beta is None else 'tempered ', type(self).__name__,
                ' on a regression likelihood of user data under a normal prior' if gprior else ' on a regression likelihood of user data' if glm else ' on a Gaussian likelihood from user data' if gdata else ''))
        tempered = () if beta is None and not mixed and not adapt and not gdata else (ctypes.c_double(1.0 if beta is None else float(beta)),)
        dev = self.device
        z = _as_dev_f32(z, dev).contiguous()
        C, D, steps = z.shape[0], self.D, int(steps)
        if z.shape != (C, D):
            raise ValueError('mcmc_steps: z must be shaped [C, %d], got %s' % (D, tuple(z.shape)))
        if (lp is None) != (logl is None):
            raise ValueError('mcmc_steps: lp and logl: both or neither')
        f32 = dict(dtype=torch.float32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        t_std, t_mean, lo_t, hi_t = target_vectors('mcmc_steps', dev, t_std, t_mean, lo, hi, D=D)
        if lp is not None:
            lp = torch.as_tensor(lp, dtype=torch.float64).to(dev).contiguous()
            logl = torch.as_tensor(logl, dtype=torch.float64).to(dev).contiguous()
        hist = bool(history) and steps > 0
        out = dict(z=torch.empty(C, D, **f32) if steps > 0 else z, x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64),
                   logl=torch.empty(C, **f64),
                   hist_z=torch.empty(C, steps, D, **f32) if hist else None, hist_x=torch.empty(C, steps, D, **f32) if hist else None,
                   hist_logl=torch.empty(C, steps, **f64) if hist else None,
                   n_accept=torch.empty(C, dtype=torch.int32, device=dev) if steps > 0 else torch.zeros(C, dtype=torch.int32, device=dev))
        if mixed:
            out['n_accept_global'] = (torch.empty if steps > 0 else torch.zeros)(C, dtype=torch.int32, device=dev)
            tempered += (global_every, _lib.ptr(out['n_accept_global']))
        elif gdata:
            tempered += (0, None)
        if gdata and not adapt:   # (the adaptive entry's arguments with the adaptation off: the mixed walk)
            tempered += (None, None, None, ctypes.c_uint32(0), ctypes.c_double(float(adapt_rate)), ctypes.c_double(float(target_accept)))
        if adapt:
            if step_in is not None:
                step_in = torch.as_tensor(step_in, dtype=torch.float64).to(dev).contiguous()
                if step_in.shape != (C,):
                    raise ValueError('mcmc_steps: step_in must be shaped [%d], got %s' % (C, tuple(step_in.shape)))
            if steps > 0:
                out['step'] = torch.empty(C, **f64)
            else:   # (nothing is stepped: the start's steps, unclamped)
                out['step'] = step_in if step_in is not None else torch.full((C,), float(np.float32(step_size)), **f64)
            out['hist_step'] = torch.empty(C, steps, **f64) if hist else None
            if not mixed and not gdata:
                tempered += (0, None)
            tempered += (_lib.ptr(step_in), _lib.ptr(out['step']) if steps > 0 else None, _lib.ptr(out['hist_step']),
                         ctypes.c_uint32(min(adapt_steps, 0xFFFFFFFF)), ctypes.c_double(float(adapt_rate)), ctypes.c_double(float(target_accept)))
        with torch.cuda.device(dev):
            if glm:
                lk, keep = glm_spec(like_glm, dev)   # (`keep`, as below)
                if gprior:
                    pspec, pkeep = gauss_prior_spec(prior_gauss, dev)
            elif gdata:
                lk, keep = gdata_spec(like_data, dev)   # (`keep`: the staged arrays, alive until the call has been enqueued)
            else:
                lk = _lib.like_spec(like_id, 1.0, like_params)
            _lib.check(fn(
                self._h, ctypes.byref(lk), *((ctypes.byref(pspec),) if gprior else ()), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo_t),
                _lib.ptr(hi_t), _lib.ptr(z), _lib.ptr(lp),
                _lib.ptr(logl), _lib.ptr(out['z']) if steps > 0 else None, _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']),
                _lib.ptr(out['hist_z']), _lib.ptr(out['hist_x']), _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, steps,
                ctypes.c_float(float(step_size)), int(step0) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF,
                int(walker_offset) & 0xFFFFFFFFFFFFFFFF, *tempered, _lib.current_stream(dev)))
        return out

    def mcmc_mixed_refusal(self, like_id):
        """why `mcmc_steps` with global_every > 0 would refuse this flow (its shape, its base) or this likelihood id -- the library's
        own words (the family's `mcmc_mixed_check` entry; nothing is launched) --, or None where it is taken.  NotImplementedError
        for a family without such a kernel"""
        fn = self._sym.get('mcmc_mixed_check')
        if fn is None or 'mcmc_mixed' not in self._sym:
            raise NotImplementedError('no fused mixed random-walk Metropolis kernel for %s' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, int(like_id))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def mcmc_gdata_refusal(self, D=None):
        """why `mcmc_steps` with a like_data of dimension D (None: the flow's own) would refuse this flow (its shape, its base) -- the
        library's own words (the family's `mcmc_gdata_check` entry; nothing is launched) --, or None where it is taken.
        NotImplementedError for a family without such a kernel"""
        fn = self._sym.get('mcmc_gdata_check')
        if fn is None or 'mcmc_gdata' not in self._sym:
            raise NotImplementedError('no fused random-walk Metropolis kernel for %s on a Gaussian likelihood from user data' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, self.D if D is None else int(D))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def mcmc_glm_refusal(self, D=None):
        """why `mcmc_steps` with a like_glm of dimension D (None: the flow's own) would refuse this flow (its shape, its base) -- the
        library's own words (the family's `mcmc_glm_check` entry; nothing is launched) --, or None where it is taken.
        NotImplementedError for a family without such a kernel"""
        fn = self._sym.get('mcmc_glm_check')
        if fn is None or 'mcmc_glm' not in self._sym:
            raise NotImplementedError('no fused random-walk Metropolis kernel for %s on a regression likelihood of user data' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, self.D if D is None else int(D))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def mcmc_glm_prior_refusal(self, D=None):
        """why `mcmc_steps` with a like_glm of dimension D (None: the flow's own) and a prior_gauss would refuse this flow (its shape,
        its base) -- the library's own words (the family's `mcmc_glm_prior_check` entry; nothing is launched) --, or None where it is
        taken.  NotImplementedError for a family without such a kernel"""
        fn = self._sym.get('mcmc_glm_prior_check')
        if fn is None or 'mcmc_glm_prior' not in self._sym:
            raise NotImplementedError('no fused random-walk Metropolis kernel for %s on a regression likelihood of user data under a normal '
                                      'prior' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, self.D if D is None else int(D))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def mcmc_adapt_refusal(self, like_id):
        """why `mcmc_steps` with adapt_steps > 0 or a step_in would refuse this flow (its shape, its base) or this likelihood id --
        the library's own words (the family's `mcmc_adapt_check` entry; nothing is launched) --, or None where it is taken.
        NotImplementedError for a family without such a kernel"""
        fn = self._sym.get('mcmc_adapt_check')
        if fn is None or 'mcmc_adapt' not in self._sym:
            raise NotImplementedError('no fused adaptive random-walk Metropolis kernel for %s' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, int(like_id))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def importance_refusal(self, like_id):
        """why `importance_evidence` would refuse this flow (its shape, its base) or this likelihood id -- the library's own words
        (the family's `importance_check` entry; nothing is launched) --, or None where it is taken.  NotImplementedError for a
        family without such a kernel"""
        fn = self._sym.get('importance_check')
        if fn is None or 'importance' not in self._sym:
            raise NotImplementedError('no fused importance-sampling kernel for %s' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, int(like_id))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def importance_glm_refusal(self, D=None):
        """why `importance_evidence` with a like_glm of dimension D (None: the flow's own) would refuse this flow (its shape, its
        base) -- the library's own words (the family's `importance_glm_check` entry; nothing is launched) --, or None where it is
        taken.  NotImplementedError for a family without such a kernel"""
        fn = self._sym.get('importance_glm_check')
        if fn is None or 'importance_glm' not in self._sym:
            raise NotImplementedError('no fused importance-sampling kernel for %s on a regression likelihood of user data' % type(self).__name__)
        with torch.cuda.device(self.device):
            rc = fn(self._h, self.D if D is None else int(D))
        if rc == _lib.NNEST_OK:
            return None
        msg = self._lib.nnest_hip_last_error()
        return msg.decode() if msg else 'error %d' % rc

    def importance_evidence(self, like_id, M, t_std=None, t_mean=None, lo=None, hi=None, seed=0, sample_offset=0, like_params=None,
                            want_samples=False, like_glm=None, prior_gauss=None):
        """the sums of the importance-sampled evidence with this flow as the proposal, M samples drawn, evaluated and reduced in ONE
        launch (the family's `importance` entry point: nnest_importance_evidence, nnest_spline_importance_evidence; build-defined:
        include/nnest_hip.h has the definition).  The likelihood `like_id` sees T(x) = x * t_std + t_mean (per dimension; None:
        identity); lo / hi [D]: the prior box on T(x) (None: no prior); sample_offset: the global index of sample 0 -- a sample
        depends on (seed, global index) only, so a run cut into launches is the same run.  Returns a dict: sums [4] float64 on the
        device ({a, S1, S2, n_live}: _lib.merge_importance / importance_result read them) and, with want_samples, z, x [M, D]
        float32 (x before T), logl, logw [M] float64.  Asynchronous on the current stream.
        like_glm: None -- the entry above, as it was; the descriptor of a regression likelihood of user data
        (likelihoods.GLMData.hip_like_glm, as `mcmc_steps` takes it) -- `like_id` must then be None, and the launch goes through the
        family's `importance_glm` entry (nnest_importance_glm_evidence, nnest_spline_importance_glm_evidence), with the same keys.
        prior_gauss: None, or the descriptor of independent normal priors on T(x) (priors.GaussianPrior.hip_gauss_prior) -- only
        with a like_glm and without lo / hi (ValueError otherwise): lp = (logL + log|det|) + log pi.
        NotImplementedError for a family without such a kernel (its handle must not reach another family's)."""
        glm = like_glm is not None
        gprior = prior_gauss is not None
        if glm and like_id is not None:
            raise ValueError('importance_evidence: like_glm goes with like_id=None, got like_id=%r' % (like_id,))
        if gprior and not glm:
            raise ValueError('importance_evidence: prior_gauss goes only with a like_glm (a GaussianPrior beside a regression likelihood of '
                             'user data)')
        if gprior and (lo is not None or hi is not None):
            raise ValueError('importance_evidence: prior_gauss goes without lo / hi (the prior is the normal one or the box, not both)')
        fn = self._sym.get('importance_glm' if glm else 'importance')
        if fn is None:
            raise NotImplementedError('no fused importance-sampling kernel for %s%s' % (
                type(self).__name__, ' on a regression likelihood of user data' if glm else ''))
        dev = self.device
        M, D = int(M), self.D
        if M < 0:
            raise ValueError('importance_evidence: M=%d' % M)
        f32 = dict(dtype=torch.float32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        t_std, t_mean, lo_t, hi_t = target_vectors('importance_evidence', dev, t_std, t_mean, lo, hi, D=D)
        out = dict(sums=torch.empty(4, **f64))
        if want_samples:
            out.update(z=torch.empty(M, D, **f32), x=torch.empty(M, D, **f32), logl=torch.empty(M, **f64), logw=torch.empty(M, **f64))
        with torch.cuda.device(dev):
            groups = int(self._lib.nnest_importance_groups(M, self._IMPORTANCE_TILE))
            if groups < 0:
                raise _lib.NnestHipError('nnest_importance_groups(%d, %d) failed' % (M, self._IMPORTANCE_TILE))
            partials = torch.empty(3 * max(groups, 1), **f64)
            if glm:
                lk, keep = glm_spec(like_glm, dev)   # (`keep`: the staged arrays, alive until the call has been enqueued)
                pspec, pkeep = gauss_prior_spec(prior_gauss, dev) if gprior else (None, None)
            else:
                lk = _lib.like_spec(like_id, 1.0, like_params)
            _lib.check(fn(
                self._h, ctypes.byref(lk), *(((ctypes.byref(pspec) if gprior else None),) if glm else ()), _lib.ptr(t_std),
                _lib.ptr(t_mean), _lib.ptr(lo_t), _lib.ptr(hi_t), _lib.ptr(out.get('z')),
                _lib.ptr(out.get('x')), _lib.ptr(out.get('logl')), _lib.ptr(out.get('logw')), _lib.ptr(partials), _lib.ptr(out['sums']), M,
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset) & 0xFFFFFFFFFFFFFFFF, _lib.current_stream(dev)))
        out['groups'] = groups
        return out

    def mh_form_for(self, C, dynamic=False, lag=None, free=False, form=None, warm=0):
        """the K4 form (name) `mh_steps` runs for C walkers under this step rule -- asked of the library
        (nnest_mh_form_for), which knows the shapes each form is built for; None if the launch would be refused.  A caller
        that shards one batch over ranks asks for the WHOLE batch and pins the answer on every shard."""
        fn = getattr(self._lib, 'nnest_mh_form_for', None) if self._sym.get('mh') is getattr(self._lib, 'nnest_mh_constrained_steps', None) else None
        if fn is None:
            return None
        f = fn(self._h, int(C), _lib.mh_flags(dynamic, free, lag, form, warm))
        return _lib.MH_FORM_NAMES.get(f)

    def default_lag(self, C, form=None):
        """steps between an MCMC step and the proposal scale that reflects its batch-wide accept count when the caller names
        none.  The count of a step reaches every compute unit about 4.5 us after the step ended (atomics -> publishing wave ->
        one fetch); the lag is what keeps that off the step's critical path: 4 steps of the 2 us forms, 8 steps of the solo
        form's 1.2 us.  0 is the reference's rule exactly."""
        if form == 'solo' or (form is None and self.mh_form_for(C, dynamic='batch', lag=_lib.MH_SOLO_LAG) == 'solo'):
            return _lib.MH_SOLO_LAG
        return _lib.MH_DEFAULT_LAG

    def default_warm(self, C, dynamic, lag, form=None):
        """exact steps in front of a lagged batch rule when the caller names none: MH_WARM_STEPS where the form that runs
        implements them (the solo form), 0 elsewhere.  Every launch restarts the rule from the caller's step_size with gain
        1 / (1 + votes): its first votes move the scale by e-folds, and a lag there is so many steps spent at the initial
        scale."""
        if dynamic not in (True, 'batch') or not lag:
            return 0
        w = _lib.MH_WARM_STEPS
        return w if self.mh_form_for(C, dynamic='batch', lag=lag, form=form, warm=w) == 'solo' else 0

    @staticmethod
    def check_sync(res):
        """raise if a bounded wait of the batch-wide step rule ran out (a workgroup was not resident); synchronises"""
        if res.get('sync') is not None and int(res['sync'][-1].item()) != 0:
            raise _lib.NnestHipError('batch-wide step rule: a wait on the per-step counters ran out')

    def fill_noise(self, steps, C, seed=0, walker_offset=0):
        dz = torch.empty(steps, C, self.D, dtype=torch.float32, device=self.device)
        u = torch.empty(steps, C, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_mh_fill_noise(_lib.ptr(dz), _lib.ptr(u), steps, C, self.D,
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset),
                                                     _lib.current_stream(self.device)))
        return dz, u


def split_move_word(word):
    """the proposal kernels' n_accept / n_move word -> (count, moved): bit NNEST_MH_ALL_MOVED says that every coordinate of the
    chain's last x differs from its first (the reference's usable-chain test, nested.py:432)"""
    return word & (_lib.MH_ALL_MOVED - 1), (word & _lib.MH_ALL_MOVED) != 0


class _MhResult(dict):
    """what mh_steps returns; 'n_accept' (the count) and 'moved' (the reference's usable-chain test, nested.py:432) are split off
    the kernel's word (NNEST_MH_ALL_MOVED) when first asked for"""

    def __missing__(self, key):
        if key in ('n_accept', 'moved'):
            self['n_accept'], self['moved'] = split_move_word(dict.__getitem__(self, 'n_accept_word'))
            return dict.__getitem__(self, key)
        raise KeyError(key)

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default


def train_epochs_host(net, epoch_body, xtrain, xvalid, perm, noise, seed, jitter, batch, max_epochs, patience, lr, weight_decay,
                      valid_sum=None):
    """Trainer.train's epoch loop (nnest/trainer.py:198-241, :384-418) driven from the host, for every flow and shape the one-launch
    training kernels do not take (HipNVP / HipSpline at batch_size > 128, and the MAF, Cholesky and fast/slow flows always): train an
    epoch, validate, keep the best weights, count patience, restore the best.  A slower path (a few launches per minibatch), not a
    refusal.  Needs nothing of `net` but store_packed / load_packed / log_probs / device (and `P`, handed back to load_packed where
    the flow has one), so the books run on the CPU with a stand-in (tests/test_host_epoch_loop.py).

    epoch_body(rows, epoch, n_train, batch, lr, weight_decay) pushes one epoch's minibatches through the flow and returns the sum of
    their losses (a device scalar, read back together with the validation loss, or a float).  rows(epoch, lo, hi) are that epoch's
    rows lo..hi in loader order with the jitter added (data + jitter * randn_like(data), trainer.py:392): recorded `noise`, or draws
    of one generator seeded from `seed` -- in the order the body asks, so a body that asks for the whole epoch at once and one that
    asks per minibatch see different draws, and each flow keeps the granularity it has.
    valid_sum(xvalid): the validation loss before the division by n_valid; None = -mean over the whole set in one batch, as the
    reference's valid_loader has it (trainer.py:190, :405-418).  Arguments and return value as HipNVP.train_epochs."""
    dev = net.device
    xtrain = _as_dev_f32(xtrain, dev)
    xvalid = _as_dev_f32(xvalid, dev)
    n_train, n_valid, D = xtrain.shape[0], xvalid.shape[0], xtrain.shape[1]
    perm = perm.to(device=dev, dtype=torch.int64).view(max_epochs, n_train)
    if noise is not None:
        noise = noise.to(device=dev, dtype=torch.float32).view(max_epochs, n_train, D)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)

    def rows(epoch, lo, hi):
        r = xtrain[perm[epoch, lo:hi]]
        if jitter != 0.0:
            nz = noise[epoch, lo:hi] if noise is not None else torch.randn(r.shape, device=dev, generator=gen)
            r = r + float(jitter) * nz
        return r

    losses = np.zeros((max(max_epochs, 1), 2), np.float32)
    best, best_epoch, counter, stopped, epochs_run = float('inf'), 0, 0, False, 0
    best_w = net.store_packed()                                            # best_model = deepcopy(netG)  trainer.py:194
    for epoch in range(max_epochs):
        tot = epoch_body(rows, epoch, n_train, int(batch), lr, weight_decay)   # train_loss += loss.item()  trainer.py:398
        vsum = -net.log_probs(xvalid).mean() if valid_sum is None else valid_sum(xvalid)
        if torch.is_tensor(tot):
            tot, vsum = torch.stack([tot, vsum.to(tot.dtype)]).cpu().tolist()  # one read-back per epoch
        train_loss, valid_loss = tot / n_train, float(vsum) / n_valid      # trainer.py:403, :418
        losses[epoch] = (train_loss, valid_loss)
        epochs_run = epoch + 1
        if valid_loss < best:                                              # trainer.py:205-209
            best, best_epoch, counter, best_w = valid_loss, epoch + 1, 0, net.store_packed()
        counter += 1
        if counter > patience:                                             # trainer.py:223-232
            stopped = True
            break
    P = getattr(net, 'P', None)                                            # the spline flows' permutations travel beside the packed vector
    if P is None:
        net.load_packed(best_w)                                            # netG.load_state_dict(best_model)  trainer.py:241
    else:
        net.load_packed(best_w, P)
    return dict(losses=torch.from_numpy(losses), epochs_run=epochs_run, best_epoch=best_epoch, best_validation_loss=best,
                last_train_loss=float(losses[max(epochs_run - 1, 0), 0]), counter=counter, stopped=stopped, result=None)


def chunked_epoch(net, chunk_rows):
    """the epoch body of HipNVP / HipSpline for train_epochs_host: per minibatch the gradient of -mean(log_probs) from `net.loss_grad`
    over chunks of at most `chunk_rows` rows -- the mean over M rows is the chunk means weighted m_c / M, exact up to rounding -- and
    one `net.adam_step`; one gather and one draw per epoch, a minibatch is a slice"""
    def body(rows, epoch, n_train, batch, lr, weight_decay):
        rows_all = rows(epoch, 0, n_train)
        tot = torch.zeros((), dtype=torch.float32, device=net.device)
        for lo in range(0, n_train, batch):
            mb = rows_all[lo:lo + batch]
            M = mb.shape[0]
            if getattr(net, 'data_dep_init_done', True) is False:          # ActNorm: the first minibatch pushed forward through a
                net.actnorm_init(mb.contiguous())                          # fresh spline flow initialises it (networks.py:698-705)
            grad = loss = None
            for c0 in range(0, M, int(chunk_rows)):
                part = mb[c0:c0 + int(chunk_rows)].contiguous()
                l_c, g_c = net.loss_grad(part)
                wgt = part.shape[0] / M
                grad = g_c * wgt if grad is None else grad + g_c * wgt
                loss = l_c[0] * wgt if loss is None else loss + l_c[0] * wgt
            net.adam_step(grad, lr, weight_decay)                          # trainer.py:400-401
            tot = tot + loss
        return tot
    return body


def native_hidden(H):
    """the hidden width the kernels are instantiated for that holds H: 16, 32 or 64 (one, two or four 16-wide matrix-core tiles);
    beyond 64 the next multiple of 16 (the library says what it cannot take)"""
    for w in (16, 32, 64):
        if H <= w:
            return w
    return -(-H // 16) * 16


def pad_index(blocks):
    """blocks: [(user_shape, native_shape, native_offset)] in the order of the user's packed vector -> for every element of that
    vector its position in the native one (a tensor of user_shape sits in the leading corner of a zero tensor of native_shape)."""
    out = []
    for su, sn, off in blocks:
        if len(su) == 0:
            out.append(np.array([off], dtype=np.int64))
            continue
        ix = np.indices(su).reshape(len(su), -1)
        out.append(np.ravel_multi_index(ix, sn).astype(np.int64) + off)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


class _PaddedVectors(object):
    """A flow whose hidden width is not a multiple of the 16-wide matrix-core tile runs on a native handle of the next multiple:
    the extra hidden units have zero weights in and out and zero biases.  That is EXACT, not an approximation: their
    pre-activations are 0, tanh 0 = relu 0 = leaky_relu 0 = 0, nothing flows out of them; in reverse mode the gradient reaching them
    is W_out^T g = 0 and the gradients of their own weights are products with those zeros; Adam with coupled weight decay maps
    (w, g, m, v) = (0, 0, 0, 0) to itself.  (The reference accepts any hidden_dim: nnest/networks.py:253-287, trainer.py:32-48.)
    `_pidx` (None when nothing is padded): position of every element of the user's packed vector in the native one."""
    _pidx = None
    _pidx_dev = None
    _native_params = None

    def _set_pad_index(self, idx, native_params):
        self._native_params = int(native_params)
        if idx is None or (len(idx) == native_params and np.array_equal(idx, np.arange(native_params))):
            self._pidx = self._pidx_dev = None
            return
        self._pidx = idx
        self._pidx_dev = torch.from_numpy(idx).to(self.device)

    def _to_native(self, vec):
        vec = np.ascontiguousarray(vec, dtype=np.float32)
        if self._pidx is None:
            return vec
        out = np.zeros(self._native_params, np.float32)
        out[self._pidx] = vec
        return out

    def _from_native(self, vec):
        return vec if self._pidx is None else np.ascontiguousarray(vec[self._pidx])

    def _native_buffer(self):
        return np.empty(self._native_params if self._native_params is not None else self.num_params, np.float32)

    def _to_native_dev(self, t):
        if self._pidx_dev is None:
            return t.contiguous()
        out = torch.zeros(self._native_params, dtype=torch.float32, device=self.device)
        out[self._pidx_dev] = t
        return out

    def _from_native_dev(self, t):
        return t if self._pidx_dev is None else t[self._pidx_dev].contiguous()


class HipNVP(_PaddedVectors, _HipFlow):
    """num_inputs=D, num_hidden=H, num_blocks=B, num_layers=L, scale as SingleSpeedNVP (networks.py:328-347).

    scale='translate' / 'constant' (translate-only couplings; 'constant' adds a ScaleLayer scalar after each block):
    state_dict() has the reference's keys (no scale nets; `flow.flows.<2b+1>.scale` scalars); the packed vector of
    the C ABI keeps the scale_net slots (zero) and appends the scalars (include/nnest_hip.h)."""

    def __init__(self, num_inputs, num_hidden=16, num_blocks=3, num_layers=1, device=None, seed=None, scale=''):
        if not torch.cuda.is_available():
            raise _lib.NnestHipError('HipNVP needs an MI355X visible to PyTorch-ROCm (torch.cuda.is_available() is False); '
                                     'there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.D, self.H, self.B, self.L = int(num_inputs), int(num_hidden), int(num_blocks), int(num_layers)
        self.num_inputs = self.D
        if scale not in SCALE_MODES:
            raise ValueError("scale=%r: expected '', 'translate' or 'constant' (networks.py:330-332)" % (scale,))
        self.scale = scale
        self._lib = _lib.load()
        self._bind('nnest_nvp', mh='nnest_mh_constrained_steps', slice='nnest_slice_steps', ensemble='nnest_ensemble_steps',
                   ensemble_max_walkers='nnest_ensemble_max_walkers', ensemble_moves='nnest_ensemble_moves_steps',
                   ensemble_moves_max_walkers='nnest_ensemble_moves_max_walkers', mcmc='nnest_mcmc_steps',
                   importance='nnest_importance_evidence', importance_check='nnest_importance_check',
                   mcmc_tempered='nnest_mcmc_tempered_steps', mcmc_mixed='nnest_mcmc_mixed_steps',
                   mcmc_mixed_check='nnest_mcmc_mixed_check', mcmc_adapt='nnest_mcmc_adapt_steps',
                   mcmc_adapt_check='nnest_mcmc_adapt_check', mcmc_gdata='nnest_mcmc_gdata_steps',
                   mcmc_gdata_check='nnest_mcmc_gdata_check', mcmc_glm='nnest_mcmc_glm_steps',
                   mcmc_glm_check='nnest_mcmc_glm_check', slice_glm='nnest_slice_glm_steps',
                   slice_glm_check='nnest_slice_glm_check', mh_glm='nnest_mh_glm_steps', mh_glm_check='nnest_mh_glm_check',
                   mcmc_glm_prior='nnest_mcmc_glm_prior_steps',
                   mcmc_glm_prior_check='nnest_mcmc_glm_prior_check', importance_glm='nnest_importance_glm_evidence',
                   importance_glm_check='nnest_importance_glm_check')
        self._h = ctypes.c_void_p()
        self._Hn = native_hidden(self.H)     # the native handle's hidden width (_PaddedVectors)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_nvp_create_scaled(self.D, self._Hn, self.B, self.L, SCALE_MODES[scale],
                                                         ctypes.byref(self._h)))
        self._init_padding()
        self.prior = torch.distributions.MultivariateNormal(torch.zeros(self.D, device=self.device),
                                                            torch.eye(self.D, device=self.device))
        self.load_packed(self.default_init(seed))

    ensemble_fused_by_default = True

    def supports_fused_slice(self, C):
        """nnest_slice_steps runs the reference's default coupling shape only (hidden 16, 3 blocks, 1 layer, scale '')"""
        return super().supports_fused_slice(C) and self._Hn == 16 and self.B == 3 and self.L == 1 and self.scale == ''

    def _init_padding(self):
        """num_params and the packed layout are the USER's (hidden width H); the native vector has width _Hn"""
        D, H, Hn, L, B = self.D, self.H, getattr(self, '_Hn', self.H), self.L, self.B
        native = self._lib.nnest_nvp_num_params(self._h)
        ns = H * D + H + L * (H * H + H) + D * H + D
        self.num_params = 2 * B * ns + (B if self.scale == 'constant' else 0)
        if Hn == H:
            assert self.num_params == native
            return self._set_pad_index(None, native)
        nn_ = Hn * D + Hn + L * (Hn * Hn + Hn) + D * Hn + D
        blocks = []
        for k in range(2 * B):
            off = k * nn_
            for su, sn in [((H, D), (Hn, D)), ((H,), (Hn,))] + [((H, H), (Hn, Hn)), ((H,), (Hn,))] * L + [((D, H), (D, Hn)), ((D,), (D,))]:
                blocks.append((su, sn, off))
                off += int(np.prod(sn))
        if self.scale == 'constant':
            blocks += [((), (), 2 * B * nn_ + b) for b in range(B)]
        self._set_pad_index(pad_index(blocks), native)
        assert len(self._pidx) == self.num_params

    # ---- weights ---------------------------------------------------------------------------------
    def layer_shapes(self):
        """[(name, shape, offset into the packed vector)] in torch state_dict order; with
        scale='translate'/'constant' a block has no scale_net, and with 'constant' the flows alternate coupling /
        ScaleLayer (networks.py:336-346)"""
        out = []
        D, H, L = self.D, self.H, self.L
        ns = H * D + H + L * (H * H + H) + D * H + D
        stride = 2 if self.scale == 'constant' else 1
        for b in range(self.B):
            for n, net in enumerate(('scale_net', 'translate_net')):
                if n == 0 and self.scale != '':
                    continue
                off = (2 * b + n) * ns
                dims = [(H, D)] + [(H, H)] * L + [(D, H)]
                for i, (o, k) in enumerate(dims):
                    out.append(('flow.flows.%d.%s.%d.weight' % (stride * b, net, 2 * i), (o, k), off))
                    off += o * k
                    out.append(('flow.flows.%d.%s.%d.bias' % (stride * b, net, 2 * i), (o,), off))
                    off += o
            if self.scale == 'constant':
                out.append(('flow.flows.%d.scale' % (2 * b + 1), (), 2 * self.B * ns + b))
        return out

    def default_init(self, seed=None):
        """nn.Linear's default init (kaiming_uniform(a=sqrt(5)) = U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for both
        weight and bias), which is what the reference ends up with: its orthogonal init closure is never
        applied (networks.py:284-287)."""
        g = torch.Generator()
        if seed is None:
            g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        else:
            g.manual_seed(int(seed))
        packed = np.zeros(self.num_params, np.float32)
        for name, shape, off in self.layer_shapes():
            if len(shape) == 0:
                continue                     # ScaleLayer scalar starts at 0 (networks.py:316)
            fan_in = shape[1] if len(shape) == 2 else None
            if fan_in is None:
                fan_in = last_fan_in
            else:
                last_fan_in = fan_in
            bound = 1.0 / math.sqrt(fan_in)
            n = int(np.prod(shape))
            packed[off:off + n] = ((torch.rand(n, generator=g) * 2 - 1) * bound).numpy()
        return packed

    def load_packed(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.float32)
        if packed.size != self.num_params:
            raise ValueError('expected %d packed weights, got %d' % (self.num_params, packed.size))
        packed = self._to_native(packed)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_nvp_load_weights(self._h, packed.ctypes.data_as(ctypes.c_void_p),
                                                        _lib.current_stream(self.device)))

    def store_packed(self):
        out = self._native_buffer()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_nvp_store_weights(self._h, out.ctypes.data_as(ctypes.c_void_p),
                                                         _lib.current_stream(self.device)))
        return self._from_native(out)

    def state_dict(self):
        return self.state_dict_from_packed(self.store_packed())

    def state_dict_from_packed(self, packed):
        """the reference's state_dict out of a packed-layout vector (no device access: safe on a worker thread)"""
        sd = {}
        for name, shape, off in self.layer_shapes():
            n = int(np.prod(shape))
            sd[name] = torch.from_numpy(packed[off:off + n].reshape(shape).copy())
        return sd

    def load_state_dict(self, sd):
        packed = np.zeros(self.num_params, np.float32)
        for name, shape, off in self.layer_shapes():
            v = sd[name]
            v = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32).ravel()
            packed[off:off + v.size] = v
        self.load_packed(packed)

    def reference_vector(self, packed=None):
        """the concatenated state_dict (what the reference's parameters() hold) out of a packed-layout vector"""
        packed = self.store_packed() if packed is None else np.asarray(packed)
        return np.concatenate([packed[off:off + int(np.prod(shape))] for _, shape, off in self.layer_shapes()])

    def load_reference_vector(self, vec):
        packed = np.zeros(self.num_params, np.float32)
        pos = 0
        for _, shape, off in self.layer_shapes():
            n = int(np.prod(shape))
            packed[off:off + n] = vec[pos:pos + n]
            pos += n
        self.load_packed(packed)

    def adam_step_count(self):
        n = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_nvp_adam_state(self._h, ctypes.byref(n), -1, 0, _lib.current_stream(self.device)))
        return n.value

    def adam_moments(self):
        """host copies of Adam's (exp_avg, exp_avg_sq)"""
        m = self._native_buffer()
        v = self._native_buffer()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_nvp_store_adam(self._h, m.ctypes.data_as(ctypes.c_void_p),
                                                      v.ctypes.data_as(ctypes.c_void_p), _lib.current_stream(self.device)))
        return self._from_native(m), self._from_native(v)

    def set_adam(self, m, v, step):
        m = self._to_native(m)
        v = self._to_native(v)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nnest_nvp_load_adam(self._h, m.ctypes.data_as(ctypes.c_void_p),
                                                     v.ctypes.data_as(ctypes.c_void_p), _lib.current_stream(self.device)))
            _lib.check(self._lib.nnest_nvp_adam_state(self._h, None, int(step), 0, _lib.current_stream(self.device)))

    def train_form_for(self, batch, one_cu=False):
        """(name, detail) of the kernel train_epochs runs minibatches of `batch` rows in (nnest_nvp_train_form): ('single', how many
        of the two fragment images live in LDS), ('grid', 10 NT + L) or ('rows', U)"""
        detail = ctypes.c_int(-1)
        form = self._lib.nnest_nvp_train_form(self._h, int(batch), _lib.TRAIN_ONE_CU if one_cu else 0, ctypes.byref(detail))
        if form < 0:
            raise _lib.NnestHipError('nnest_nvp_train_form: no training kernel takes batch=%d on this handle' % int(batch))
        return ('single', 'grid', 'rows')[form], detail.value

    def epoch_loop_on_host(self, batch, n_train):
        """whether train_epochs drives minibatches of `batch` rows out of n_train from the host (flow.train_epochs_host: a run in ONE
        call, no chunks -- Trainer.train asks before it cuts a run into launches).  The reference takes any batch_size (trainer.py:36,
        :76, :185), so more than 128 rows are a slower path, not a refusal; and so is a minibatch that one workgroup cannot stage
        (nnest_nvp_train_form answers -1: more than 96 / 64 rows at hidden 64 with two / three hidden layers, more than 112 at hidden 32
        with three and x_dim > 32) -- loss_grad splits such a batch over launches, the one-launch epoch loop cannot"""
        rows = max(1, min(int(batch), int(n_train)))
        return int(batch) > TRAIN_KERNEL_MAX_BATCH or self._lib.nnest_nvp_train_form(self._h, rows, 0, None) < 0

    def train_epochs(self, xtrain, xvalid, perm, noise=None, seed=0, jitter=0.0, batch=100, max_epochs=1, patience=50,
                     lr=1e-3, weight_decay=1e-6, epoch_offset=0, resume=False, finalize=True, result=None, one_cu=False):
        """K5: Trainer.train's epoch loop (trainer.py:198-241) in one launch.  perm int32 [max_epochs, n_train];
        noise None (in-kernel Philox) or float32 [max_epochs, n_train, D] in loader order.
        A long train() can be split into chunks: pass the previous chunk's `result` tensor with resume=True,
        epoch_offset = epochs already run, finalize=True only for the last chunk (see include/nnest_hip.h) -- except where
        epoch_loop_on_host(batch, n_train) says that the loop is driven from the host, which takes a run in one call.
        Returns dict(losses [epochs,2] tensor, epochs_run, best_epoch, best_validation_loss, last_train_loss,
        counter, stopped, result)."""
        dev = self.device
        if self.epoch_loop_on_host(batch, len(xtrain)):
            if resume or epoch_offset != 0:
                raise ValueError('batch_size %d on this flow: the host-driven epoch loop takes a run in one call (epoch_loop_on_host)' % int(batch))
            return train_epochs_host(self, chunked_epoch(self, TRAIN_KERNEL_MAX_BATCH), xtrain, xvalid, perm, noise, seed, jitter, batch,
                                     max_epochs, patience, lr, weight_decay)
        xtrain = _as_dev_f32(xtrain, dev)
        xvalid = _as_dev_f32(xvalid, dev)
        perm = perm.to(device=dev, dtype=torch.int32).contiguous()
        n_train, n_valid = xtrain.shape[0], xvalid.shape[0]
        assert perm.numel() == max_epochs * n_train
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            assert noise.numel() == max_epochs * n_train * self.D
        losses = torch.zeros(max(max_epochs, 1), 2, dtype=torch.float32, device=dev)
        if result is None:
            assert not resume
            result = torch.zeros(6, dtype=torch.int32, device=dev)  # nnest_train_result_t
        flags = (_lib.TRAIN_RESUME if resume else 0) | (_lib.TRAIN_FINALIZE if finalize else 0) | (_lib.TRAIN_ONE_CU if one_cu else 0)
        with torch.cuda.device(dev):
            _lib.check(self._lib.nnest_nvp_train(self._h, _lib.ptr(xtrain), n_train, _lib.ptr(xvalid), n_valid,
                                                 _lib.ptr(perm), _lib.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                 float(jitter), int(batch), int(max_epochs), int(patience), float(lr),
                                                 float(weight_decay), int(epoch_offset), flags, _lib.ptr(losses),
                                                 _lib.ptr(result), _lib.current_stream(dev)))
        r = result.cpu()
        if int(r[5]) == 2:
            raise _lib.NnestHipError('nnest_nvp_train: a grid barrier of the multi-CU training kernel ran out (results invalid; error word 0x%x)' % (int(r[4]) & 0xffffffff))
        fl = r[2:4].view(torch.float32)
        return dict(losses=losses, epochs_run=int(r[0]), best_epoch=int(r[1]), best_validation_loss=float(fl[0]),
                    last_train_loss=float(fl[1]), counter=int(r[4]), stopped=bool(int(r[5])), result=result)


def loglike(like_id, x_unit, like_scale, device=None, like_params=None):
    """K6: batched analytic likelihood through safe_loglike (sampler.py:110-133): float64 [N]."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    x = _as_dev_f32(x_unit, device)
    out = torch.empty(x.shape[0], dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        lk = _lib.like_spec(like_id, like_scale, like_params)
        _lib.check(_lib.load().nnest_loglike(ctypes.byref(lk), _lib.ptr(x), _lib.ptr(out), x.shape[0],
                                             x.shape[1], _lib.current_stream(device)))
    return out


def mcmc_fill_noise(steps, C, D, seed=0, step0=0, walker_offset=0, device=None):
    """the draws of the fused random-walk Metropolis kernels (nnest_mcmc_fill_noise), exported for the checker through the kernels' own
    functions: (eps [steps, C, D], u [steps, C]) float32, for steps step0 .. and walkers walker_offset .. (flow-independent)"""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    dz = torch.empty(int(steps), int(C), int(D), dtype=torch.float32, device=dev)
    u = torch.empty(int(steps), int(C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nnest_mcmc_fill_noise(_lib.ptr(dz), _lib.ptr(u), int(steps), int(C), int(D), int(step0) & 0xFFFFFFFFFFFFFFFF,
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset) & 0xFFFFFFFFFFFFFFFF,
                                                     _lib.current_stream(dev)))
    return dz, u


def gdata_spec(data, device):
    """the nnest_gdata_t of a Gaussian likelihood from user data on `device`: data = the mapping likelihoods.GaussianData.hip_like_data
    holds (mu [D] and R [D, D] float32, arrays or tensors; logl0).  Arrays already on the device are used as they are.  Returns
    (spec, keep): `keep` holds the staged tensors the spec points into"""
    mu = _as_dev_f32(data['mu'], device).reshape(-1)   # (a [D] array comes back as [1, D])
    R = _as_dev_f32(data['R'], device)
    D = mu.shape[0]
    if D < 1 or R.shape != (D, D):
        raise ValueError('like_data: mu must be shaped [D] and R [D, D], got %s and %s' % (tuple(mu.shape), tuple(R.shape)))
    return _lib.GdataSpec(mu.data_ptr(), R.data_ptr(), float(data['logl0']), D), (mu, R)


def loglike_gdata(data, t, device=None):
    """the Gaussian likelihood from user data alone (nnest_loglike_gdata; include/nnest_hip.h has the arithmetic): data as
    `gdata_spec` takes it, t [N, D] rows that are already T(x) (float32 on the device, or anything convertible).  Returns logL [N]
    float64 on the device.  Asynchronous on the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _as_dev_f32(t, dev).contiguous()
    if t.dim() != 2:
        raise ValueError('loglike_gdata: t must be shaped [N, D], got %s' % (tuple(t.shape),))
    N, D = t.shape
    out = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        spec, keep = gdata_spec(data, dev)
        _lib.check(_lib.load().nnest_loglike_gdata(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(out), N, D, _lib.current_stream(dev)))
    return out


def glm_spec(data, device):
    """the nnest_glm_t of a regression likelihood of user data on `device`: data = the mapping likelihoods.GLMData.hip_like_glm holds
    (at [D, ld], y [ld], o [ld] float32, arrays or tensors; logl0; n; family 'logistic' | 'poisson' or the library's number).  Arrays
    already on the device are used as they are.  Returns (spec, keep): `keep` holds the staged tensors the spec points into.
    ValueError for misshapen arrays or an unknown family name; the ranges are the library's to refuse"""
    at = _as_dev_f32(data['at'], device)
    y = _as_dev_f32(data['y'], device).reshape(-1)   # (a [ld] array comes back as [1, ld])
    o = _as_dev_f32(data['o'], device).reshape(-1)
    if at.dim() != 2 or at.shape[0] < 1 or y.shape != (at.shape[1],) or o.shape != (at.shape[1],):
        raise ValueError('like_glm: at must be shaped [D, ld], y and o [ld], got %s, %s and %s' % (tuple(at.shape), tuple(y.shape), tuple(o.shape)))
    at, y, o = at.contiguous(), y.contiguous(), o.contiguous()
    fam = data['family']
    if isinstance(fam, str):
        if fam not in _lib.GLM_FAMILIES:
            raise ValueError('like_glm: family=%r (one of %s)' % (fam, sorted(_lib.GLM_FAMILIES)))
        fam = _lib.GLM_FAMILIES[fam]
    D, ld = at.shape
    return _lib.GlmSpec(at.data_ptr(), y.data_ptr(), o.data_ptr(), float(data['logl0']), int(data['n']), ld, D, int(fam)), (at, y, o)


def loglike_glm(data, t, device=None):
    """a regression likelihood of user data alone (nnest_loglike_glm; include/nnest_hip.h has the arithmetic): data as `glm_spec`
    takes it, t [N, D] rows that are already T(x) (float32 on the device, or anything convertible).  Returns logL [N] float64 on the
    device.  Asynchronous on the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _as_dev_f32(t, dev).contiguous()
    if t.dim() != 2:
        raise ValueError('loglike_glm: t must be shaped [N, D], got %s' % (tuple(t.shape),))
    N, D = t.shape
    out = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        spec, keep = glm_spec(data, dev)
        _lib.check(_lib.load().nnest_loglike_glm(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(out), N, D, _lib.current_stream(dev)))
    return out


def _glm_pointwise(entry, slots, data, t, device):
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _as_dev_f32(t, dev).contiguous()
    if t.dim() != 2:
        raise ValueError('%s: t must be shaped [S, D], got %s' % (entry, tuple(t.shape),))
    S, D = t.shape
    with torch.cuda.device(dev):
        spec, keep = glm_spec(data, dev)
        if S == 0:
            t = torch.zeros(1, D, dtype=torch.float32, device=dev)   # (an empty tensor has no pointer; the entry reads nothing of it)
        n = max(int(spec.n), 1)
        G = max(_lib.load().nnest_glm_pointwise_groups(S, n), 1)   # (-1: a shape the entry refuses before it touches the partials)
        out = torch.empty(n, slots, dtype=torch.float64, device=dev)
        partials = torch.empty(G * n * slots, dtype=torch.float64, device=dev)
        _lib.check(getattr(_lib.load(), entry)(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(out), _lib.ptr(partials), S, D,
                                               _lib.current_stream(dev)))
    return out


def glm_pointwise(data, t, device=None):
    """the pointwise predictive statistics of a regression likelihood of user data over the draws t (nnest_glm_pointwise;
    include/nnest_hip.h has the definition): data as `glm_spec` takes it, t [S, D] rows that are already T(x) (float32 on the device,
    or anything convertible; S = 0 is valid).  Returns [n, 8] float64 on the device: per data row {a, P, b, Q, Q2, cnt, mean, M2}
    over the live draws.  Deterministic: the same call twice returns the same bits.  Asynchronous on the current stream."""
    return _glm_pointwise('nnest_glm_pointwise', 8, data, t, device)


def glm_predict(data, t, device=None):
    """the posterior predictive mean at new design rows (nnest_glm_predict): data as `glm_spec` takes it with A_new and offset_new in
    the places of A and the offset (y is ignored), t [S, D] as in `glm_pointwise`.  Returns [n_new, 3] float64 on the device: per new
    row {cnt, mean, M2} of the inverse link -- 1 / (1 + exp(-eta)) or exp(eta) -- over the live draws.  Asynchronous on the current
    stream."""
    return _glm_pointwise('nnest_glm_predict', 3, data, t, device)


def glm_terms(data, t, device=None):
    """the matrix of terms l_is = log p(y_i | theta_s) of a regression likelihood of user data over the draws t (nnest_glm_terms):
    data and t as `glm_pointwise` takes them.  Returns [S, n] float64 on the device, NaN for a dead pair, with the bits
    `glm_pointwise` reduced.  Asynchronous on the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _as_dev_f32(t, dev).contiguous()
    if t.dim() != 2:
        raise ValueError('glm_terms: t must be shaped [S, D], got %s' % (tuple(t.shape),))
    S, D = t.shape
    with torch.cuda.device(dev):
        spec, keep = glm_spec(data, dev)
        n = max(int(spec.n), 1)
        out = torch.empty(S, n, dtype=torch.float64, device=dev)
        if S == 0:
            return out
        _lib.check(_lib.load().nnest_glm_terms(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(out), S, D, _lib.current_stream(dev)))
    return out


def glm_psis(data, t, device=None, with_work=False):
    """Pareto-smoothed leave-one-out of a regression likelihood of user data over the draws t (nnest_glm_psis; include/nnest_hip.h
    has the definition): data and t as `glm_pointwise` takes them, at most 2^20 draws.  Runs nnest_glm_pointwise first for the row
    statistics.  Returns (stats [n, 8], out [n, 16]) float64 on the device -- with_work: and the work buffer (uint8), whose first
    n Mcap doubles are the rows' sorted tails.  Deterministic.  Asynchronous on the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _as_dev_f32(t, dev).contiguous()
    if t.dim() != 2:
        raise ValueError('glm_psis: t must be shaped [S, D], got %s' % (tuple(t.shape),))
    S, D = t.shape
    stats = glm_pointwise(data, t, dev)
    with torch.cuda.device(dev):
        spec, keep = glm_spec(data, dev)
        if S == 0:
            t = torch.zeros(1, D, dtype=torch.float32, device=dev)   # (an empty tensor has no pointer; the entry reads nothing of it)
        n = max(int(spec.n), 1)
        nbytes = int(_lib.load().nnest_glm_psis_work_bytes(S, n))
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)   # (-1: a shape the entry refuses before it touches the buffer)
        out = torch.empty(n, 16, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().nnest_glm_psis(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(stats), _lib.ptr(out), _lib.ptr(work), S, D,
                                              _lib.current_stream(dev)))
    return (stats, out, work) if with_work else (stats, out)


def gauss_prior_spec(data, device):
    """the nnest_gauss_prior_t of independent normal priors on `device`: data = the mapping priors.GaussianPrior.hip_gauss_prior holds
    (m [D] and r = 1 / sigma [D] float32, arrays or tensors; logc).  Arrays already on the device are used as they are.  Returns
    (spec, keep): `keep` holds the staged tensors the spec points into.  ValueError for misshapen arrays; the ranges are the
    library's to refuse"""
    m = _as_dev_f32(data['m'], device).reshape(-1).contiguous()   # (a [D] array comes back as [1, D])
    r = _as_dev_f32(data['r'], device).reshape(-1).contiguous()
    if m.shape[0] < 1 or r.shape != m.shape:
        raise ValueError('prior_gauss: m and r must both be shaped [D], got %s and %s' % (tuple(m.shape), tuple(r.shape)))
    return _lib.GaussPriorSpec(m.data_ptr(), r.data_ptr(), float(data['logc']), m.shape[0]), (m, r)


def logprior_gauss(data, t, device=None):
    """independent normal priors alone (nnest_logprior_gauss; include/nnest_hip.h has the arithmetic): data as `gauss_prior_spec`
    takes it, t [N, D] rows that are already T(x) (float32 on the device, or anything convertible).  Returns log pi [N] float64 on
    the device (-inf on a row with a non-finite coordinate).  Asynchronous on the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _as_dev_f32(t, dev).contiguous()
    if t.dim() != 2:
        raise ValueError('logprior_gauss: t must be shaped [N, D], got %s' % (tuple(t.shape),))
    N, D = t.shape
    out = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        spec, keep = gauss_prior_spec(data, dev)
        _lib.check(_lib.load().nnest_logprior_gauss(ctypes.byref(spec), _lib.ptr(t), _lib.ptr(out), N, D, _lib.current_stream(dev)))
    return out


def _as_dev_f64(x, device):
    """a flat contiguous float64 tensor on `device` (a float64 tensor already there is used as it is)"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    return x.to(device=device, dtype=torch.float64).reshape(-1).contiguous()


def glm_curvature(data, theta, device=None):
    """the log-likelihood, its gradient and its negative Hessian at ONE theta for a regression likelihood of user data
    (nnest_glm_curv; include/nnest_hip.h has the arithmetic): data as `glm_spec` takes it, theta [D] (float64 on the device, or
    anything convertible).  Returns [1 + D + D D] float64 on the device: {logL (-1e100 where not finite), the gradient [D], the
    negative Hessian [D, D] row-major, bit-symmetric}.  Deterministic: the same call twice returns the same bits.  Asynchronous on
    the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    theta = _as_dev_f64(theta, dev)
    D = int(theta.shape[0])
    with torch.cuda.device(dev):
        spec, keep = glm_spec(data, dev)
        G = max(_lib.load().nnest_glm_curv_groups(max(int(spec.n), 1), max(D, 1)), 1)   # (-1: a shape the entry refuses first)
        out = torch.empty(1 + D + D * D, dtype=torch.float64, device=dev)
        partials = torch.empty(G * (1 + D + D * (D + 1) // 2), dtype=torch.float64, device=dev)
        _lib.check(_lib.load().nnest_glm_curv(ctypes.byref(spec), _lib.ptr(theta), _lib.ptr(out), _lib.ptr(partials), D,
                                              _lib.current_stream(dev)))
    return out


def glm_newton_solve(curv, theta, prior=None, device=None):
    """the Newton step of a regression posterior from `glm_curvature`'s result at theta (nnest_glm_newton_solve; include/nnest_hip.h
    has the arithmetic): prior None or as `gauss_prior_spec` takes it (the mapping priors.GaussianPrior.hip_gauss_prior holds).
    Returns (step [D], chol [D, D] the lower Cholesky factor of the negative Hessian of the log posterior, info [4] = {log L + log
    pi, the Newton decrement g^T step, log det, status}) float64 on the device; status 1: not positive definite, 2: a non-finite
    log L or log pi -- step and chol are zeros then.  Asynchronous on the current stream."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    theta = _as_dev_f64(theta, dev)
    curv = _as_dev_f64(curv, dev)
    D = int(theta.shape[0])
    if curv.shape[0] != 1 + D + D * D:
        raise ValueError('glm_newton_solve: curv must hold 1 + D + D D = %d values for theta [%d], got %d' % (1 + D + D * D, D, curv.shape[0]))
    with torch.cuda.device(dev):
        pspec, keep = gauss_prior_spec(prior, dev) if prior is not None else (None, None)
        step = torch.empty(D, dtype=torch.float64, device=dev)
        chol = torch.empty(D, D, dtype=torch.float64, device=dev)
        info = torch.empty(4, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().nnest_glm_newton_solve(_lib.ptr(curv), ctypes.byref(pspec) if pspec is not None else None, _lib.ptr(theta),
                                                      _lib.ptr(step), _lib.ptr(chol), _lib.ptr(info), D, _lib.current_stream(dev)))
    return step, chol, info


SMC_MAX_PARTICLES = 1 << 20   # the population nnest_smc_reweight and nnest_smc_resample take (one workgroup each)


def smc_reweight(logl, beta, ess_fraction):
    """the next temperature of a sequential Monte Carlo ladder and the weights that lead there (nnest_smc_reweight; include/nnest_hip.h
    has the definition): logl [N] float64 on the device (safe values), beta in [0, 1) the population's temperature, ess_fraction in
    (0, 1).  Returns (out, m): out [4] float64 on the device = {beta', log mean exp((beta' - beta) logL), ESS(beta'), max logL}, beta'
    where the effective sample size of w_i = exp((beta' - beta) (logL_i - max logL)) falls to ess_fraction * N (bisection; 1 where it
    never does), and m [N] int64 = floor(w_i 2^31), the integer weights smc_resample takes.  Deterministic: the same call twice
    returns the same bits.  Asynchronous on the current stream."""
    logl = torch.as_tensor(logl)
    if not logl.is_cuda:
        raise ValueError('smc_reweight: logl must be on the device')
    logl = logl.to(torch.float64).contiguous().reshape(-1)
    dev, N = logl.device, logl.shape[0]
    out = torch.empty(4, dtype=torch.float64, device=dev)
    m = torch.empty(N, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nnest_smc_reweight(_lib.ptr(logl), N, float(beta), float(ess_fraction), _lib.ptr(out), _lib.ptr(m),
                                                  _lib.current_stream(dev)))
    return out, m


def smc_resample(m, theta, logl, seed, stage):
    """systematic resampling of a population on integer weights (nnest_smc_resample; include/nnest_hip.h has the definition): m [N]
    int64 (>= 0, as smc_reweight returns them), theta [N, D] float32 and logl [N] float64 on the device; the one uniform of the draw
    is a function of (seed, stage) (Philox stream 8).  Returns (anc [N] int32, theta[anc], logl[anc]) as new tensors: anc_j is the
    smallest i whose inclusive prefix sum of m exceeds floor((j + u) sum(m) / N).  Returns after the kernel has finished; NnestHipError
    where the weights sum to 0."""
    m = torch.as_tensor(m)
    if not m.is_cuda:
        raise ValueError('smc_resample: m must be on the device')
    dev = m.device
    m = m.to(torch.int64).contiguous().reshape(-1)
    theta = _as_dev_f32(theta, dev).contiguous()
    logl = torch.as_tensor(logl, dtype=torch.float64).to(dev).contiguous().reshape(-1)
    N = m.shape[0]
    if theta.shape[0] != N or logl.shape[0] != N:
        raise ValueError('smc_resample: m [%d], theta %s and logl [%d]: one row per particle' % (N, tuple(theta.shape), logl.shape[0]))
    anc = torch.empty(N, dtype=torch.int32, device=dev)
    theta_out, logl_out = torch.empty_like(theta), torch.empty_like(logl)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nnest_smc_resample(_lib.ptr(m), N, theta.shape[1], int(seed) & 0xFFFFFFFFFFFFFFFF, int(stage), _lib.ptr(theta),
                                                  _lib.ptr(logl), _lib.ptr(anc), _lib.ptr(theta_out), _lib.ptr(logl_out),
                                                  _lib.current_stream(dev)))
    return anc, theta_out, logl_out


def importance_fill_noise(M, D, seed=0, sample_offset=0, device=None):
    """the draws of the fused importance-sampling kernels (nnest_importance_fill_noise), exported for the checker through the kernels'
    own function: z [M, D] float32, for samples sample_offset .. (flow-independent)"""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    z = torch.empty(int(M), int(D), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nnest_importance_fill_noise(_lib.ptr(z), int(M), int(D), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                           int(sample_offset) & 0xFFFFFFFFFFFFFFFF, _lib.current_stream(dev)))
    return z


def ensemble_x_max_walkers(D, like_id, device=None, moves=None):
    """the population ensemble_x_steps takes for x_dim D, this likelihood and these moves (every workgroup resident); 0 where it
    takes none"""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    mv = _lib.ens_moves(moves)
    with torch.cuda.device(device):
        if mv is None:
            return max(0, int(_lib.load().nnest_ensemble_x_max_walkers(int(D), int(like_id))))
        return max(0, int(_lib.load().nnest_ensemble_x_moves_max_walkers(int(D), int(like_id), _lib.moves_ref(mv))))


def ensemble_x_steps(like_id, x, steps, t_std=None, t_mean=None, lo=None, hi=None, lp=None, loglstar=None, seed=0, step0=0,
                     like_params=None, device=None, moves=None):
    """`steps` steps of emcee's stretch move in X space, in ONE launch (nnest_ensemble_x_steps: HipNVP.ensemble_steps' run with
    the identity for the flow; build-defined stream, emcee's move).  x [C, D] float32: the walkers' start (read only); lp [C]
    float64 or None (evaluated); the target is lp(x) = logL(T(x)) + prior with T(x) = x * t_std + t_mean (both None: the identity),
    the prior the box lo / hi [D] on T(x) (None: none); loglstar: None, or the hard constraint.  Returns x, tx (= T(x)), lp (the
    last state), hist_x [C, steps, D], hist_lp [C, steps] and n_accept [C].  Raises NnestHipError (code NNEST_E_UNSUPPORTED) when C
    exceeds ensemble_x_max_walkers.  moves: as HipNVP.ensemble_steps (nnest_ensemble_x_moves_steps)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    x = _as_dev_f32(x, dev).contiguous()
    (C, D), steps = x.shape, int(steps)
    mv = _lib.ens_moves(moves, 'ensemble_x_steps')
    _lib.ens_moves_mix(mv, C, 'ensemble_x_steps')
    f32 = dict(dtype=torch.float32, device=dev)
    t_std, t_mean, lo_t, hi_t = target_vectors('ensemble_x_steps', dev, t_std, t_mean, lo, hi, D=D)
    if lp is not None:
        lp = torch.as_tensor(lp, dtype=torch.float64).to(dev).contiguous()
    lib = _lib.load()
    out = dict(x=torch.empty(C, D, **f32), tx=torch.empty(C, D, **f32), lp=torch.empty(C, dtype=torch.float64, device=dev),
               hist_x=torch.empty(C, steps, D, **f32), hist_lp=torch.empty(C, steps, dtype=torch.float64, device=dev),
               n_accept=torch.empty(C, dtype=torch.int32, device=dev))
    words = lib.nnest_ensemble_work_words(C, steps)
    if words < 0:
        raise ValueError('ensemble_x_steps: %d walkers x %d steps: the work buffer is too large; launch fewer steps' % (C, steps))
    work = torch.empty(words, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        lk = _lib.like_spec(like_id, 1.0, like_params)
        fn = lib.nnest_ensemble_x_steps if mv is None else lib.nnest_ensemble_x_moves_steps
        _lib.check(fn(
            ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo_t), _lib.ptr(hi_t), _lib.ptr(x), _lib.ptr(lp),
            _lib.ptr(out['x']), _lib.ptr(out['tx']), _lib.ptr(out['lp']), _lib.ptr(out['hist_x']), _lib.ptr(out['hist_lp']),
            _lib.ptr(out['n_accept']), _lib.ptr(work), C, D, steps, int(step0) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF,
            0 if loglstar is None else 1, 0.0 if loglstar is None else float(loglstar), _lib.current_stream(dev),
            *(() if mv is None else (_lib.moves_ref(mv),))))
    return out
