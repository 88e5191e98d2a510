"""The slice proposal in latent space for ANY flow and ANY likelihood (include/nnest_hip.h nnest_slice_rounds_*).

BUILD-DEFINED, parity unpinned: the reference proposes random-walk Metropolis moves only (nnest/sampler.py:310-316).  The definition
is nnest_slice_steps's -- the fused kernels of the default NVP (HipNVP.slice_steps) and of the spline flow (HipSpline.slice_steps)
keep running where they apply.  Here each walker's slice state machine lives on the device and advances in rounds; per round:

1. the flow's own `inverse` maps every walker's candidate (NVP of any shape, spline, MAF, Cholesky, fast/slow);
2. a screen kernel tests the box and the slice level and packs the rows that need a likelihood, in ascending walker order;
3. the likelihood is evaluated on those rows only: a host callable, the device likelihood kernel (nnest_loglike) for a known id, or
   the regression likelihood of user data on the device (nnest_loglike_glm on T(rows)) for a `like_glm`;
4. an advance kernel consumes the results and writes the next candidates.

One small device-to-host copy per round tells the host how many rows to evaluate and whether any walker is still live.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import flow as _flow
from .device_target import affine_on_device

_HANDLES = {}
_MAX_HANDLES = 4


class _Handle(object):
    """nnest_slice_rounds_t for (C, D, steps) plus the round buffers; kept per (device, stream, C, D, steps) for reuse"""

    def __init__(self, lib, dev, C, D, steps):
        self.lib = lib
        self.h = ctypes.c_void_p()
        _lib.check(lib.nnest_slice_rounds_create(C, D, steps, ctypes.byref(self.h)))
        f32 = dict(dtype=torch.float32, device=dev)
        self.z_cand = torch.empty(C, D, **f32)
        self.rows = torch.empty(C, D, **f32)
        self.idx = torch.empty(C, dtype=torch.int32, device=dev)
        self.counts = torch.empty(2, dtype=torch.int32, device=dev)
        self.logl_rows = torch.empty(C, dtype=torch.float64, device=dev)
        self.inbox = torch.empty(C, dtype=torch.int32, device=dev)
        # one pinned host buffer per direction: counts + rows device -> host, likelihoods / prior flags host -> device
        self.down = torch.empty(2 + C * D, dtype=torch.float32).pin_memory()
        self.up = torch.empty(C, dtype=torch.float64).pin_memory()

    def __del__(self):
        try:
            if self.h.value:
                self.lib.nnest_slice_rounds_destroy(self.h)
                self.h = ctypes.c_void_p()
        except Exception:
            pass


def _handle(lib, dev, C, D, steps):
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, C, D, steps)
    h = _HANDLES.get(key)
    if h is None:
        if len(_HANDLES) >= _MAX_HANDLES:
            torch.cuda.synchronize(dev)   # (an evicted handle may still be read by queued work of its stream)
            _HANDLES.pop(next(iter(_HANDLES)))
        h = _HANDLES[key] = _Handle(lib, dev, C, D, steps)
    return h


def slice_rounds(flow, z, logl, loglstar, width, steps, loglike=None, like_id=None, like_scale=1.0, like_params=None, prior=None,
                 num_derived=0, init_derived=None, max_stepout=8, max_shrink=32, noise=None, seed=0, walker_offset=0, history=False,
                 like_glm=None, t_std=None, t_mean=None):
    """`steps` slice-sampling updates of every walker (stepping out + shrinkage along a random direction of latent space) under the
    hard constraint logL > loglstar, of the target |det dx/dz| on {x(z) in the prior, logL(x(z)) > loglstar}.  With a fast/slow flow
    the directions span all coordinates (there are no fast-only updates).

    flow: any object with inverse(z) -> (x, log|det dx/dz|) on the device and a `device`.
    z [C, D] float32 and logl [C] float64 (device tensors) are updated in place.
    The likelihood, exactly one of:
      loglike(x [n, D] float32 numpy) -> logl [n] (or (logl, derived [n, num_derived])), called only on the rows whose likelihood
          decides (never with zero rows); non-finite values count as -1e100;
      like_id (NNEST_LIKE_*, with like_scale / like_params): the device likelihood kernel, the rows never leave the device;
      like_glm (the descriptor of a regression likelihood of user data, likelihoods.GLMData.hip_like_glm): logL = GLM(T(row)) with
          T(x) = x * t_std + t_mean per dimension in float32 (affine_on_device; t_std / t_mean [D], both or neither, None: the
          identity) through flow.loglike_glm, the rows never leave the device -- the definition of nnest_slice_glm_steps for the
          flows and shapes its kernels do not take.  The box stays on x.
    prior: None = the unit box on the device; else a host callable x [C, D] -> bool [C] (inside the prior) applied to every candidate
        in place of the box (host-callable route only; every candidate row is copied back for it).
    init_derived [C, num_derived]: the starting points' derived parameters (host-callable route).
    noise: recorded directions dz [steps, C, D] (fill_slice_noise exports the in-kernel ones for (seed, walker_offset)).
    Returns x, n_call (rows evaluated), n_move, moved (every coordinate of x changed: nested.py:432), n_eval (candidates), hist_x,
    plus hist_z, hist_logl (history=True), derived [C, num_derived] and hist_derived (numpy; None without num_derived), rounds."""
    if (loglike is not None) + (like_id is not None) + (like_glm is not None) != 1:
        raise ValueError('slice_rounds: give exactly one of loglike (host callable), like_id (device likelihood) and like_glm (regression '
                         'likelihood of user data on the device)')
    on_device = like_id is not None or like_glm is not None
    if on_device and (prior is not None or num_derived):
        raise ValueError('slice_rounds: the device likelihood runs in the unit box without derived parameters')
    if like_glm is None and (t_std is not None or t_mean is not None):
        raise ValueError('slice_rounds: t_std and t_mean go only with a like_glm')
    assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.dim() == 2
    assert logl.is_cuda and logl.dtype == torch.float64 and logl.is_contiguous()
    dev = z.device
    C, D = z.shape
    steps = int(steps)
    nd = int(num_derived)
    lib = _lib.load()
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        sp = _lib.current_stream(dev)
        h = _handle(lib, dev, C, D, steps)
        if like_glm is not None:   # (staged once for the batch's rounds)
            t_std, t_mean, _, _ = _flow.target_vectors('slice_rounds', dev, t_std, t_mean, None, None, D=D)
            _, (at, y, o) = _flow.glm_spec(like_glm, dev)
            like_glm = dict(like_glm, at=at, y=y, o=o)
        x0, ld0 = flow.inverse(z)
        hx = torch.empty(C, steps + 1, D, dtype=torch.float32, device=dev) if history else None
        hz = torch.empty(C, steps + 1, D, dtype=torch.float32, device=dev) if history else None
        hl = torch.empty(C, steps + 1, dtype=torch.float64, device=dev) if history else None
        mref = torch.empty(C, steps, **i32) if nd else None
        dz = None
        if noise is not None:
            dz = noise.reshape(steps * C, D)
            assert dz.is_cuda and dz.dtype == torch.float32 and dz.is_contiguous()
        _lib.check(lib.nnest_slice_rounds_begin(h.h, _lib.ptr(z), _lib.ptr(x0), _lib.ptr(ld0), _lib.ptr(logl), float(loglstar),
                                                float(width), int(max_stepout), int(max_shrink), _lib.ptr(dz),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(walker_offset), _lib.ptr(hx), _lib.ptr(hz),
                                                _lib.ptr(hl), _lib.ptr(mref), _lib.ptr(h.z_cand), sp))
        counts_host = h.down[:2].view(torch.int32)
        derived_rounds = []
        rounds = 0
        while True:
            xc, ldc = flow.inverse(h.z_cand)
            inbox = None
            if prior is not None:   # the caller's prior on every candidate, in place of the box
                xh = h.down[2:2 + C * D].view(C, D)
                xh.copy_(xc, non_blocking=True)
                stream.synchronize()
                ok = np.asarray(prior(xh.numpy().copy()), dtype=bool).reshape(C)
                up = h.up[:C].view(torch.int32)[:C]
                up.numpy()[:] = ok
                inbox = h.inbox
                inbox.copy_(up, non_blocking=True)
            _lib.check(lib.nnest_slice_rounds_screen(h.h, _lib.ptr(xc), _lib.ptr(ldc), _lib.ptr(inbox), _lib.ptr(h.rows),
                                                     _lib.ptr(h.idx), _lib.ptr(h.counts), sp))
            counts_host.copy_(h.counts, non_blocking=True)
            stream.synchronize()
            n_rows, n_live = int(counts_host[0]), int(counts_host[1])
            if n_live == 0:
                break
            rounds += 1
            lrows = h.logl_rows
            if n_rows and like_id is not None:
                lrows = _flow.loglike(like_id, h.rows[:n_rows], like_scale, device=dev, like_params=like_params)
            elif n_rows and like_glm is not None:
                rows = h.rows[:n_rows]
                lrows = _flow.loglike_glm(like_glm, rows if t_std is None else affine_on_device(rows, t_std, t_mean), device=dev)
            elif n_rows:
                xr = h.down[2:2 + n_rows * D].view(n_rows, D)
                xr.copy_(h.rows[:n_rows], non_blocking=True)
                stream.synchronize()
                out = loglike(xr.numpy().copy())
                lv, dv = out if isinstance(out, tuple) else (out, None)
                lv = np.array(lv, dtype=np.float64, ndmin=1).reshape(n_rows)
                lv[~np.isfinite(lv)] = -1e100
                if nd:
                    derived_rounds.append(np.asarray(dv, dtype=np.float64).reshape(n_rows, nd))
                up = h.up[:n_rows]
                up.numpy()[:] = lv
                lrows.narrow(0, 0, n_rows).copy_(up, non_blocking=True)
            _lib.check(lib.nnest_slice_rounds_advance(h.h, _lib.ptr(h.rows), _lib.ptr(lrows), _lib.ptr(h.z_cand), sp))
        x = torch.empty_like(z)
        n_call = torch.empty(C, **i32)
        n_move = torch.empty(C, **i32)
        n_eval = torch.empty(C, **i32)
        _lib.check(lib.nnest_slice_rounds_finish(h.h, _lib.ptr(z), _lib.ptr(x), _lib.ptr(logl), _lib.ptr(n_call), _lib.ptr(n_move),
                                                 _lib.ptr(n_eval), sp))
    derived = hist_derived = None
    if nd:
        cur = np.array(init_derived, dtype=np.float64).reshape(C, nd) if init_derived is not None else np.full((C, nd), np.nan)
        every = np.concatenate(derived_rounds) if derived_rounds else np.empty((0, nd))
        ref = mref.cpu().numpy()
        hist_derived = np.empty((C, steps + 1, nd))
        hist_derived[:, 0] = cur
        for it in range(steps):
            sel = ref[:, it] >= 0
            cur[sel] = every[ref[sel, it]]
            hist_derived[:, it + 1] = cur
        derived = cur
    n_move, moved = _flow.split_move_word(n_move)
    return dict(x=x, n_call=n_call, n_move=n_move, moved=moved, n_eval=n_eval, hist_x=hx, hist_z=hz, hist_logl=hl, derived=derived,
                hist_derived=hist_derived, rounds=rounds)
