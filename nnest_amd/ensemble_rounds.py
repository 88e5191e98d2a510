"""emcee's stretch move in latent space for ANY flow and ANY likelihood (include/nnest_hip.h nnest_ensemble_rounds_*).

BUILD-DEFINED STREAM, EMCEE'S MOVE: the definition is nnest_ensemble_steps's (the fused kernels of the default NVP shape and of
the spline flow, `ensemble_steps` of HipNVP / HipSpline), with the same draws, so the routes compute the same run.  Per half-step:

1. the propose kernel writes the moving set's proposals q, one row per walker in ascending walker order;
2. the flow's own `inverse` maps them (NVP of any shape, spline, MAF, Cholesky, fast/slow);
3. the likelihood runs on those rows: the device likelihood kernel (nnest_loglike) on T(x) for a known id, or else the caller's
   callables on the host;
4. the accept kernel applies the rule and writes the step's history rows.

With `moves` the run mixes the stretch move with emcee's differential-evolution move, one move per step by weight
(nnest_ensemble_rounds_moves_*; the definition: include/nnest_hip.h nnest_ensemble_moves_steps): on a DE step the propose kernel
writes the DE proposal and the accept kernel applies the rule without the stretch factor.
"""
import numpy as np
import torch

from . import _lib
from . import flow as _flow
from .device_target import affine_on_device


def work_buffer(lib, C, steps, dev):
    words = lib.nnest_ensemble_work_words(int(C), int(steps))
    if words < 0:
        raise ValueError('ensemble: %d walkers x %d steps: the work buffer is too large; use fewer steps per launch' % (C, steps))
    return torch.empty(words, dtype=torch.int32, device=dev)


def fill_noise(C, steps, seed=0, step0=0, device=None):
    """the draws of steps step0 .. step0 + steps - 1 (nnest_ensemble_fill_noise), exported for the checker: inds [steps, C] int32
    (the split: 0 = set 0) and u [steps, C, 3] float32 (u1, u2, u3)"""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    with torch.cuda.device(dev):
        work = work_buffer(lib, C, steps, dev)
        u = torch.empty(steps, C, 3, dtype=torch.float32, device=dev)
        _lib.check(lib.nnest_ensemble_fill_noise(_lib.ptr(work), _lib.ptr(u), int(C), int(steps), int(step0) & 0xFFFFFFFFFFFFFFFF,
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.current_stream(dev)))
        off = lib.nnest_ensemble_work_words(int(C), 0)
        inds = work[off:off + steps * C].reshape(steps, C).clone()
    return inds, u


def fill_moves(C, D, steps, moves=None, seed=0, step0=0, device=None):
    """the moves' draws of steps step0 .. step0 + steps - 1 (nnest_ensemble_fill_moves), exported for the checker beside
    fill_noise's: move [steps] int32 (0: a stretch step, 1: a DE step), jb [steps, C] int32 (the DE step's second partner, an
    index into the other set's members in ascending walker order, already shifted past the first partner's) and gamma
    [steps, C] float32 (the DE scale).  moves: {'stretch': w, 'de': w} (None: every step a stretch step)"""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    mv = _lib.ens_moves(moves, 'fill_moves')
    seed, step0 = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0) & 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(dev):
        sp = _lib.current_stream(dev)
        work = work_buffer(lib, C, steps, dev)
        _lib.check(lib.nnest_ensemble_fill_noise(_lib.ptr(work), None, int(C), int(steps), step0, seed, sp))
        move = torch.empty(steps, dtype=torch.int32, device=dev)
        jb = torch.empty(steps, C, dtype=torch.int32, device=dev)
        gamma = torch.empty(steps, C, dtype=torch.float32, device=dev)
        _lib.check(lib.nnest_ensemble_fill_moves(_lib.ptr(work), _lib.ptr(move), _lib.ptr(jb), _lib.ptr(gamma), int(C), int(D), int(steps),
                                                 step0, seed, _lib.moves_ref(mv), sp))
    return move, jb, gamma


class IdentityFlow(object):
    """the identity as a flow, for the stretch move in x space on the round route: inverse(z) -> (z, zeros)"""

    def __init__(self, device=None):
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def inverse(self, z):
        return z, torch.zeros(z.shape[0], dtype=torch.float32, device=z.device)


class EnsembleState(object):
    """the walkers between launches: z, x [C, D] float32, lp [C] float64, n_accept [C] int32 (device), derived [C, nd] (host)"""

    def __init__(self, z, x, lp, n_accept, derived=None):
        self.z, self.x, self.lp, self.n_accept, self.derived = z, x, lp, n_accept, derived


def ensemble_rounds(flow, z, steps, state=None, lp=None, t_std=None, t_mean=None, lo=None, hi=None, like_id=None, like_params=None,
                    loglike=None, prior=None, num_derived=0, init_derived=None, loglstar=None, seed=0, step0=0, moves=None):
    """`steps` steps of the stretch move (moves=None), or of a mixture {'stretch': w, 'de': w} with emcee's DE move (_lib.ens_moves),
    global steps step0 .. step0 + steps - 1.

    flow: any object with inverse(z) -> (x, log|det dx/dz|) on the device and a `device`.
    Start: `state` (an EnsembleState from the previous call), else z [C, D] with lp [C] (None: evaluated here, C likelihood calls).
    The likelihood, exactly one of:
      like_id (with like_params): the device likelihood of T(x) = x * t_std + t_mean (float32), the prior the box [lo, hi] on T(x)
          (lo = hi = None: none);
      loglike(x [n, D] float32 numpy) -> (logl [n], derived [n, num_derived]) with the transform inside (Sampler.loglike: safe,
          counts its calls), and prior(x [n, D]) -> log prior [n] (Sampler.prior; None: 0).  With loglstar set the derived
          parameters of the accepted proposals are carried; without, they are zeros, as the reference's (sampler.py:687).
    Returns (state, hist) with hist = dict(hist_z, hist_x [C, steps, D], hist_lp [C, steps] device tensors, hist_derived
    [C, steps, nd] numpy)."""
    if (loglike is None) == (like_id is None):
        raise ValueError('ensemble_rounds: give exactly one of loglike (host callable) and like_id (device likelihood)')
    dev = flow.device
    lib = _lib.load()
    mv = _lib.ens_moves(moves, 'ensemble_rounds')
    steps, nd = int(steps), int(num_derived)
    constrained = 0 if loglstar is None else 1
    star = 0.0 if loglstar is None else float(loglstar)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    step0 = int(step0) & 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        sp = _lib.current_stream(dev)
        if state is not None:
            C, D = state.z.shape
        else:
            z = _flow._as_dev_f32(z, dev).contiguous()
            C, D = z.shape
        _lib.ens_moves_mix(mv, C, 'ensemble_rounds')
        # (moves=None: the stretch move's own entries, which are the moves entries with NULL)
        propose_fn = lib.nnest_ensemble_rounds_propose if mv is None else lib.nnest_ensemble_rounds_moves_propose
        accept_fn = lib.nnest_ensemble_rounds_accept if mv is None else lib.nnest_ensemble_rounds_moves_accept
        mv_arg = () if mv is None else (_lib.moves_ref(mv),)
        t_std_t = t_mean_t = lo_t = hi_t = None
        if like_id is not None:
            t_std_t, t_mean_t, lo_t, hi_t = _flow.target_vectors('ensemble_rounds', dev, t_std, t_mean, lo, hi, D=D, identity=True)
        work = work_buffer(lib, C, steps, dev)
        _lib.check(lib.nnest_ensemble_fill_noise(_lib.ptr(work), None, C, steps, step0, seed, sp))

        def evaluate(q, n):
            """x, ld, logl, lprior (device) and derived (host) of the rows q[:n]"""
            x, ld = flow.inverse(q[:n])
            if like_id is not None:
                return x, ld, _flow.loglike(like_id, affine_on_device(x, t_std_t, t_mean_t), 1.0, device=dev, like_params=like_params), None, None
            xh = x.cpu().numpy()
            out = loglike(xh)
            lv, dv = out if isinstance(out, tuple) else (out, None)
            lv = np.array(lv, dtype=np.float64, ndmin=1).reshape(n)
            lv[~np.isfinite(lv)] = -1e100
            lpr = np.zeros(n) if prior is None else np.asarray(prior(xh), dtype=np.float64).reshape(n)
            dv = np.zeros((n, nd)) if dv is None or nd == 0 else np.asarray(dv, dtype=np.float64).reshape(n, nd)
            return (x, ld, torch.from_numpy(lv).to(dev), torch.from_numpy(np.ascontiguousarray(lpr)).to(dev), dv)

        def accept(i, half, q, x, ld, logl, lprior, st, hist, acc_rows=None):
            _lib.check(accept_fn(
                _lib.ptr(work), C, steps, D, i, half, step0, seed, _lib.ptr(q), _lib.ptr(x), _lib.ptr(ld), _lib.ptr(logl),
                _lib.ptr(lprior), _lib.ptr(t_std_t), _lib.ptr(t_mean_t), _lib.ptr(lo_t), _lib.ptr(hi_t), _lib.ptr(st.z), _lib.ptr(st.x),
                _lib.ptr(st.lp), _lib.ptr(hist.get('hist_z')), _lib.ptr(hist.get('hist_x')), _lib.ptr(hist.get('hist_lp')),
                _lib.ptr(st.n_accept), _lib.ptr(acc_rows), constrained, star, sp, *mv_arg))

        if state is None:
            st = EnsembleState(z.clone(), torch.empty_like(z), torch.empty(C, dtype=torch.float64, device=dev),
                               torch.zeros(C, dtype=torch.int32, device=dev))
            if lp is None:   # the initial evaluation: every walker is a row (C likelihood calls)
                x, ld, logl, lprior, dv = evaluate(z, C)
                accept(0, -1, z, x, ld, logl, lprior, st, {})
                st.derived = dv if constrained else np.zeros((C, nd))
            else:
                st.x.copy_(flow.inverse(z)[0])
                st.lp.copy_(torch.as_tensor(lp, dtype=torch.float64).to(dev))
                st.derived = (np.zeros((C, nd)) if init_derived is None or not constrained
                              else np.array(init_derived, dtype=np.float64).reshape(C, nd))
        else:
            st = state
            if st.derived is None:
                st.derived = np.zeros((C, nd))
        f32 = dict(dtype=torch.float32, device=dev)
        hist = dict(hist_z=torch.empty(C, steps, D, **f32), hist_x=torch.empty(C, steps, D, **f32),
                    hist_lp=torch.empty(C, steps, dtype=torch.float64, device=dev))
        hist_derived = np.zeros((C, steps, nd))
        n0 = (C + 1) // 2
        q = torch.empty(n0, D, **f32)
        acc = torch.empty(n0, dtype=torch.int32, device=dev) if (nd and constrained and loglike is not None) else None
        off = lib.nnest_ensemble_work_words(C, 0) + steps * C
        members = work[off:off + steps * C].reshape(steps, C) if acc is not None else None
        for i in range(steps):
            for half in (0, 1):
                n = n0 if half == 0 else C - n0
                _lib.check(propose_fn(_lib.ptr(work), C, steps, D, i, half, step0, seed, _lib.ptr(st.z), _lib.ptr(q), sp, *mv_arg))
                x, ld, logl, lprior, dv = evaluate(q, n)
                accept(i, half, q, x, ld, logl, lprior, st, hist, acc)
                if acc is not None:   # the derived parameters of the accepted proposals (host)
                    stream.synchronize()
                    taken = acc[:n].cpu().numpy() != 0
                    who = members[i, (0 if half == 0 else n0):(n0 if half == 0 else C)].cpu().numpy()
                    st.derived[who[taken]] = dv[taken]
            if nd:
                hist_derived[:, i] = st.derived
    hist['hist_derived'] = hist_derived
    return st, hist
