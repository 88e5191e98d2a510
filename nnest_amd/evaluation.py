"""Chain statistics on the GPU: the reference's nnest/utils/evaluation.py (acceptance rate, mean jump distance, lag autocorrelation,
effective sample size, Gelman-Rubin R-hat) over a batch of chains x [C, T, D], computed by the HIP kernels behind
include/nnest_hip.h nnest_chain_stats*.  The inputs are numpy arrays (copied to the device as float32) or CUDA tensors (read in place
through their chain and step strides when float32 with a unit dimension stride).  The definitions, the reference's quirks included
(the autocorrelation divided by the standard deviation; the ESS sum stopped globally over the dimensions), are in the header.
There is no CPU path: without a GPU these raise NnestHipError."""

import logging

import numpy as np
import torch

from . import _lib
from ._lib import NnestHipError

LAG_BLOCK = 256


def _device_chains(x):
    """x [C, T, D] -> (float32 CUDA tensor with unit dimension stride, chain stride, step stride); views of a CUDA tensor in place"""
    if not torch.cuda.is_available():
        raise NnestHipError('chain statistics run on the GPU (HIP); no device is available and there is no CPU fallback')
    if isinstance(x, torch.Tensor):
        t = x.detach()
        if not t.is_cuda:
            t = t.cuda()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).cuda()
    if t.dim() != 3:
        raise ValueError('chains must be shaped [C, T, D], got %s' % (tuple(t.shape),))
    if t.dtype != torch.float32 or t.stride(2) != 1:
        t = t.float().contiguous()
    return t, t.stride(0), t.stride(1)


def _vec(v, D, device):
    if v is None:
        return None
    a = torch.as_tensor(np.broadcast_to(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64), (D,)).copy())
    return a.to(device)


def _affine(affine, D, device):
    """affine = (a, b): T(x) = x * a + b per dimension -> [2, D] float64 on the device"""
    if affine is None:
        return None
    a, b = affine
    return torch.cat([_vec(a, D, device), _vec(b, D, device)]).contiguous()


def chain_stats(x, mean=None, std=None, affine=None, all_lags=False, return_p=False, ess=True, rhat_at_mean=False):
    """All the statistics of chains x [C, T, D] from one pass: a dict with acceptance, jump_distance (floats), ess, rhat (None for
    one chain), mean, std ([D] float64 numpy), stop_lag (the lag at which the ESS sum stopped, T if it never did) and, with
    return_p, p [T - 1, D] (the lag autocorrelations; NaN in the rows of lags not computed).  mean / std: those of
    Sampler._chain_stats (default: over all C T rows); affine: (a, b), the statistics of x * a + b, computed without a copy;
    all_lags: compute every lag, not only those up to the stop; ess=False: skip the lags; rhat_at_mean: R-hat about `mean`
    (gelman_rubin_diagnostic(x, mu))."""
    t, cs, ss = _device_chains(x)
    C, T, D = t.shape
    dev = t.device
    lib = _lib.load()
    words = lib.nnest_chain_stats_work_words(C, T, D)
    if words < 0:
        raise ValueError('chain_stats: unsupported shape C=%d T=%d D=%d (C >= 1, T >= 2, D >= 1)' % (C, T, D))
    flags = ((_lib.CHAIN_STATS_ALL_LAGS if all_lags else 0) | (0 if ess else _lib.CHAIN_STATS_NO_ESS)
             | (_lib.CHAIN_STATS_RHAT_AT_MEAN if rhat_at_mean else 0))
    with torch.cuda.device(dev):
        mu, sd, aff = _vec(mean, D, dev), _vec(std, D, dev), _affine(affine, D, dev)
        work = torch.empty(words, dtype=torch.float64, device=dev)
        out = torch.empty(4 + 4 * D, dtype=torch.float64, device=dev)
        p = torch.full((T - 1, D), float('nan'), dtype=torch.float64, device=dev) if return_p else None
        _lib.check(lib.nnest_chain_stats(_lib.ptr(t), C, T, D, cs, ss, _lib.ptr(aff), _lib.ptr(mu), _lib.ptr(sd), flags,
                                         _lib.ptr(work), _lib.ptr(p), _lib.ptr(out), _lib.current_stream(dev)))
        o = out.cpu().numpy()
    res = dict(acceptance=float(o[0]), jump_distance=float(o[1]), stop_lag=None if np.isnan(o[2]) else int(o[2]),
               ess=o[4:4 + D].copy() if ess else None, rhat=o[4 + D:4 + 2 * D].copy() if C > 1 else None,
               mean=o[4 + 2 * D:4 + 3 * D].copy(), std=o[4 + 3 * D:4 + 4 * D].copy())
    if return_p:
        res['p'] = p.cpu().numpy()
    return res


class ShardedChainStats(object):
    """The stages of include/nnest_hip.h for one shard of a batch whose chains are split over ranks: the chain sums and the lag
    sums are additive, so `allreduce` (a callable summing a float64 CUDA tensor over the ranks in place) between the stages gives
    every rank the statistics of the whole batch.  mean and std are required (the moments of the whole batch would need one
    more round)."""

    def __init__(self, allreduce):
        self.allreduce = allreduce

    def __call__(self, x, mean, std, affine=None):
        """(acceptance, ESS [D], jump distance) of the whole batch; x [C_local, T, D] may hold no chains (C_local = 0)"""
        t, cs, ss = _device_chains(x)
        C, T, D = t.shape
        dev = t.device
        lib = _lib.load()
        st = _lib.current_stream(dev)
        with torch.cuda.device(dev):
            work = torch.empty(lib.nnest_chain_stats_work_words(max(C, 1), T, D), dtype=torch.float64, device=dev)
            sums = torch.zeros(3 + 3 * D, dtype=torch.float64, device=dev)
            mu, sd, aff = _vec(mean, D, dev), _vec(std, D, dev), _affine(affine, D, dev)
            if C > 0:
                _lib.check(lib.nnest_chain_stats_chains(_lib.ptr(t), C, T, D, cs, ss, _lib.ptr(aff), _lib.ptr(mu), _lib.ptr(work),
                                                        _lib.ptr(sums), st))
            self.allreduce(sums)
            Cw = max(C, 1)   # (the work layout of an empty shard)
            _lib.check(lib.nnest_chain_stats_prepare(_lib.ptr(sums), Cw, T, D, _lib.ptr(mu), _lib.ptr(sd), _lib.ptr(work), st))
            lag_sums = torch.zeros((LAG_BLOCK, D), dtype=torch.float64, device=dev)
            for lag0 in range(1, T, LAG_BLOCK):
                if C > 0:
                    _lib.check(lib.nnest_chain_stats_lags(_lib.ptr(t), C, T, D, cs, ss, _lib.ptr(aff), lag0, LAG_BLOCK, 0, _lib.ptr(work),
                                                          _lib.ptr(lag_sums), st))
                self.allreduce(lag_sums)
                _lib.check(lib.nnest_chain_stats_advance(_lib.ptr(sums), _lib.ptr(lag_sums), Cw, T, D, lag0, LAG_BLOCK, 0, _lib.ptr(work),
                                                         None, st))
            out = torch.empty(4 + 4 * D, dtype=torch.float64, device=dev)
            _lib.check(lib.nnest_chain_stats_finish(_lib.ptr(sums), Cw, T, D, 0, _lib.ptr(work), _lib.ptr(out), st))
            o = out.cpu().numpy()
        return float(o[0]), o[4:4 + D].copy(), float(o[1])


# ---- emcee's integrated autocorrelation time (emcee 3 autocorr.integrated_time, has_walkers=True), restated ------------------------
class AutocorrError(Exception):
    """the chain is shorter than `tol` autocorrelation times: `tau` [D] is the estimate, `thresh` the chain length each one
    would need over tol (emcee's AutocorrError carries the same two)"""

    def __init__(self, tau, thresh, *args):
        self.tau, self.thresh = tau, thresh
        super(AutocorrError, self).__init__(*args)


def autocorr_function(x):
    """f [T, D] float64 (device): f(s) = mean_k acf_k(s) / acf_k(0) over the walkers of x [C, T, D], every lag, each walker
    centred on its own mean (include/nnest_hip.h nnest_chain_autocorr)"""
    t, cs, ss = _device_chains(x)
    C, T, D = t.shape
    dev = t.device
    lib = _lib.load()
    words = lib.nnest_chain_autocorr_work_words(C, T, D)
    if words < 0:
        raise ValueError('autocorr_function: unsupported shape C=%d T=%d D=%d (C >= 1, T >= 2, D >= 1)' % (C, T, D))
    with torch.cuda.device(dev):
        work = torch.empty(words, dtype=torch.float64, device=dev)
        f = torch.empty(T, D, dtype=torch.float64, device=dev)
        _lib.check(lib.nnest_chain_autocorr(_lib.ptr(t), C, T, D, cs, ss, _lib.ptr(work), _lib.ptr(f), _lib.current_stream(dev)))
    return f / C


def integrated_autocorr_time(x, c=5, tol=50, quiet=False, return_window=False):
    """emcee's integrated autocorrelation time tau [D] of walkers x [C, T, D]: taus = 2 cumsum(f) - 1 with f = autocorr_function,
    cut at Sokal's window: with m = arange(T) < c * taus, argmin(m) if any entry of m is true, else T - 1 (so an all-true m gives
    window 0, as emcee's auto_window does).  This is NOT auto_correlation_time / effective_sample_size below (the reference's own
    estimator: global mean, divided by the standard deviation, stopped globally).  If tol * tau > T for any dimension the chain
    is too short for the estimate: AutocorrError (with tau and thresh), or a warning and the estimate when `quiet`.  The lag sums
    run on the GPU; the cumulative sum and the window are torch on the [T, D] table."""
    f = autocorr_function(x)
    T, D = f.shape
    taus = 2.0 * torch.cumsum(f, dim=0) - 1.0
    m = torch.arange(T, device=f.device, dtype=torch.float64)[:, None] < float(c) * taus
    window = torch.where(m.any(dim=0), torch.argmin(m.to(torch.int8), dim=0), torch.full((D,), T - 1, device=f.device))
    tau = taus.gather(0, window[None, :])[0].cpu().numpy()
    window = window.cpu().numpy()
    flag = tol * tau > T
    if np.any(flag) and tol > 0:
        msg = ('The chain is shorter than %d times the integrated autocorrelation time for %d parameter(s). Use this estimate with '
               'caution and run a longer chain!\nN/%d = %.0f;\ntau: %s' % (tol, int(np.sum(flag)), tol, T / tol, tau))
        if not quiet:
            raise AutocorrError(tau, T / tol, msg)
        import logging
        logging.getLogger(__name__).warning(msg)
    return (tau, window) if return_window else tau


# ---- the reference's functions (nnest/utils/evaluation.py), same names and signatures ----------------------------------------
def auto_correlation_time(x, s, mu, var):
    """p_s [D]: (1 / C) sum_i mean_j (x_ij - mu)(x_i,j+s - mu) / var  (evaluation.py:6-14; `var` as the reference divides by it)"""
    T = x.shape[1]
    if not 1 <= s < T:
        raise ValueError('lag s=%d outside 1..T-1 = %d' % (s, T - 1))
    return chain_stats(x, mean=mu, std=var, all_lags=True, return_p=True)['p'][s - 1]


def effective_sample_size(x, mu, var):
    """evaluation.py:17-41"""
    return chain_stats(x, mean=mu, std=var)['ess']


def acceptance_rate(x):
    """evaluation.py:44-58"""
    return chain_stats(x, ess=False)['acceptance']


def mean_jump_distance(x):
    """evaluation.py:61-74"""
    return chain_stats(x, ess=False)['jump_distance']


def gelman_rubin_diagnostic(x, mu=None):
    """evaluation.py:77-93 (one chain divides by C - 1 = 0, as in the reference)"""
    if x.shape[0] < 2:
        raise ZeroDivisionError('gelman_rubin_diagnostic: one chain (B divides by C - 1)')
    return chain_stats(x, mean=mu, ess=False, rhat_at_mean=mu is not None)['rhat']


def predictive_criteria(like, samples, route=None, psis=False):
    """The predictive model-comparison criteria of a regression posterior (build-defined: the reference has none) -- the other half
    of model comparison beside the evidence.  like: a likelihoods.GLMData; samples: [S, x_dim] or [N, steps, x_dim] posterior draws
    theta (unweighted); route: None, 'host' or 'fused', as GLMData.pointwise takes it (the 'host' route needs no GPU).
    Returns a dict: the totals over the n data rows elpd_waic, p_waic, lppd, elpd_isloo; their standard errors elpd_waic_se,
    p_waic_se, lppd_se, elpd_isloo_se = sqrt(n var_i) of the pointwise values (n - 1 in the divisor; NaN for one row);
    min_isloo_ess, the smallest per-row effective sample size of the leave-one-out weights; pointwise, GLMData.pointwise's dict;
    n_samples; route.  elpd_isloo is PLAIN importance-sampled leave-one-out, without Pareto smoothing: where min_isloo_ess is small
    (a handful of draws) it is unreliable and too optimistic -- prefer elpd_waic there, or more draws.  psis=True adds Pareto-smoothed
    leave-one-out (GLMData.pointwise has it): the totals elpd_psis, elpd_psis_se and p_loo; max_pareto_k, the largest fitted shape
    (NaN and +inf -- no fit -- aside); n_pareto_k_bad, the rows whose khat is above loo's threshold min(1 - 1 / log10(S), 0.7) and
    whose elpd_psis is therefore unreliable; pareto_k_threshold.  Logs one line."""
    pw = like.pointwise(samples, route=route, psis=True) if psis else like.pointwise(samples, route=route)
    n = len(pw['lppd'])
    out = {}
    with np.errstate(invalid='ignore'):
        for k in ('elpd_waic', 'p_waic', 'lppd', 'elpd_isloo'):
            out[k] = float(np.sum(pw[k]))
            out[k + '_se'] = float(np.sqrt(n * np.var(pw[k], ddof=1))) if n > 1 else float('nan')
    out['min_isloo_ess'] = float(np.min(pw['isloo_ess']))
    out['pointwise'] = pw
    out['n_samples'] = int(np.prod(np.shape(samples)[:-1]))
    out['route'] = like.pointwise_route
    extra = ''
    if psis:
        from .psis import pareto_k_threshold
        with np.errstate(invalid='ignore'):
            out['elpd_psis'] = float(np.sum(pw['elpd_psis']))
            out['elpd_psis_se'] = float(np.sqrt(n * np.var(pw['elpd_psis'], ddof=1))) if n > 1 else float('nan')
            out['p_loo'] = float(np.sum(pw['p_loo']))
            k = pw['pareto_k']
            fitted = k[np.isfinite(k)]
            out['max_pareto_k'] = float(np.max(fitted)) if len(fitted) else float('nan')
            out['pareto_k_threshold'] = pareto_k_threshold(out['n_samples'])
            out['n_pareto_k_bad'] = int(np.sum(fitted > out['pareto_k_threshold']))
        extra = ' elpd_psis [%5.4f +- %5.4f] p_loo [%5.4f] max Pareto k [%.3f] rows above %.2f [%d]' % (
            out['elpd_psis'], out['elpd_psis_se'], out['p_loo'], out['max_pareto_k'], out['pareto_k_threshold'], out['n_pareto_k_bad'])
    logging.getLogger(__name__).info('predictive: elpd_waic [%5.4f +- %5.4f] p_waic [%5.4f] lppd [%5.4f] elpd_isloo [%5.4f +- %5.4f] '
                                     'min IS-LOO ESS [%.1f] rows [%d] route [%s]%s' % (
                                         out['elpd_waic'], out['elpd_waic_se'], out['p_waic'], out['lppd'], out['elpd_isloo'],
                                         out['elpd_isloo_se'], out['min_isloo_ess'], n, out['route'], extra))
    return out


def laplace_evidence(like, prior, **kw):
    """The Laplace evidence of a regression posterior (build-defined: the reference has none) -- the third evidence beside the
    annealed (SMCSampler.logz) and the importance-sampled one (importance_evidence), and the cheapest: a few Newton steps, no flow.
    like: a likelihoods.GLMData; prior: a priors.GaussianPrior (ValueError for None: no evidence is defined without a proper prior,
    as importance_evidence refuses it); further keywords go to GLMData.laplace (theta0, tol, max_iter, route).
    Returns a dict: logz = logl + logprior + (D / 2) log 2 pi - logdet / 2 at the mode, logl, logdet, iterations, converged, and
    fit, the LaplaceFit.  Logs one line."""
    if prior is None:
        raise ValueError('laplace_evidence: no evidence is defined without a proper prior: pass a priors.GaussianPrior')
    fit = like.laplace(prior=prior, **kw)
    out = dict(logz=fit.logz, logl=fit.logl, logdet=fit.logdet, iterations=fit.iterations, converged=fit.converged, fit=fit)
    logging.getLogger(__name__).info('Laplace: log Z [%5.4f] at logL [%5.4f] in [%d] Newton steps' % (out['logz'], out['logl'], out['iterations']))
    return out
