"""Chain statistics restated in vectorised float64 numpy from their definitions (include/nnest_hip.h nnest_chain_stats; the
reference's nnest/utils/evaluation.py): the checker of nnest_amd.evaluation.  Not the product: the product has no CPU path."""
import numpy as np


def moments(x):
    r = x.reshape(-1, x.shape[2])
    return r.mean(axis=0), r.std(axis=0)


def acceptance(x):
    moved = np.any(x[:, 1:] != x[:, :-1], axis=2)
    return moved.sum() / float(x.shape[0] * (x.shape[1] - 1))


def jump(x):
    return np.sqrt(((x[:, 1:] - x[:, :-1]) ** 2).sum(axis=2)).sum() / float(x.shape[0] * (x.shape[1] - 1))


def autocorr(x, mu, sd, lags=None):
    """p [len(lags), D]; lags default 1..T-1.  Divided by sd (the reference's `var` argument), averaged over chains."""
    C, T, D = x.shape
    y = x - mu
    lags = range(1, T) if lags is None else lags
    return np.array([np.einsum('ijd,ijd->d', y[:, :T - s], y[:, s:]) / (T - s) / C / sd for s in lags]).reshape(-1, D)


def ess_from_p(p, T):
    """ESS_d = T / e_d and the stop lag (T when the sum never stops), p [n >= lags examined, D] with row s - 1 = lag s"""
    e = np.ones(p.shape[1])
    for s in range(1, T):
        above = p[s - 1] > 0.05
        if not above.any():
            return T / e, s
        e = e + np.where(above, 2.0 * p[s - 1] * (1.0 - float(s) / T), 0.0)
    return T / e, T


def rhat(x, mu=None):
    C, T, _ = x.shape
    theta, sigma = x.mean(axis=1), x.var(axis=1)
    tb = mu if mu is not None else theta.mean(axis=0)
    b = T / (C - 1.0) * ((theta - tb) ** 2).sum()     # summed over the dimensions too (evaluation.py:88: np.sum, no axis)
    w = 1.0 / (C * sigma.sum(axis=0) + 1e-5)
    v = (T - 1.0) / T * w + (C + 1.0) / (C * T) * b
    return np.sqrt(v / w)


def stats(x, mean=None, std=None):
    """everything nnest_amd.evaluation.chain_stats returns, from float64 arithmetic on x (cast first)"""
    x = np.asarray(x, dtype=np.float64)
    m0, s0 = moments(x)
    mu = m0 if mean is None else np.asarray(mean, np.float64)
    sd = s0 if std is None else np.asarray(std, np.float64)
    p = autocorr(x, mu, sd)
    ess, stop = ess_from_p(p, x.shape[1])
    return dict(acceptance=acceptance(x), jump_distance=jump(x), p=p, ess=ess, stop_lag=stop,
                rhat=rhat(x) if x.shape[0] > 1 else None, mean=mu, std=sd)
