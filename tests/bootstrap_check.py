"""Numpy restatements of what EnsembleSampler.bootstrap takes from emcee (float64), for the tests:

`integrated_time`: emcee 3's autocorr.integrated_time with has_walkers=True, by direct sums -- per dimension,
    acf_k(s) = sum_{t < T - s} (x_kt - m_k)(x_k,t+s - m_k) with m_k the walker's own mean (not divided by T - s),
    f(s) = mean_k acf_k(s) / acf_k(0), taus = 2 cumsum(f) - 1, window = argmin(arange(T) < c taus) if any entry is true else T - 1
    (an all-true comparison gives window 0: emcee's auto_window), tau = taus[window]; AutocorrError when tol tau > T.
`integrated_time_fft`: the same definition with the sums taken by FFT (zero-padded to the next power of two at least 2 T), the
    way emcee computes them.
`emcee_thin`: get_chain(discard, thin, flat=True) on a chain [steps, walkers, D].
`ar1`: the AR(1) walkers the tests use.
"""
import numpy as np


class AutocorrError(Exception):
    def __init__(self, tau, thresh):
        self.tau, self.thresh = tau, thresh
        super(AutocorrError, self).__init__('chain shorter than tol tau: tau %s, thresh %s' % (tau, thresh))


def acf_direct(x):
    """f [T, D]: x [C, T, D]"""
    x = np.asarray(x, np.float64)
    C, T, D = x.shape
    y = x - x.mean(axis=1, keepdims=True)
    f = np.empty((T, D))
    a0 = np.einsum('ktd,ktd->kd', y, y)
    for s in range(T):
        f[s] = np.mean(np.einsum('ktd,ktd->kd', y[:, :T - s], y[:, s:]) / a0, axis=0)
    return f


def acf_fft(x):
    x = np.asarray(x, np.float64)
    C, T, D = x.shape
    y = x - x.mean(axis=1, keepdims=True)
    n = 1
    while n < 2 * T:
        n *= 2
    F = np.fft.fft(y, n=n, axis=1)
    acf = np.fft.ifft(F * np.conjugate(F), axis=1)[:, :T].real
    return np.mean(acf / acf[:, :1], axis=0)


def auto_window(taus, c):
    m = np.arange(len(taus)) < c * taus
    return int(np.argmin(m)) if np.any(m) else len(taus) - 1


def tau_of(f, c=5, tol=50, quiet=False):
    """(tau [D], windows [D]) of an autocorrelation table f [T, D]"""
    T, D = f.shape
    tau, windows = np.empty(D), np.empty(D, int)
    for d in range(D):
        taus = 2.0 * np.cumsum(f[:, d]) - 1.0
        windows[d] = auto_window(taus, c)
        tau[d] = taus[windows[d]]
    if tol > 0 and np.any(tol * tau > T) and not quiet:
        raise AutocorrError(tau, T / tol)
    return tau, windows


def integrated_time(x, c=5, tol=50, quiet=False):
    return tau_of(acf_direct(x), c, tol, quiet)


def integrated_time_fft(x, c=5, tol=50, quiet=False):
    return tau_of(acf_fft(x), c, tol, quiet)


def emcee_thin(chain, discard, thin):
    """chain [steps, walkers, D] -> the rows get_chain(discard=discard, thin=thin, flat=True) returns"""
    chain = np.asarray(chain)
    return chain[discard + thin - 1:len(chain):thin].reshape(-1, chain.shape[2])


def ar1(rng, C, T, D, phi):
    """stationary AR(1) walkers x [C, T, D], unit variance"""
    x = np.empty((C, T, D))
    x[:, 0] = rng.normal(size=(C, D))
    e = rng.normal(size=(C, T, D)) * np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x
