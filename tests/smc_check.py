"""A numpy restatement of the sequential Monte Carlo sampler's pieces (include/nnest_hip.h nnest_smc_reweight, nnest_smc_resample,
nnest_mcmc_tempered_steps): the reweighting rule (the same bisection in the same order), the integer weights, the
systematic rule with the Philox word of stream 8, the tempered latent target, and a numpy-only sampler (identity preconditioner, numpy
Metropolis) that pins the estimator and the convention of log Z.  Float64 throughout, each operation rounded."""
import numpy as np

from tests.mcmc_walk_check import philox4x32_10

STREAM_SMC = 8
WEIGHT_ONE = 2.0 ** 31
MAX_N = 1 << 20


def weights(logl, beta, b, mx=None):
    """w_i(b) = exp((b - beta) (logL_i - max logL))"""
    logl = np.asarray(logl, np.float64)
    mx = float(np.max(logl)) if mx is None else mx
    return np.exp((b - beta) * (logl - mx))


def ess_of(w):
    s1, s2 = float(np.sum(w)), float(np.sum(w * w))
    return s1 * s1 / s2


def next_beta(logl, beta, ess_fraction):
    """the next temperature: 1 where ESS(1) reaches the target, else 64 bisection steps on [beta, 1]; never at or below beta"""
    logl = np.asarray(logl, np.float64)
    target = ess_fraction * len(logl)
    mx = float(np.max(logl))
    if ess_of(weights(logl, beta, 1.0, mx)) >= target:
        return 1.0
    lo, hi = float(beta), 1.0
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if ess_of(weights(logl, beta, mid, mx)) < target:
            hi = mid
        else:
            lo = mid
    return hi if hi > beta else 1.0


def increment(logl, beta, b, carried=None):
    """log((1 / N) sum_i exp((b - beta) logL_i)), through max logL: log Z(b) - log Z(beta) from a population at beta.  carried: the
    weights W_i a population that was NOT resampled carries (a ladder without resampling): log(sum W_i w_i / sum W_i)"""
    logl = np.asarray(logl, np.float64)
    mx = float(np.max(logl))
    w = weights(logl, beta, b, mx)
    if carried is None:
        return (b - beta) * mx + np.log(np.sum(w) / len(logl))
    carried = np.asarray(carried, np.float64)
    return (b - beta) * mx + np.log(np.sum(carried * w) / np.sum(carried))


def integer_weights(logl, beta, b):
    return np.floor(weights(logl, beta, b) * WEIGHT_ONE).astype(np.int64)


def reweight(logl, beta, ess_fraction):
    """what nnest_smc_reweight returns: out = (beta', increment, ESS(beta'), max logL) and m [N] int64"""
    b = next_beta(logl, beta, ess_fraction)
    return (b, increment(logl, beta, b), ess_of(weights(logl, beta, b)), float(np.max(logl))), integer_weights(logl, beta, b)


def smc_uniform(seed, stage):
    """u of (seed, stage): the top 24 bits of word 0 of Philox(key seed; counter (0, stage, 0, 8 << 28)) / 2^24"""
    r = philox4x32_10(np.array([0, int(stage), 0, STREAM_SMC << 28], np.uint64), seed)
    return float(int(r[0]) >> 8) * 2.0 ** -24


def systematic(m, u):
    """anc [N]: anc_j the smallest i whose inclusive prefix sum of m exceeds p_j = floor(((j + u) T) / N), T = sum m; float64 positions
    (every operand exact), integer prefix sums"""
    m = np.asarray(m, np.int64)
    N = len(m)
    cum = np.cumsum(m)
    T = int(cum[-1])
    assert T > 0 and np.all(m >= 0)
    p = np.floor(((np.arange(N, dtype=np.float64) + np.float64(u)) * np.float64(T)) / np.float64(N)).astype(np.int64)
    assert p.min() >= 0 and p.max() < T
    return np.searchsorted(cum, p, side='right').astype(np.int64)


def tempered_target(x_of_z, logl, in_prior, beta):
    """lp_beta(z) = ((beta * logL) + log|det|) + prior for a flow given as x_of_z(q) -> (x, log|det dx/dz|): tests/ensemble_check's
    latent_target with the likelihood to the power beta"""
    def lp_fn(q):
        x, ld = x_of_z(q)
        ll = np.asarray(logl(x), np.float64)
        prior = np.where(in_prior(x), 0.0, -np.inf)
        return ((np.float64(beta) * ll) + np.asarray(ld, np.float64)) + prior
    return lp_fn


def numpy_smc(logl_fn, lo, hi, N, mcmc_steps, ess_fraction, rng, max_stages=1000):
    """the sampler with the identity for the flow: theta ~ U[lo, hi]^D, then per stage reweight, resample (u from `rng`), and
    `mcmc_steps` Metropolis steps on L^beta' in the box, the step per dimension from the population's spread.  Returns log Z (with the
    NORMALISED prior), the betas and theta"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    D = len(lo)
    theta = lo + (hi - lo) * rng.uniform(size=(N, D))
    logl = np.asarray(logl_fn(theta), np.float64)
    beta, logz, betas = 0.0, 0.0, []
    while beta < 1.0:
        assert len(betas) < max_stages
        (b, inc, _, _), m = reweight(logl, beta, ess_fraction)
        anc = systematic(m, np.floor(rng.uniform() * 2 ** 24) / 2 ** 24)
        theta, logl = theta[anc], logl[anc]
        step = 2.0 / np.sqrt(D) * np.std(theta, axis=0)
        for _ in range(mcmc_steps):
            q = theta + step * rng.standard_normal((N, D))
            lq = np.asarray(logl_fn(q), np.float64)
            inside = np.all((q >= lo) & (q <= hi), axis=1)
            acc = inside & (b * (lq - logl) > np.log(rng.uniform(size=N)))
            theta[acc], logl[acc] = q[acc], lq[acc]
        logz += inc
        beta = b
        betas.append(b)
    return logz, betas, theta
