"""A numpy restatement of the independent normal priors of the fused Metropolis runs (include/nnest_hip.h nnest_gauss_prior_t,
nnest_logprior_gauss, nnest_mcmc_glm_prior_steps), the a-priori bound on what any legal evaluation may differ from
float64 by, and the latent target with that prior beside a regression likelihood of user data (tests/glm_check.Restated, extended
by composition).

The definition, on a float32 row t and the float32 descriptor (m [D], r [D], logc):
    u_c    = (t_c - m_c) * r_c                 float32, each operation rounded
    ss     = sum_c (double)u_c (double)u_c     float64, in an order of the evaluator's own
    log pi = logc - 0.5 ss                     float64;  -inf where ss is not finite
`exact` evaluates it in float64 throughout from the float32 inputs.

The bound B_pi(t) = 2^-22 * 1/2 ss + 2^-45 * (|logc| + 1/2 ss) + 2^-240, with ss the float64 value:
  * u_c carries two float32 roundings, each of relative size d <= 2^-24 / (1 + 2^-24) (round to nearest), so the computed u_c^2 is
    the true one times (1 + d)^4 at most: off by at most 4 d + 6 d^2 + ... <= 2^-22 + 2^-47 of itself.  Summed over c that is the
    first term, 2^-22 * 1/2 ss in log pi, and 2^-47 * 1/2 ss left over.
  * the float64 part: the products (double)u (double)u are exact; a sum of D <= 128 non-negative terms in ANY order is off by at
    most (D - 1) 2^-53 < 2^-46 of the sum; 0.5 ss is exact; the subtraction adds 2^-53 (|logc| + 1/2 ss); `exact` itself is a dozen
    float64 roundings, 12 * 2^-53 < 2^-49 of ss.  Together (2^-47 + 2^-46 + 2^-53 + 2^-49) 1/2 ss + 2^-53 |logc|, below the
    second term 2^-45 (|logc| + 1/2 ss).
  * 2^-240 is the floor for float32 products (t - m) r that underflow: below 2^-126 in size u keeps fewer bits or is flushed to 0,
    and the relative argument above fails; but then both the computed and the true u^2 are below 2^-252, and D <= 128 of them
    add up to less than 2^-245.  It matters only where ss and logc are 0.
A row with a non-finite coordinate has no bound: log pi is -inf there, exactly."""
import numpy as np

from tests import glm_check as gk


def descriptor(prior):
    """the float32 descriptor of a priors.GaussianPrior (its hip_gauss_prior), or the mapping itself"""
    return getattr(prior, 'hip_gauss_prior', prior)


def sum_sq(data, t):
    """ss [N] in float64 from the float32 inputs"""
    data = descriptor(data)
    m, r = np.asarray(data['m'], np.float32).astype(np.float64), np.asarray(data['r'], np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        u = (np.asarray(t, np.float32).astype(np.float64) - m) * r
        return np.sum(u * u, axis=1)


def exact(data, t):
    """log pi [N] in float64 from the float32 inputs; -inf where the sum of squares is not finite (never NaN)"""
    ss = sum_sq(data, t)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(np.isfinite(ss), float(descriptor(data)['logc']) - 0.5 * ss, -np.inf)


def bound(data, t):
    """B_pi(t) [N] (the module's docstring derives it); NaN or inf on a non-finite row"""
    ss = sum_sq(data, t)
    return 2.0 ** -22 * 0.5 * ss + 2.0 ** -45 * (abs(float(descriptor(data)['logc'])) + 0.5 * ss) + 2.0 ** -240


def float32_eval(data, t, order='forward'):
    """the definition as the kernels compute it: u in float32 numpy with both operations rounded, the squares and their sum in
    float64, summed `forward` (c = 0 .. D - 1) or `reversed`"""
    data = descriptor(data)
    m, r = np.asarray(data['m'], np.float32), np.asarray(data['r'], np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        u = ((np.asarray(t, np.float32) - m).astype(np.float32) * r).astype(np.float32).astype(np.float64)
        sq = u * u
        cols = range(sq.shape[1]) if order == 'forward' else range(sq.shape[1] - 1, -1, -1)
        ss = np.zeros(len(sq))
        for c in cols:
            ss = ss + sq[:, c]
        return np.where(np.isfinite(ss), float(data['logc']) - 0.5 * ss, -np.inf)


def sensitivity(data, t, t_std, x_tol):
    """how far log pi can move when x moves by x_tol per coordinate under T(x) = x t_std + t_mean: log pi is quadratic in t, so
    Taylor's expansion ends at the second order -- x_tol sum_c |u_c| r_c |t_std_c| + 1/2 sum_c (r_c |t_std_c| x_tol)^2"""
    data = descriptor(data)
    m, r = np.asarray(data['m'], np.float32).astype(np.float64), np.asarray(data['r'], np.float32).astype(np.float64)
    s = np.abs(np.asarray(t_std, np.float64)) * r
    x_tol = np.asarray(x_tol, np.float64).reshape(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        u = np.abs((np.asarray(t, np.float32).astype(np.float64) - m) * r)
        return x_tol * (u @ s) + 0.5 * x_tol * x_tol * np.sum(s * s)


class RestatedPrior(object):
    """the latent target of nnest_mcmc_glm_prior_steps in the kernels' arithmetic: tests/glm_check.Restated (the oracle's inverse,
    T in float32, logL in float64 from the float32 row) with log pi of `exact` in the target where that one has 0.0,
    lp_beta = ((beta logL) + log|det|) + log pi, each operation rounded; -inf outside the box +-half (None: no box)"""

    def __init__(self, o, data, prior, sd, mu, half=None, beta=1.0):
        self.base = gk.Restated(o, data, sd, mu, np.inf if half is None else half)
        self.o, self.data, self.sd, self.mu, self.half = o, data, self.base.sd, self.base.mu, half
        self.prior, self.beta = descriptor(prior), float(beta)
        self.T, self.x_of_z, self.logl = self.base.T, self.base.x_of_z, self.base.logl

    def in_prior(self, x):
        """inside the box (every row where there is none: the kernels count a NaN as inside, and log pi refuses it)"""
        return np.ones(len(x), bool) if self.half is None else self.base.in_prior(x)

    def logpi(self, x):
        return exact(self.prior, self.T(x))

    def lp(self, q):
        x, ld = self.x_of_z(q)
        ll = np.asarray(self.logl(x), np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            return ((self.beta * ll) + np.asarray(ld, np.float64)) + np.where(self.in_prior(x), self.logpi(x), -np.inf)

    def like_tol(self, x, x_tol):
        """what the kernel's logL + log pi at a row may differ from the restated by when its x is within x_tol of x: B and B_pi plus
        the two sensitivities"""
        t = self.T(x)
        with np.errstate(invalid='ignore', over='ignore'):
            return self.base.like_tol(x, x_tol) + bound(self.prior, t) + sensitivity(self.prior, t, self.sd, x_tol)


def mixed_step(t, k, z, lp, eps, u, step_size, rs, record=None):
    """tests/mcmc_adapt_check.mixed_step on the target `rs` (a RestatedPrior): the walk itself is unchanged, only lp differs"""
    from tests import mcmc_adapt_check as ac
    return ac.mixed_step(t, k, z, lp, eps, u, step_size, rs.lp, record=record)


def replay_prior(D, width):
    """the replay's prior (tests/test_gpu_mcmc_glm_prior.py, tools/mcmc_glm_prior_cases.py): means in +-0.3 and sigmas in
    width * [0.7, 1.3], drawn from RandomState(D)"""
    from nnest_amd.priors import GaussianPrior
    r = np.random.RandomState(1000 + D)
    return GaussianPrior(D, r.uniform(-0.3, 0.3, D), width * r.uniform(0.7, 1.3, D))
