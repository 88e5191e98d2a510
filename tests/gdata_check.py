"""A numpy restatement of the Gaussian likelihood from user data (include/nnest_hip.h nnest_gdata_t, nnest_loglike_gdata; DESIGN.md
3.15) and the a-priori bound on what any legal evaluation may differ from float64 by.

The definition, on a float32 row t and the float32 descriptor (mu [D], R [D, D] upper triangular, logl0):
    d_c  = t_c - mu_c                       float32, one rounding
    y_r  = sum_{c >= r} R[r, c] d_c         float32, in an order of the evaluator's own (fused multiply-adds allowed)
    q    = sum_r (double)y_r (double)y_r    float64
    logL = logl0 - 0.5 q;  -1e100 where that is not finite.

The bound, with y_r the exact value from the float32 inputs, n_r = D - r terms in row r and u = 2^-23 (one ulp: it covers a
truncating accumulate in the matrix cores as well as round-to-nearest):
    gamma_n = n u / (1 - n u)
    e_r     = gamma_{n_r + 1} sum_c |R[r, c]| |t_c - mu_c|
    B(t)    = sum_r (|y_r| e_r + 1/2 e_r^2) + 2^-50 (|logl0| + q).
gamma_{n + 1} is the classical bound of a length-n inner product in any order (Higham, Accuracy and Stability, 3.1) with one more
rounding for d_c; the computed y~_r is within e_r of y_r, so 1/2 |y~_r^2 - y_r^2| <= |y_r| e_r + 1/2 e_r^2, and the float64 sum of D
exact squares and the last subtraction add at most (D + 2) 2^-53 < 2^-50 relative to |logl0| + q."""
import numpy as np

U = 2.0 ** -23
SAFE = -1e100


def make_target(D, seed):
    """the GPU tests' target: P = Q diag(lambda) Q^T with lambda in [0.5, 4] and Q a random rotation (R dense, condition number at
    most 8), mu in +-0.3"""
    r = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(r.normal(size=(D, D)))
    lam = r.uniform(0.5, 4.0, D)
    P = (Q * lam) @ Q.T
    return r.uniform(-0.3, 0.3, D), 0.5 * (P + P.T)


def finish(logl0, q):
    with np.errstate(invalid='ignore', over='ignore'):
        acc = np.float64(logl0) - 0.5 * np.asarray(q, np.float64)
    return np.where(np.abs(acc) <= np.finfo(np.float64).max, acc, SAFE)   # (a NaN compares false)


def exact(data, t):
    """float64 from the float32 inputs: (logL, y [N, D], q [N]); the safe rule applied to logL"""
    mu, R = np.asarray(data['mu'], np.float32).astype(np.float64), np.triu(np.asarray(data['R'], np.float32)).astype(np.float64)
    d = np.asarray(t, np.float32).astype(np.float64) - mu
    with np.errstate(invalid='ignore', over='ignore'):
        y = d @ R.T
        q = np.sum(y * y, axis=1)
    return finish(data['logl0'], q), y, q


def bound(data, t):
    """B(t) [N]"""
    mu, R = np.asarray(data['mu'], np.float32).astype(np.float64), np.triu(np.asarray(data['R'], np.float32)).astype(np.float64)
    D = len(mu)
    ad = np.abs(np.asarray(t, np.float32).astype(np.float64) - mu)
    _, y, q = exact(data, t)
    n = (D - np.arange(D)) + 1.0                      # n_r + 1
    gamma = n * U / (1.0 - n * U)
    with np.errstate(invalid='ignore', over='ignore'):   # (a non-finite row has no bound: NaN)
        e = gamma * (ad @ np.abs(R).T)
        return np.sum(np.abs(y) * e + 0.5 * e * e, axis=1) + 2.0 ** -50 * (abs(float(data['logl0'])) + q)


def float32_eval(data, t, order):
    """the definition in float32 numpy, y_r summed `forward` (c = r .. D - 1), `reversed` (c = D - 1 .. r) or `pairwise` (a balanced
    tree over c = r .. D - 1); the products are rounded (no fused multiply-add in numpy), q in float64 over r = 0 .. D - 1"""
    mu, R = np.asarray(data['mu'], np.float32), np.triu(np.asarray(data['R'], np.float32))
    t = np.asarray(t, np.float32)
    D = len(mu)
    d = t - mu
    y = np.zeros(t.shape, np.float32)

    def tree(terms):   # terms: list of [N] float32
        while len(terms) > 1:
            nxt = [terms[i] + terms[i + 1] for i in range(0, len(terms) - 1, 2)]
            if len(terms) % 2:
                nxt.append(terms[-1])
            terms = nxt
        return terms[0]

    for r in range(D):
        terms = [R[r, c] * d[:, c] for c in range(r, D)]
        if order == 'pairwise':
            y[:, r] = tree(terms)
        else:
            if order == 'reversed':
                terms = terms[::-1]
            acc = np.zeros(len(t), np.float32)
            for v in terms:
                acc = acc + v
            y[:, r] = acc
    q = np.zeros(len(t), np.float64)
    for r in range(D):
        q = q + y[:, r].astype(np.float64) * y[:, r].astype(np.float64)
    return finish(data['logl0'], q)


def sensitivity(data, t, t_std, x_tol):
    """how far logL can move when x moves by x_tol per coordinate under T(x) = x t_std + t_mean: first and second order in
    dt_c = x_tol |t_std_c|:  x_tol sum_c |(R^T y)_c| |t_std_c| + 1/2 x_tol^2 sum_rc |P_rc| |t_std_r| |t_std_c|"""
    R = np.triu(np.asarray(data['R'], np.float32)).astype(np.float64)
    _, y, _ = exact(data, t)
    s = np.abs(np.asarray(t_std, np.float64))
    P = R.T @ R
    return x_tol * (np.abs(y @ R) @ s) + 0.5 * x_tol ** 2 * float(s @ np.abs(P) @ s)


LOGL0 = -3.25


def replay_target(D):
    """the replay's target at width D (tests/test_gpu_mcmc_gdata.py, tools/mcmc_gdata_cases.py): the descriptor of make_target(D, D)
    at logl0 = -3.25, as GaussianData makes it"""
    from nnest_amd.likelihoods import GaussianData
    mu, P = make_target(D, D)
    return GaussianData(mu, precision=P, logl_max=LOGL0).hip_like_data


class Restated(object):
    """the latent target on this likelihood in the kernels' arithmetic: the oracle's inverse `o` (float32), T in float32 (two
    roundings), the box +-half on T(x), logL in float64 from the float32 row (`exact`)"""

    def __init__(self, o, data, sd, mu, half):
        from tests.ensemble_check import latent_target
        self.o, self.data, self.sd, self.mu, self.half = o, data, np.asarray(sd, np.float32), np.asarray(mu, np.float32), half
        self.lp = latent_target(self.x_of_z, self.logl, self.in_prior)

    def T(self, x):
        return (np.asarray(x, np.float32) * self.sd) + self.mu

    def in_prior(self, x):
        return np.all(np.abs(np.asarray(self.T(x), np.float64)) <= self.half, axis=1)

    def x_of_z(self, q):
        return self.o.inverse(np.asarray(q, np.float32))

    def logl(self, x):
        return exact(self.data, self.T(x))[0]

    def like_tol(self, x, x_tol):
        """what the kernel's logL at a row may differ from logl(x) by when its x is within x_tol of x: B plus the sensitivity"""
        t = self.T(x)
        with np.errstate(invalid='ignore', over='ignore'):
            return bound(self.data, t) + sensitivity(self.data, t, self.sd, x_tol)
