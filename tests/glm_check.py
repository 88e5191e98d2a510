"""A numpy restatement of the regression likelihoods of user data (include/nnest_hip.h nnest_glm_t, nnest_loglike_glm)
and the a-priori bound on what any legal evaluation may differ from float64 by.

The definition, on a float32 row t and the float32 descriptor (at [D, ld] = A^T, y [ld], o [ld], logl0, n, family):
    eta_i = o_i + sum_c A[i, c] t_c         float32, in an order of the evaluator's own (fused multiply-adds allowed)
    l_i   = -softplus((1 - 2 y_i) eta_i)    logistic;   y_i eta_i - exp(eta_i)   poisson;   float64 from (double)eta_i;
            softplus(s) = max(s, 0) + log1p(exp(-|s|));  NaN where eta_i is not finite
    logL  = logl0 + sum_{i < n} l_i         float64;  -1e100 where that is not finite.  Rows i >= n are masked.

The bound, with u = 2^-23 (one ulp: it covers a truncating accumulate in the matrix cores as well as round-to-nearest) and
gamma_k = k u / (1 - k u):
    e_i   = gamma_{D + 2} (|o_i| + sum_c |A[i, c]| |t_c|)
    lip_i = 1 (logistic);  |y_i| + exp(eta_i + e_i) (poisson)
    B(t)  = sum_i lip_i e_i + (n + 16) 2^-53 (|logl0| + sum_i (|l_i| + |y_i eta_i| + [poisson] exp(eta_i))).
gamma_{D + 1} is the classical bound of a length-(D + 1) sum of products in any order (Higham, Accuracy and Stability, 3.1: the D
products and the offset), with one more rounding to spare; the computed eta~_i is within e_i of eta_i.  |d l_i / d eta| <= 1 for the
logistic family (the derivative of softplus is a probability) and <= |y_i| + exp(eta) for the Poisson one, largest at the upper end
eta_i + e_i of the interval, so |l_i(eta~_i) - l_i(eta_i)| <= lip_i e_i.  The second term is the float64 part: each l_i is a few
float64 operations on values no larger than |l_i|, |y_i eta_i| and exp(eta_i) with exp and log1p good to a few ulp -- 16 ulp of slack
in all --, and the sum of n terms and logl0 in any order adds at most n 2^-53 times the sum of the magnitudes."""
import numpy as np

U = 2.0 ** -23
SAFE = -1e100
LOGL0 = -3.25
FAMILIES = ('logistic', 'poisson')


def make_data(D, n, family, seed, with_offset=True):
    """the tests' data: A uniform in +-1/sqrt(D) (so that |eta| stays moderate for t in a box of a few units), a true theta in
    +-1, y drawn from the model, an offset in +-0.2.  Returns (A, y, offset) in float64"""
    r = np.random.RandomState(seed)
    A = r.uniform(-1.0, 1.0, size=(n, D)) / np.sqrt(D)
    theta = r.uniform(-1.0, 1.0, D)
    o = r.uniform(-0.2, 0.2, n) if with_offset else np.zeros(n)
    eta = o + A @ theta
    if family == 'logistic':
        y = (r.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = r.poisson(np.exp(eta + 0.5)).astype(np.float64)
    return A, y, o


def make_like(D, n, family, seed, logl_const=LOGL0):
    from nnest_amd.likelihoods import GLMData
    A, y, o = make_data(D, n, family, seed)
    return GLMData(A, y, family=family, offset=o, logl_const=logl_const)


def _parts(data):
    n = int(data['n'])
    at = np.asarray(data['at'], np.float32)[:, :n].astype(np.float64)
    return n, at.T, np.asarray(data['y'], np.float32)[:n].astype(np.float64), np.asarray(data['o'], np.float32)[:n].astype(np.float64)


def finish(logl0, s):
    with np.errstate(invalid='ignore', over='ignore'):
        acc = np.float64(logl0) + np.asarray(s, np.float64)
    return np.where(np.abs(acc) <= np.finfo(np.float64).max, acc, SAFE)   # (a NaN compares false)


def terms(family, eta, y):
    """l_i in float64 from eta [N, n] float64 (NaN where eta is not finite)"""
    with np.errstate(invalid='ignore', over='ignore'):
        if family == 'logistic':
            s = (1.0 - 2.0 * y) * eta
            l = -(np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))))
        else:
            l = y * eta - np.exp(eta)
    return np.where(np.isfinite(eta), l, np.nan)


def exact(data, t):
    """float64 from the float32 inputs: (logL [N], eta [N, n], l [N, n]); the safe rule applied to logL"""
    n, A, y, o = _parts(data)
    with np.errstate(invalid='ignore', over='ignore'):
        eta = o + np.asarray(t, np.float32).astype(np.float64) @ A.T
        l = terms(data['family'], eta, y)
        return finish(data['logl0'], np.sum(l, axis=1)), eta, l


def eta_error(data, t):
    """e_i [N, n]"""
    n, A, y, o = _parts(data)
    D = A.shape[1]
    k = D + 2.0
    gamma = k * U / (1.0 - k * U)
    with np.errstate(invalid='ignore', over='ignore'):
        return gamma * (np.abs(o) + np.abs(np.asarray(t, np.float32).astype(np.float64)) @ np.abs(A).T)


def lipschitz(data, eta, e):
    n, A, y, o = _parts(data)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.ones_like(eta) if data['family'] == 'logistic' else np.abs(y) + np.exp(eta + e)


def bound(data, t):
    """B(t) [N] (a non-finite row has no bound: NaN or inf)"""
    n, A, y, o = _parts(data)
    _, eta, l = exact(data, t)
    e = eta_error(data, t)
    with np.errstate(invalid='ignore', over='ignore'):
        mag = np.abs(l) + np.abs(y * eta) + (np.exp(eta) if data['family'] == 'poisson' else 0.0)
        return np.sum(lipschitz(data, eta, e) * e, axis=1) + (n + 16) * 2.0 ** -53 * (abs(float(data['logl0'])) + np.sum(mag, axis=1))


def float32_eval(data, t, order):
    """the definition with eta in float32 numpy, summed `forward` (o_i, then c = 0 .. D - 1), `reversed` (c = D - 1 .. 0, then o_i)
    or `pairwise` (a balanced tree over the D products and o_i); the products are rounded (no fused multiply-add in numpy); the
    terms and their sum in float64.  It reads the PADDED arrays and masks the rows i >= n, as the kernels do"""
    n = int(data['n'])
    at, y, o = np.asarray(data['at'], np.float32), np.asarray(data['y'], np.float32), np.asarray(data['o'], np.float32)
    t = np.asarray(t, np.float32)
    D, ld = at.shape
    N = len(t)

    def tree(v):
        while len(v) > 1:
            nxt = [v[i] + v[i + 1] for i in range(0, len(v) - 1, 2)]
            if len(v) % 2:
                nxt.append(v[-1])
            v = nxt
        return v[0]

    with np.errstate(invalid='ignore', over='ignore'):
        prods = [np.outer(t[:, c], at[c]).astype(np.float32) for c in range(D)]   # [N, ld] each, rounded to float32
        off = np.broadcast_to(o, (N, ld)).astype(np.float32)
        if order == 'pairwise':
            eta = tree(prods + [off])
        else:
            seq = [off] + prods if order == 'forward' else prods[::-1] + [off]
            eta = seq[0]
            for v in seq[1:]:
                eta = (eta + v).astype(np.float32)
        l = terms(data['family'], eta.astype(np.float64), y.astype(np.float64))
        l = np.where(np.arange(ld) < n, l, 0.0)   # (masked, not padded)
        s = np.zeros(N)
        for i in range(ld):
            s = s + l[:, i]
    return finish(data['logl0'], s)


def sensitivity(data, t, t_std, x_tol):
    """how far logL can move when x moves by x_tol per coordinate under T(x) = x t_std + t_mean, by Taylor's theorem with the
    Lagrange remainder in dt_c = x_tol |t_std_c|: the first order x_tol sum_c |g_c| |t_std_c| with the gradient
    g_c = sum_i l_i'(eta_i) A[i, c], and the second order 1/2 sum_i w_i d_i^2, where eta_i moves by at most
    d_i = x_tol sum_c |A[i, c]| |t_std_c| and w_i bounds |l_i''| over that interval: 1/4 (logistic), exp(eta_i + d_i) (poisson)"""
    n, A, y, o = _parts(data)
    _, eta, _ = exact(data, t)
    s = np.abs(np.asarray(t_std, np.float64))
    x_tol = np.asarray(x_tol, np.float64).reshape(-1, 1)
    d = x_tol * (np.abs(A) @ s)[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        if data['family'] == 'logistic':
            dl = (2.0 * y - 1.0) / (1.0 + np.exp((2.0 * y - 1.0) * eta))   # d/d eta of -softplus((1 - 2 y) eta)
            w = 0.25
        else:
            dl = y - np.exp(eta)
            w = np.exp(eta + d)
        return x_tol[:, 0] * (np.abs(dl @ A) @ s) + 0.5 * np.sum(w * d * d, axis=1)


def replay_target(D, n, family):
    """the replay's target (tests/test_gpu_mcmc_glm.py, tools/mcmc_glm_cases.py): the descriptor of make_like(D, n, family, D)"""
    return make_like(D, n, family, D).hip_like_glm


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


def posterior_mode(like, lo, hi, iters=50):
    """the maximum of the (concave) log-likelihood over the box [lo, hi]: damped Newton steps in float64, clipped to the box.
    Returns (theta, logL(theta))"""
    A, y, o = like.A, like.y, like.offset
    D = A.shape[1]
    th = np.clip(np.zeros(D), lo, hi)
    for _ in range(iters):
        eta = o + A @ th
        if like.family == 'logistic':
            p = 1.0 / (1.0 + np.exp(-eta))
            g, w = A.T @ (y - p), p * (1.0 - p)
        else:
            mu = np.exp(eta)
            g, w = A.T @ (y - mu), mu
        H = (A * w[:, None]).T @ A + 1e-9 * np.eye(D)
        step = np.linalg.solve(H, g)
        f0 = like.loglike_rows(th[None])[0]
        a = 1.0
        while a > 1e-6:
            cand = np.clip(th + a * step, lo, hi)
            if like.loglike_rows(cand[None])[0] >= f0:
                break
            a *= 0.5
        th = cand if a > 1e-6 else th
    return th, float(like.loglike_rows(th[None])[0])
