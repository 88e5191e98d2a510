"""A numpy.longdouble restatement of the gradient, curvature and Newton step of the regression likelihoods of user data
(include/nnest_hip.h nnest_glm_curv, nnest_glm_newton_solve) and the a-priori bounds on what any legal float64
evaluation may differ from it by.

The definition, on a float64 theta and the float32 descriptor (at [D, ld] = A^T, y [ld], o [ld], logl0, n, family), everything
float64 in the evaluator:
    eta_i = o_i + sum_c A[i, c] theta_c      in an order of the evaluator's own (fused multiply-adds allowed)
    l_i   = -softplus((1 - 2 y_i) eta_i)     logistic;   y_i eta_i - exp(eta_i)   poisson
    mu_i  = 1 / (1 + exp(-eta_i)), w_i = mu_i (1 - mu_i)   logistic;   mu_i = w_i = exp(eta_i)   poisson
    logL  = logl0 + sum_i l_i,   g_c = sum_i (y_i - mu_i) A[i, c],   H_cd = sum_i w_i A[i, c] A[i, d].   Rows i >= n are masked.
and, with the prior's float32 m, r = float32(1 / sigma) and logc,
    g_c <- g_c - (theta_c - m_c) r_c^2,   H_cc <- H_cc + r_c^2,   log pi = logc - 1/2 sum_c ((theta_c - m_c) r_c)^2,
    H = L L^T,   H delta = g,   lambda^2 = g^T delta,   log det H = 2 sum_c log L_cc.

THE BOUNDS, with u = 2^-53 and gamma_k = k u / (1 - k u).  They are derived, not measured.
  * eta.  The computed eta~_i is within e_i = gamma_{D + 2} (|o_i| + sum_c |A[i, c]| |theta_c|) of eta_i: the classical bound of a
    length-(D + 1) sum of products in any order (Higham, Accuracy and Stability, 3.1), one rounding to spare.
  * the row functions.  |d l / d eta| <= 1 (logistic), |y_i| + exp(eta_i + e_i) (poisson);  |d mu / d eta| and |d w / d eta| <= 1/4
    (logistic: mu (1 - mu) <= 1/4 and |w'| = w |1 - 2 mu| <= 1/4), exp(eta_i + e_i) (poisson: the largest over the interval).  Each
    of l_i, mu_i, w_i and the product w_i A[i, c] is a handful of float64 operations with exp and log1p good to a few ulp: 16 ulp of
    the magnitudes involved in all.
  * the sums.  A sum of n terms in any order adds at most (n + 16) u sum |term| (gamma_n <= (n + 16) u for n <= 65536).  So
      B_logL = sum_i lip_i e_i + (n + 16) u (|logl0| + sum_i (|l_i| + |y_i eta_i| + [poisson] exp(eta_i)))      (tests/glm_check.py's, at u)
      B_g[c] = sum_i |A[i, c]| (dmu_i e_i + 16 u (|y_i| + mu_i)) + (n + 16) u sum_i |y_i - mu_i| |A[i, c]|
      B_H[c, d] = sum_i |A[i, c] A[i, d]| (dw_i e_i + 16 u w_i) + (n + 16) u sum_i w_i |A[i, c] A[i, d]|.
  * the solve, from the evaluator's own g and H (so that the curvature's error is not counted twice).  The prior's terms are three
    float64 operations per coordinate: dg_c = 4 u (|g_c| + |theta_c - m_c| r_c^2), a relative 2 u on the diagonal of H.  Higham's
    backward error of a Cholesky solve (Theorem 10.4): (H + dH) delta~ = g with ||dH||_2 <= D gamma_{3 D + 1} ||H||_2.  With
    eps = D gamma_{3 D + 1} + 4 u and kappa = cond_2(H), for eps kappa < 1,
      ||delta~ - delta||_2 <= kappa / (1 - eps kappa) (eps + ||dg||_2 / ||g||_2) ||delta||_2                      (relative bound on delta)
      |log det~ - log det| <= -D log(1 - eps kappa) + (D + 16) u 2 sum_c |log L_cc|                             (absolute bound)
    -- the computed factor is the exact factor of H + dH', ||dH'||_2 <= eps ||H||_2 (Theorem 10.3), each eigenvalue of H^-1/2 dH'
    H^-1/2 is at most eps kappa in size, and log det is the sum of the D logarithms of one plus them; the second term is the sum
    of the D computed logarithms --, and
      |lambda^2~ - lambda^2| <= ||g||_2 ||delta~ - delta||_2 + ||dg||_2 ||delta||_2 + (D + 16) u sum_c |g_c delta_c|,
      |log pi~ - log pi| <= (D + 16) u (|logc| + sum_c ((theta_c - m_c) r_c)^2)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SAFE = -1e100


def gamma(k):
    return k * U / (1.0 - k * U)


def parts(data):
    """(n, A [n, D], y [n], o [n]) in longdouble from the float32 descriptor"""
    n = int(data['n'])
    at = np.asarray(data['at'], np.float32)[:, :n].astype(LD)
    return n, at.T, np.asarray(data['y'], np.float32)[:n].astype(LD), np.asarray(data['o'], np.float32)[:n].astype(LD)


def _is_logistic(data):
    return data['family'] in ('logistic', 0)


def rows(data, theta):
    """(eta, l, mu, w) [n] in longdouble at theta [D]"""
    n, A, y, o = parts(data)
    eta = o + A @ np.asarray(theta, np.float64).astype(LD)
    if _is_logistic(data):
        s = (1 - 2 * y) * eta
        l = -(np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s))))
        t = np.exp(-np.abs(eta))
        big, small = 1 / (1 + t), t / (1 + t)
        mu, w = np.where(eta >= 0, big, small), big * small
    else:
        mu = np.exp(eta)
        l, w = y * eta - mu, mu
    return eta, l, mu, w


def exact(data, theta):
    """(logL, g [D], H [D, D]) in longdouble"""
    n, A, y, o = parts(data)
    eta, l, mu, w = rows(data, theta)
    return LD(data['logl0']) + np.sum(l), A.T @ (y - mu), (A * w[:, None]).T @ A


def curvature_bounds(data, theta):
    """(B_logL, B_g [D], B_H [D, D]) in float64"""
    n, A, y, o = parts(data)
    D = A.shape[1]
    eta, l, mu, w = rows(data, theta)
    absA = np.abs(A)
    e = gamma(D + 2.0) * (np.abs(o) + absA @ np.abs(np.asarray(theta, np.float64).astype(LD)))
    if _is_logistic(data):
        lip, dmu, dw = np.ones_like(eta), np.full_like(eta, 0.25), np.full_like(eta, 0.25)
        mag = np.abs(l) + np.abs(y * eta)
    else:
        top = np.exp(eta + e)
        lip, dmu, dw = np.abs(y) + top, top, top
        mag = np.abs(l) + np.abs(y * eta) + np.exp(eta)
    tail = (n + 16) * U
    b_logl = np.sum(lip * e) + tail * (abs(LD(data['logl0'])) + np.sum(mag))
    b_g = absA.T @ (dmu * e + 16 * U * (np.abs(y) + mu)) + tail * (absA.T @ np.abs(y - mu))
    b_h = (absA * (dw * e + 16 * U * w)[:, None]).T @ absA + tail * ((absA * w[:, None]).T @ absA)
    return float(b_logl), b_g.astype(np.float64), b_h.astype(np.float64)


def prior_parts(prior_data):
    """(m [D], r [D], logc) in longdouble from the float32-rounded descriptor; None for no prior"""
    if prior_data is None:
        return None
    return np.asarray(prior_data['m'], np.float32).astype(LD), np.asarray(prior_data['r'], np.float32).astype(LD), LD(prior_data['logc'])


def add_prior(g, H, theta, prior_data):
    """(g, H, log pi, dg [D] the bound on the float64 g's own rounding) in longdouble with the prior's terms; unchanged without one"""
    g, H = np.asarray(g).astype(LD), np.asarray(H).astype(LD)
    pp = prior_parts(prior_data)
    if pp is None:
        return g, H, LD(0), np.zeros(len(g))
    m, r, logc = pp
    d = np.asarray(theta, np.float64).astype(LD) - m
    dg = 4 * U * (np.abs(g) + np.abs(d) * r * r)
    u = d * r
    return g - d * r * r, H + np.diag(r * r), logc - np.sum(u * u) / 2, dg.astype(np.float64)


def cholesky(H):
    """the lower Cholesky factor in longdouble (column by column); ValueError where H is not positive definite"""
    H = np.asarray(H).astype(LD)
    D = H.shape[0]
    L = np.zeros((D, D), LD)
    for j in range(D):
        s = H[j:, j] - L[j:, :j] @ L[j, :j]
        if not s[0] > 0:
            raise ValueError('not positive definite at column %d' % j)
        L[j:, j] = s / np.sqrt(s[0])
        L[j, j] = np.sqrt(s[0])
    return L


def solve(L, g):
    """delta of L L^T delta = g in longdouble"""
    D = len(g)
    y = np.zeros(D, LD)
    for j in range(D):
        y[j] = (g[j] - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros(D, LD)
    for j in range(D - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def solve_eps(D):
    """eps = D gamma_{3 D + 1} + 4 u: the relative size of the backward error of the Cholesky solve, the prior's diagonal included"""
    return D * gamma(3.0 * D + 1.0) + 4 * U


def logdet_bound(Hp, L=None):
    """the absolute bound on a float64 log det of Hp [D, D] (the prior included) by Cholesky; inf where eps kappa >= 1"""
    Hp = np.asarray(Hp)
    D = Hp.shape[0]
    L = cholesky(Hp) if L is None else L
    ek = solve_eps(D) * float(np.linalg.cond(Hp.astype(np.float64), 2))
    if ek >= 1.0:
        return np.inf
    return float(-D * np.log1p(-ek) + (D + 16) * U * 2.0 * float(np.sum(np.abs(np.log(np.diag(L))))))


def newton(g, H, theta, prior_data):
    """from an evaluator's own g [D] and H [D, D] (without the prior): dict of the longdouble step, chol, logdet, decrement, logpi, the
    matrix H with the prior, and the bounds step_rel, logdet_abs, decrement_abs, logpi_abs (float64; inf where eps kappa >= 1)"""
    gp, Hp, logpi, dg = add_prior(g, H, theta, prior_data)
    D = len(gp)
    L = cholesky(Hp)
    step = solve(L, gp)
    kappa = float(np.linalg.cond(Hp.astype(np.float64), 2))
    eps = solve_eps(D)
    ng, nd, ndg = float(np.sqrt(np.sum(gp * gp))), float(np.sqrt(np.sum(step * step))), float(np.sqrt(np.sum(dg * dg)))
    rel = kappa / (1.0 - eps * kappa) * (eps + (ndg / ng if ng > 0 else 0.0)) if eps * kappa < 1.0 else np.inf
    b_dec = ng * rel * nd + ndg * nd + (D + 16) * U * float(np.sum(np.abs(gp * step)))
    pp = prior_parts(prior_data)
    b_logpi = 0.0 if pp is None else (D + 16) * U * float(abs(pp[2]) + 2 * abs(logpi - pp[2]))
    return dict(step=step, chol=L, logdet=2 * np.sum(np.log(np.diag(L))), decrement=gp @ step, logpi=logpi, kappa=kappa, H=Hp,
                step_rel=rel, logdet_abs=logdet_bound(Hp, L), decrement_abs=b_dec, logpi_abs=b_logpi, step_norm=nd)


def decrement(data, prior_data, theta):
    """the Newton decrement lambda^2 of the log posterior at theta, restated in longdouble from the float32 descriptors"""
    logl, g, H = exact(data, theta)
    gp, Hp, logpi, _ = add_prior(g, H, theta, prior_data)
    return float(gp @ solve(cholesky(Hp), gp))
