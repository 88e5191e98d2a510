"""A numpy restatement of the pointwise predictive statistics of the regression likelihoods (include/nnest_hip.h nnest_glm_pointwise,
nnest_glm_predict) and the a-priori bounds on what any legal evaluation may differ from float64 by.

The definition, on float32 draws t [S, D] and the float32 descriptor: eta_is in float32 in the evaluator's own order, l_is in float64
from it (tests/glm_check.py `terms`), and per data row over the live draws (l_is finite)
    stats[i] = {a = max l, P = sum e^(l - a), b = max -l, Q = sum e^(-l - b), Q2 = sum e^(2 (-l - b)), cnt, mean, M2}
(nnest_glm_predict: {cnt, mean, M2} of mu_js = 1 / (1 + exp(-eta)) or exp(eta)).  What is compared is what the statistics are for:
    lppd = a + log P - log cnt,   elpd_isloo = -(b + log Q - log cnt),   mean,   var = M2 / (cnt - 1),   isloo_ess = Q^2 / Q2.

The bounds, from tests/glm_check.py's pieces (e_is = `eta_error`, lip_is = `lipschitz`), with S the number of draws:
    delta_is = lip_is e_is + 16 2^-53 (|l_is| + |y_i eta_is| + [poisson] exp(eta_is))      one term: the float32 eta, then float64
    Delta_i  = max_s delta_is
    R_i      = (S + 64) 2^-52 (1 + max_s |l_is|)                                            the float64 reduction over S draws
    a, b:                      Delta_i      (a maximum is 1-Lipschitz in the sup norm)
    lppd, elpd_isloo, mean:    Delta_i + R_i   (log-mean-exp and the mean are 1-Lipschitz in the sup norm)
    var:                       (2 sd_i Delta_i + Delta_i^2) S / (S - 1) + R_i (1 + var_i)
                               (the centred vector moves by at most Delta_i per entry in the sup norm, so its 2-norm by sqrt(S) Delta_i)
    isloo_ess:                 relative expm1(4 Delta_i) + R_i   (every weight moves by a factor within e^(+-Delta_i): Q^2 by
                               e^(+-2 Delta_i), Q2 likewise)
    cnt:                       exact
For nnest_glm_predict the same construction with the inverse link in the term's place: |d mu / d eta| <= 1/4 (logistic),
<= exp(eta + e) (poisson), and 16 2^-53 |mu| for the float64 part."""
import numpy as np

from tests import glm_check

SLOTS = ('a', 'P', 'b', 'Q', 'Q2', 'cnt', 'mean', 'M2')


def empty(n, slots=8):
    out = np.zeros((n, slots))
    if slots == 8:
        out[:, 0] = out[:, 2] = -np.inf
    return out


def _shifted(v, live):
    m = np.max(np.where(live, v, -np.inf), axis=0, initial=-np.inf)
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.where(live, np.exp(np.where(live, v, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
    return m, e.sum(axis=0), (e * e).sum(axis=0)


def moments(v, live):
    """(cnt, mean, M2) [n] of the live entries of v [S, n]: two passes in float64"""
    cnt = live.sum(axis=0).astype(np.float64)
    safe = np.where(cnt > 0, cnt, 1.0)
    v0 = np.where(live, v, 0.0)
    mean = v0.sum(axis=0) / safe
    M2 = np.where(live, (v0 - mean) ** 2, 0.0).sum(axis=0)
    return cnt, np.where(cnt > 0, mean, 0.0), np.where(cnt > 0, M2, 0.0)


def stats(l):
    """the eight statistics [n, 8] from the terms l [S, n] float64 (glm_check.exact's `l`, or a restatement's)"""
    l = np.asarray(l, np.float64)
    live = np.isfinite(l)
    out = empty(l.shape[1])
    out[:, 0], out[:, 1], _ = _shifted(l, live)
    out[:, 2], out[:, 3], out[:, 4] = _shifted(-l, live)
    out[:, 5], out[:, 6], out[:, 7] = moments(l, live)
    return out


def predict_stats(mu, eta):
    """{cnt, mean, M2} [n, 3] of the inverse link mu [S, n]; live where eta and mu are finite"""
    return np.stack(moments(mu, np.isfinite(eta) & np.isfinite(mu)), axis=1)


def inverse_link(family, eta):
    with np.errstate(invalid='ignore', over='ignore'):
        mu = 1.0 / (1.0 + np.exp(-eta)) if family == 'logistic' else np.exp(eta)
    return np.where(np.isfinite(eta), mu, np.nan)


def merge(p, q):
    """the statistics of the union of two sets of draws ([n, 8] or [n, 3]): the sums rescaled to the common maximum, Chan's rule for
    (cnt, mean, M2)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    out = np.empty_like(p)
    k = p.shape[1] - 3
    with np.errstate(invalid='ignore'):
        for m, sums, powers in ((0, (1,), (1,)), (2, (3, 4), (1, 2))) if k else ():
            top = np.maximum(p[:, m], q[:, m])
            ep = np.where(p[:, m] == top, 1.0, np.exp(p[:, m] - top))
            eq = np.where(q[:, m] == top, 1.0, np.exp(q[:, m] - top))
            out[:, m] = top
            for s, w in zip(sums, powers):
                out[:, s] = p[:, s] * ep ** w + q[:, s] * eq ** w
    n1, m1, v1, n2, m2, v2 = p[:, k], p[:, k + 1], p[:, k + 2], q[:, k], q[:, k + 1], q[:, k + 2]
    n = n1 + n2
    safe = np.where(n > 0, n, 1.0)
    d = m2 - m1
    out[:, k] = n
    out[:, k + 1] = np.where(n1 == 0, m2, np.where(n2 == 0, m1, (n1 * m1 + n2 * m2) / safe))
    out[:, k + 2] = np.where(n1 == 0, v2, np.where(n2 == 0, v1, (v1 + v2) + d * d * (n1 * n2 / safe)))
    return out


def derived(st):
    """what is compared: dict of [n] arrays from the statistics [n, 8] (or [n, 3]: cnt, mean, var only)"""
    st = np.asarray(st, np.float64)
    k = st.shape[1] - 3
    cnt, mean, M2 = st[:, k], st[:, k + 1], st[:, k + 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        out = dict(cnt=cnt, mean=mean, var=np.where(cnt >= 2, M2 / np.where(cnt >= 2, cnt - 1.0, 1.0), np.nan))
        if k:
            a, P, b, Q, Q2 = st[:, :5].T
            out.update(a=a, b=b, lppd=a + np.log(P) - np.log(cnt), elpd_isloo=-(b + np.log(Q) - np.log(cnt)),
                       isloo_ess=np.where(Q2 > 0, Q * Q / np.where(Q2 > 0, Q2, 1.0), 0.0))
    return out


def _bounds(delta, val, S):
    """from delta_is [S, n] and the exact values val [S, n] (every pair live)"""
    Delta = np.max(delta, axis=0)
    R = (S + 64) * 2.0 ** -52 * (1.0 + np.max(np.abs(val), axis=0))
    var = np.var(val, axis=0, ddof=1) if S > 1 else np.zeros(val.shape[1])
    out = dict(a=Delta, b=Delta, lppd=Delta + R, elpd_isloo=Delta + R, mean=Delta + R, cnt=np.zeros_like(Delta),
               isloo_ess_rel=np.expm1(4.0 * Delta) + R, Delta=Delta)
    out['var'] = (2.0 * np.sqrt(var) * Delta + Delta ** 2) * S / (S - 1.0) + R * (1.0 + var) if S > 1 else np.full_like(Delta, np.nan)
    return out


def pointwise_bounds(family, y, eta, l, e):
    """the bounds of nnest_glm_pointwise: y [n], the exact eta and l [S, n], and e [S, n] what the evaluated eta may be off by"""
    with np.errstate(invalid='ignore', over='ignore'):
        lip = np.ones_like(eta) if family == 'logistic' else np.abs(y) + np.exp(eta + e)
        mag = np.abs(l) + np.abs(y * eta) + (np.exp(eta) if family == 'poisson' else 0.0)
    return _bounds(lip * e + 16 * 2.0 ** -53 * mag, l, eta.shape[0])


def predict_bounds(family, eta, mu, e):
    """the bounds of nnest_glm_predict (cnt, mean and var are what it has)"""
    with np.errstate(invalid='ignore', over='ignore'):
        lip = np.full_like(eta, 0.25) if family == 'logistic' else np.exp(eta + e)
    return _bounds(lip * e + 16 * 2.0 ** -53 * np.abs(mu), mu, eta.shape[0])


def data_bounds(data, t):
    """pointwise_bounds for a descriptor `data` (GLMData.hip_like_glm) and float32 draws t: (bounds, exact statistics [n, 8])"""
    n, A, y, o = glm_check._parts(data)
    _, eta, l = glm_check.exact(data, t)
    return pointwise_bounds(data['family'], y, eta, l, glm_check.eta_error(data, t)), stats(l)


def data_predict_bounds(data, t):
    """predict_bounds likewise: (bounds, exact statistics [n, 3])"""
    _, eta, _ = glm_check.exact(data, t)
    mu = inverse_link(data['family'], eta)
    return predict_bounds(data['family'], eta, mu, glm_check.eta_error(data, t)), predict_stats(mu, eta)


def shares(got, want, bounds):
    """the share of its bound each compared quantity takes: {name: max_i |got - want| / bound} (cnt: the largest difference
    itself, which must be 0).  `got`, `want`: statistics [n, 8] or [n, 3]"""
    g, w = derived(got), derived(want)
    out = {}
    for k in w:
        if k == 'cnt':
            out[k] = float(np.max(np.abs(g[k] - w[k])))
        elif k == 'isloo_ess':
            out[k] = float(np.max(np.abs(g[k] - w[k]) / (w[k] * bounds['isloo_ess_rel'])))
        elif k == 'var' and not np.all(np.isfinite(w[k])):
            assert np.array_equal(np.isnan(g[k]), np.isnan(w[k]))   # (fewer than two live draws: no variance on either side)
        else:
            out[k] = float(np.max(np.abs(g[k] - w[k]) / bounds[k]))
    return out


def float32_eta(data, t, order):
    """eta [S, ld] with the sum in float32 numpy, `forward` (o_i, then c = 0 .. D - 1), `reversed` (c = D - 1 .. 0, then o_i) or
    `pairwise` (a balanced tree over the D products and o_i); the products are rounded (no fused multiply-add in numpy).  It reads
    the PADDED arrays: the caller masks the rows i >= n"""
    at, o = np.asarray(data['at'], np.float32), np.asarray(data['o'], np.float32)
    t = np.asarray(t, np.float32)
    D, ld = at.shape
    prods = [np.outer(t[:, c], at[c]).astype(np.float32) for c in range(D)]
    off = np.broadcast_to(o, (len(t), ld)).astype(np.float32)
    if order == 'pairwise':
        v = prods + [off]
        while len(v) > 1:
            nxt = [(v[i] + v[i + 1]).astype(np.float32) for i in range(0, len(v) - 1, 2)]
            if len(v) % 2:
                nxt.append(v[-1])
            v = nxt
        return v[0]
    seq = [off] + prods if order == 'forward' else prods[::-1] + [off]
    eta = seq[0]
    for v in seq[1:]:
        eta = (eta + v).astype(np.float32)
    return eta


def float32_stats(data, t, order, predict=False):
    """the statistics with eta from `float32_eta`, the terms (or the inverse link) and the reduction in float64"""
    n = int(data['n'])
    eta = float32_eta(data, t, order)[:, :n].astype(np.float64)
    if predict:
        return predict_stats(inverse_link(data['family'], eta), eta)
    return stats(glm_check.terms(data['family'], eta, np.asarray(data['y'], np.float32)[:n].astype(np.float64)))


def draws(S, D, seed):
    """the tests' draws: N(0, 1) U(0.2, 1.0) per row, float32"""
    r = np.random.RandomState(seed)
    return (r.standard_normal((S, D)) * r.uniform(0.2, 1.0, (S, 1))).astype(np.float32)
