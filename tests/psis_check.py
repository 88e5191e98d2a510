"""An independent restatement of Pareto-smoothed leave-one-out (include/nnest_hip.h nnest_glm_psis; nnest_amd/psis.py; DESIGN.md
3.19) in np.longdouble, planted-fault variants of it, and the distance the GPU tests compare by.

The SELECTION is defined to the bit -- d = b - (-l) in float64, the cutoff a bin edge of the top 24 bits of d's pattern, the tail the
draws below it -- and is restated here in float64 with a stable argsort and a scan, not with nnest_amd/psis.py's search.  The FIT and
the SMOOTHED SUMS are restated row by row in long double with plain loops over the grid: what float64 in any summation order may
differ from them by is the scale of the GPU tests' tolerance (F64_VS_LD below).

Faults (`fault=`): 'unregularised' -- khat = k without the prior's (k M + 5) / (M + 10); 'tail_bin' -- the cutoff one bin higher;
'no_truncation' -- the smoothed weights not capped at 1."""
import math

import numpy as np

from tests import glm_check, glm_pointwise_check

LD = np.longdouble
FAULTS = ('unregularised', 'tail_bin', 'no_truncation')
QUANTITIES = ('khat', 'sigma', 'elpd', 'ess')

# the worst distance (`distance` below) of nnest_amd/psis.py's float64 from this long double over `gpu_cases()`: measured 4.13e-12
# (khat, logistic x_dim 33, n 70, S 25: five tail values), which tests/test_psis_check.py holds under this figure.  The GPU tests allow
# 8 x, with a floor of 1e-13.
F64_VS_LD = 4.2e-12
GPU_TOL = max(8 * F64_VS_LD, 1e-13)

WIDTHS = (5, 33, 65, 128)
ROWS = (1, 17, 70)
DRAWS = (1, 17, 24, 25, 1003, 4001)


def tail_target(cnt):
    m = 0
    while m * m < 9 * cnt:   # (the smallest m with m^2 >= 9 cnt)
        m += 1
    return min(cnt // 5, m)


def key_of(d):
    return int(np.float64(d).view(np.uint64)) >> 40


def edge_of(key):
    return float(np.uint64(key << 40).view(np.float64))


def select(lcol, fault=None):
    """(b, cnt, c, tail ascending, body in draw order) of one row's terms"""
    l = np.asarray(lcol, np.float64)
    l = l[np.isfinite(l)]
    cnt = len(l)
    if cnt == 0:
        return -np.inf, 0, 0.0, np.zeros(0), np.zeros(0)
    b = np.max(-l)
    d = b - (-l)
    target = tail_target(cnt)
    order = np.argsort(d, kind='stable')
    key = key_of(d[order[target]])
    if fault == 'tail_bin':
        key += 1
    c = edge_of(key)
    tail = np.array([d[k] for k in order if d[k] < c])
    return b, cnt, c, tail, d[d >= c]


def row(lcol, fault=None):
    """the row's results in long double: dict(c, M, n_body, B, B2, sigma, khat, elpd, ess, tail)"""
    b, cnt, c, tail, body = select(lcol, fault)
    M = len(tail)
    out = dict(c=c, M=M, n_body=len(body), tail=tail, sigma=np.nan, khat=np.inf, elpd=np.nan, ess=0.0, B=0.0, B2=0.0, target=tail_target(cnt))
    if cnt == 0:
        return out
    e = np.exp(-body.astype(LD))
    Bs, B2s = np.sum(e), np.sum(e * e)
    u = np.exp(-LD(c))
    td = tail.astype(LD)
    fit = False
    if M >= 5:
        x = (np.exp(-td) - u)[::-1]
        m = 30 + int(math.isqrt(M))
        xstar = x[int(math.floor(M / 4.0 + 0.5)) - 1]
        theta, L = [], []
        for j in range(1, m + 1):
            th = LD(1) / x[-1] + (LD(1) - np.sqrt(LD(m) / (LD(j) - LD(0.5)))) / (LD(3) * xstar)
            kj = np.sum(np.log1p(-th * x)) / LD(M)
            theta.append(th)
            L.append(LD(M) * (np.log(-th / kj) - kj - LD(1)))
        theta, L = np.array(theta, LD), np.array(L, LD)
        with np.errstate(over='ignore'):
            w = LD(1) / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
        that = np.sum(theta * w)
        k = np.sum(np.log1p(-that * x)) / LD(M)
        if np.isfinite(k):
            fit = True
            sigma = -k / that
            khat = k if fault == 'unregularised' else (k * LD(M) + LD(5)) / (LD(M) + LD(10))
            out['sigma'], out['khat'] = float(sigma), float(khat)
        else:
            out['khat'] = np.nan
    if fit:
        lp = np.log1p(-(np.arange(1, M + 1).astype(LD) - LD(0.5)) / LD(M))
        q = u + (-sigma * lp if abs(khat) < 2.0 ** -40 else sigma * np.expm1(-khat * lp) / khat)
        if fault != 'no_truncation':
            q = np.where(q > 1, LD(1), q)
        num, den, den2 = LD(len(body)) + np.sum(q * np.exp(td[::-1])), Bs + np.sum(q), B2s + np.sum(q * q)
    else:
        q = np.exp(-td)
        num, den, den2 = LD(len(body) + M), Bs + np.sum(q), B2s + np.sum(q * q)
    out['B'], out['B2'] = float(Bs), float(B2s)
    out['elpd'] = float((-LD(b) + np.log(num)) - np.log(den))
    out['ess'] = float(den * den / den2) if den2 > 0 else 0.0
    return out


def rows(l, fault=None):
    return [row(l[:, i], fault) for i in range(l.shape[1])]


def _dist(a, b):
    a, b = float(a), float(b)
    if (np.isnan(a) and np.isnan(b)) or a == b:
        return 0.0
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    return abs(a - b) / max(1.0, abs(b))


def distance(block, want):
    """the worst |got - want| / max(1, |want|) of khat, sigma, elpd_psis and psis_ess between nnest_glm_psis's blocks [n, 16] and a
    list of `row` dicts (inf where one side is finite and the other is not): {quantity: worst}"""
    from nnest_amd import psis
    slots = dict(khat=psis.KHAT, sigma=psis.SIGMA, elpd=psis.ELPD, ess=psis.ESS)
    return {q: max([_dist(block[i, slots[q]], w[q]) for i, w in enumerate(want)], default=0.0) for q in QUANTITIES}


def block_of(want):
    """`row` dicts as blocks [n, 16] (the slots `distance` reads, and c, M, N_body, B, B2)"""
    from nnest_amd import psis
    out = np.zeros((len(want), psis.SLOTS))
    for i, w in enumerate(want):
        for k, s in (('c', psis.C), ('M', psis.M), ('n_body', psis.N_BODY), ('B', psis.B), ('B2', psis.B2), ('sigma', psis.SIGMA),
                     ('khat', psis.KHAT), ('elpd', psis.ELPD), ('ess', psis.ESS)):
            out[i, s] = w[k]
    return out


def host_terms(data, t):
    """the terms [S, n] of a descriptor over float32 draws with eta summed forward in float32: the device's definition up to the order
    of its sum (what the CPU tests stand in for the device's own matrix with)"""
    n = int(data['n'])
    eta = glm_pointwise_check.float32_eta(data, t, 'forward')[:, :n].astype(np.float64)
    return glm_check.terms(data['family'], eta, np.asarray(data['y'], np.float32)[:n].astype(np.float64))


def gpu_cases():
    """the (family, D, n, S, seed) of the GPU tests' selection and fit cases: every width, row count and S"""
    for family in glm_check.FAMILIES:
        for D in WIDTHS:
            for n in ROWS:
                for S in DRAWS:
                    yield family, D, n, S, 7 * D + n + S


def case_data(family, D, n):
    return glm_check.make_like(D, n, family, D + n).hip_like_glm


def outlier_case(seed, S=40000, n=30):
    """the front ends' construction: 1-D logistic regression, 30 rows, row 0 at A = 4 with y = 0 against the trend of the others,
    and S draws from the exact posterior (flat prior) by inverse CDF on a grid.  Returns (A [n, 1], y [n], theta [S, 1])"""
    rng = np.random.RandomState(seed)
    A = np.concatenate([[4.0], rng.uniform(-1.0, 1.0, n - 1)])[:, None]
    p = 1.0 / (1.0 + np.exp(-1.5 * A[:, 0]))
    y = (rng.uniform(size=n) < p).astype(np.float64)
    y[0] = 0.0
    grid = np.linspace(-6.0, 10.0, 64001)
    s = (1.0 - 2.0 * y)[None, :] * (grid[:, None] * A[:, 0][None, :])
    logp = -np.sum(np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))), axis=1)
    w = np.exp(logp - logp.max())
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    theta = np.interp(rng.uniform(size=S), cdf, grid)
    return A, y, theta[:, None]
