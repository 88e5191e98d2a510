"""Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024) per data row,
in float64 numpy: the definition of include/nnest_hip.h nnest_glm_psis, and GLMData.pointwise's route 'host'.
BUILD-DEFINED: the reference has no such estimator.

For a data row with the terms l_s = log p(y | theta_s) over its live draws (l_s finite), r_s = -l_s, b = max r, d_s = b - r_s >= 0:
    M*    = min(cnt // 5, ceil(3 sqrt(cnt)))                   `tail_target`
    c     = the largest double whose low 40 bits are zero with #{d_s < c} <= M*: a bin edge of key(d) = the top 24 bits of the
            pattern of d, so that ties go in or out together; the tail is {d_s < c}, M its size
    body  = the others: N_body, B = sum e^-d, B2 = sum (e^-d)^2
    fit   = Zhang & Stephens' (2009) generalised-Pareto fit of the sorted exceedances e^-d - e^-c, loo::gpdfit's prior (`gpd_fit`),
            where M >= 5
    out   = {c, M, N_body, B, B2, sigma, khat, log numerator, log denominator, elpd_psis, psis_ess, flag, M*, theta_hat, 0, 0}
"""
import math

import numpy as np

SLOTS = 16
C, M, N_BODY, B, B2, SIGMA, KHAT, LOG_NUM, LOG_DEN, ELPD, ESS, FLAG, M_STAR, THETA = range(14)
F_DROPPED, F_NOFIT, F_BADK = 1, 2, 4
KEY_SHIFT = 40
MAX_DRAWS = 1 << 20          # nnest_glm_psis: all draws of one call are resident
HOST_BYTES = 1 << 26         # the [S, rows] float64 block of `psis_rows`
SMALL_K = 2.0 ** -40


def ceil3sqrt(c):
    """the smallest integer m with m^2 >= 9 c"""
    c = int(c)
    m = math.isqrt(9 * c)
    return m if m * m == 9 * c else m + 1


def tail_target(cnt):
    """M* of a row with cnt live draws"""
    cnt = int(cnt)
    return min(cnt // 5, ceil3sqrt(cnt))


def tail_cap(S):
    """the slots of a row's tail buffer, from S alone (nnest_glm_psis_tail_cap)"""
    return 1 if S <= 0 else ceil3sqrt(S)


def cutoff(d_sorted, target):
    """c: the bin edge below the draw of rank `target` (from 0) of the ascending d"""
    key = np.asarray(d_sorted[target], np.float64).view(np.uint64) >> np.uint64(KEY_SHIFT)
    return float((key << np.uint64(KEY_SHIFT)).view(np.float64))


def gpd_fit(x):
    """Zhang & Stephens' fit on the ascending exceedances x [M], M >= 5: (k, sigma, khat, theta_hat) with k the raw and khat the
    regularised shape"""
    x = np.asarray(x, np.float64)
    Mx = len(x)
    m = 30 + math.isqrt(Mx)
    xstar = x[int(math.floor(Mx / 4.0 + 0.5)) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(all='ignore'):
        theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xstar)
        kj = np.mean(np.log1p(-theta[:, None] * x[None, :]), axis=1)
        L = Mx * (np.log(-theta / kj) - kj - 1.0)
        w = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
        theta_hat = float(np.sum(theta * w))
        k = float(np.mean(np.log1p(-theta_hat * x)))
        sigma = -k / theta_hat if theta_hat != 0.0 else math.copysign(math.inf, -k) if k != 0.0 else math.nan
    return k, sigma, (k * Mx + 5.0) / (Mx + 10.0), theta_hat


def smoothed_tail(Mx, u, sigma, khat):
    """q_j, j = 1 .. M: the quantiles of the fitted distribution at p_j = (j - 1/2) / M above u, truncated at 1"""
    p = (np.arange(1, Mx + 1, dtype=np.float64) - 0.5) / Mx
    lp = np.log1p(-p)
    with np.errstate(all='ignore'):
        q = u + (-sigma * lp if abs(khat) < SMALL_K else sigma * np.expm1(-khat * lp) / khat)
    return np.where(q > 1.0, 1.0, q)


def empty_row():
    out = np.zeros(SLOTS)
    out[SIGMA], out[KHAT], out[LOG_NUM], out[LOG_DEN], out[ELPD], out[FLAG], out[THETA] = np.nan, np.inf, -np.inf, -np.inf, np.nan, F_NOFIT, np.nan
    return out


def row_from_parts(b, cnt, c, tail, n_body, Bs, B2s):
    """a row's block from its cutoff, its ascending tail d [M] and its body sums"""
    out = empty_row()
    if cnt <= 0:
        return out
    Mx = len(tail)
    out[C], out[M], out[N_BODY], out[B], out[B2], out[M_STAR] = c, Mx, n_body, Bs, B2s, tail_target(cnt)
    u = math.exp(-c)
    flag, fit = 0, False
    if Mx >= 5:
        x = (np.exp(-tail) - u)[::-1]   # (ascending)
        k, sigma, khat, theta_hat = gpd_fit(x)
        out[THETA] = theta_hat
        if np.isfinite(k):
            fit = True
            out[SIGMA], out[KHAT] = sigma, khat
        else:
            out[KHAT] = np.nan
            flag |= F_BADK
    else:
        flag |= F_NOFIT
    with np.errstate(all='ignore'):
        if fit:
            q = smoothed_tail(Mx, u, out[SIGMA], out[KHAT])      # (q_j beside x_(j): the d descending)
            num = n_body + float(np.sum(q * np.exp(tail[::-1])))
        else:
            q = np.exp(-tail)
            num = n_body + float(Mx)
        den, den2 = Bs + float(np.sum(q)), B2s + float(np.sum(q * q))
        out[LOG_NUM], out[LOG_DEN] = (math.log(num) if num > 0 else -math.inf), (math.log(den) if den > 0 else -math.inf)
        out[ELPD] = (-b + out[LOG_NUM]) - out[LOG_DEN]
        out[ESS] = den * den / den2 if den2 > 0 else 0.0
    out[FLAG] = flag
    return out


def psis_rows(l, return_tails=False, block_bytes=HOST_BYTES):
    """the per-row blocks [n, 16] float64 from the terms l [S, n] (NaN or +-inf: a dead pair), in blocks of data rows so that memory
    stays bounded; with return_tails also the list of the rows' ascending tails d"""
    l = np.asarray(l, np.float64)
    if l.ndim != 2:
        raise ValueError('psis_rows: l must be shaped [S, n], got %s' % (l.shape,))
    S, n = l.shape
    out = np.empty((n, SLOTS))
    tails = []
    step = max(1, int(block_bytes // (8 * max(S, 1))))
    for first in range(0, n, step):
        blk = l[:, first:first + step]
        live = np.isfinite(blk)
        cnt = live.sum(axis=0)
        with np.errstate(invalid='ignore'):
            r = np.where(live, -blk, -np.inf)
            b = r.max(axis=0, initial=-np.inf)
            d = np.where(live, np.where(np.isfinite(b), b, 0.0) - r, np.inf)   # (dead pairs sort behind every live one)
        ds = np.sort(d, axis=0)
        for col in range(blk.shape[1]):
            i = first + col
            if cnt[col] == 0:
                out[i] = empty_row()
                tails.append(np.zeros(0))
                continue
            dcol = ds[:cnt[col], col]
            c = cutoff(dcol, tail_target(cnt[col]))
            Mx = int(np.searchsorted(dcol, c, side='left'))
            tail = dcol[:Mx].copy()
            dl = d[live[:, col], col]
            e = np.exp(-dl[dl >= c])     # (the body in the order of the draws)
            out[i] = row_from_parts(float(b[col]), int(cnt[col]), c, tail, float(len(e)), float(np.sum(e)), float(np.sum(e * e)))
            tails.append(tail)
    return (out, tails) if return_tails else out


def pareto_k_threshold(S):
    """loo's threshold of a reliable khat for S draws: min(1 - 1 / log10(S), 0.7)"""
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else 0.0
