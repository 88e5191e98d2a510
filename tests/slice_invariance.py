"""Invariance harness for the slice proposal (include/nnest_hip.h nnest_slice_steps and the kernels that share its definition).

The slice update under a hard constraint has a target that does not depend on its own code: for any flow, likelihood and threshold
L*, x = f^-1(z) must stay uniform on A = {x in [-1, 1]^D : logL(x) > L*} -- the |det dx/dz| factor of the slice level exists to make
this true.  So a correct update started from an exact uniform sample of A

1. keeps it (stationarity): after S updates the walkers and a fresh, independent sample of A have the same distribution;
2. is reversible (detailed balance): from stationarity the pair (x before, x after one update) is exchangeable, so the joint
   histogram of a scalar projection s(x) before and after is symmetric, H = H^T.

Neither statistic knows how the update works; they compare the kernels with the definition of a correct MCMC update, not with a
restatement of it.  The exact start is drawn on the host by rejection in float64 (seeded), so every test is deterministic.

Significance: every test makes one decision at ALPHA after a Bonferroni correction over its statistics (`assert_invariant`).

`slice_update` is a vectorised float64 statement of univariate slice sampling with an identity flow, with the stepping-out budget
kept within a total budget, split at random when the full step-out exceeds it (Neal 2003, sec. 4.1; the rule the kernels
follow), or capped per side (the rule they followed before).  It lets the
CPU suite check that the statistics here can tell the two apart (tests/test_slice_invariance_power.py).
"""
import numpy as np
from scipy import stats

ALPHA = 1e-6   # per test, after a Bonferroni correction over the test's statistics


def uniform_on(rng, n, D, inside=None, batch=1 << 16):
    """n points uniform on A = {x in [-1, 1]^D : inside(x)} by rejection, float64 (inside: x [m, D] float64 -> bool [m]; None = box)"""
    out, have = [], 0
    while have < n:
        u = rng.uniform(-1.0, 1.0, size=(batch, D))
        if inside is not None:
            u = u[inside(u)]
        out.append(u)
        have += u.shape[0]
    return np.concatenate(out)[:n]


def two_sample_chi2(a, b, edges):
    """binned two-sample chi^2 of equal-size samples a, b (1-D) on `edges`: sum (A_i - B_i)^2 / (A_i + B_i) -> (stat, dof)"""
    assert a.shape == b.shape
    ha, _ = np.histogram(a, edges)
    hb, _ = np.histogram(b, edges)
    n = ha + hb
    k = n > 0
    return float(np.sum((ha[k] - hb[k]) ** 2 / n[k])), int(k.sum()) - 1


def two_sample_chi2_2d(a, b, edges):
    """the same on a 2-D grid: a, b [n, 2]"""
    assert a.shape == b.shape
    ha, _, _ = np.histogram2d(a[:, 0], a[:, 1], [edges, edges])
    hb, _, _ = np.histogram2d(b[:, 0], b[:, 1], [edges, edges])
    n = ha + hb
    k = n > 0
    return float(np.sum((ha[k] - hb[k]) ** 2 / n[k])), int(k.sum()) - 1


def projections(D, seed, k):
    """k fixed random unit vectors of R^D"""
    v = np.random.RandomState(seed).standard_normal((k, D))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def box_depth(x):
    """the distance of x to the surface of the box, min_d (1 - |x_d|): where a capped stepping-out shows its bias"""
    return 1.0 - np.max(np.abs(x), axis=1)


def stationarity_pvalues(x, fresh, scalars=(box_depth,), bins=20, seed=12345):
    """x: the walkers after the updates; fresh: an independent uniform sample of A of the same size.  p-values of the per-coordinate
    binned chi^2 (bins on [-1, 1]), of a 2-D binned chi^2 on a fixed random pair of projections (bins on the pooled range), and of a
    binned chi^2 of each scalar statistic in `scalars` (x [n, D] -> [n]; 40 bins at the quantiles of the fresh sample)."""
    x, fresh = np.asarray(x, np.float64), np.asarray(fresh, np.float64)
    assert x.shape == fresh.shape
    N, D = x.shape
    edges = np.linspace(-1.0, 1.0, bins + 1)
    p = {}
    for d in range(D):
        s, dof = two_sample_chi2(x[:, d], fresh[:, d], edges)
        p['x%d' % d] = stats.chi2.sf(s, dof)
    v = projections(D, seed, 2)
    a, b = x @ v.T, fresh @ v.T
    lo, hi = np.minimum(a.min(0), b.min(0)).min(), np.maximum(a.max(0), b.max(0)).max()
    nb = int(min(bins, max(4, np.sqrt(N / 50.0))))   # >= ~50 expected counts per cell in the bulk
    s, dof = two_sample_chi2_2d(a, b, np.linspace(lo, hi + 1e-12, nb + 1))
    p['proj2d'] = stats.chi2.sf(s, dof)
    for f in scalars:
        sa, sb = f(x), f(fresh)
        e = np.unique(np.quantile(sb, np.linspace(0.0, 1.0, 41)))
        e[0], e[-1] = -np.inf, np.inf
        s, dof = two_sample_chi2(sa, sb, e)
        p[f.__name__] = stats.chi2.sf(s, dof)
    return p


def bowker(s0, s1, edges, min_count=10):
    """Bowker's test of symmetry of the joint histogram H of (s0, s1): sum over i < j with H_ij + H_ji >= min_count of
    (H_ij - H_ji)^2 / (H_ij + H_ji) -> (stat, dof)"""
    h, _, _ = np.histogram2d(s0, s1, [edges, edges])
    iu = np.triu_indices(h.shape[0], 1)
    a, b = h[iu], h.T[iu]
    n = a + b
    k = n >= min_count
    return float(np.sum((a[k] - b[k]) ** 2 / n[k])), int(k.sum())


def exchangeability_pvalues(x0, x1, scalars=(box_depth,), seed=54321, k=2, max_bins=64):
    """(x0, x1): the walkers before and after ONE update, x0 exactly uniform on A.  For k fixed random unit projections s(x) and each
    scalar statistic in `scalars`, Bowker's symmetry test on the joint histogram of (s(x0), s(x1)), in bins as wide as the median
    |s(x1) - s(x0)| of the walkers that moved (a bin comparable to the move: much coarser bins see no move at all).  The bin width and
    range are symmetric functions of the pair, so under exchangeability they do not bias the statistic."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    assert x0.shape == x1.shape
    fs = [('proj%d' % i, (lambda v: lambda x: x @ v)(v)) for i, v in enumerate(projections(x0.shape[1], seed, k))]
    fs += [(f.__name__, f) for f in scalars]
    p = {}
    for name, f in fs:
        s0, s1 = f(x0), f(x1)
        ds = np.abs(s1 - s0)
        h = float(np.median(ds[ds > 0])) if np.any(ds > 0) else 1.0
        lo, hi = min(s0.min(), s1.min()), max(s0.max(), s1.max()) + 1e-12
        h = max(h, (hi - lo) / max_bins)
        nb = int(np.ceil((hi - lo) / h))
        s, dof = bowker(s0, s1, lo + h * np.arange(nb + 1))
        p['bowker_' + name] = stats.chi2.sf(s, dof) if dof > 0 else 1.0
    return p


def assert_invariant(pvals, alpha=ALPHA, what=''):
    """one decision per test: the smallest p-value, Bonferroni-corrected over the test's statistics, must exceed alpha"""
    m = len(pvals)
    worst = min(pvals, key=pvals.get)
    assert pvals[worst] * m > alpha, '%s: %s p=%.3g (x %d statistics) <= %g' % (what, worst, pvals[worst], m, alpha)


def min_corrected_p(pvals):
    return min(pvals.values()) * len(pvals)


def stepout_split(v, max_stepout):
    """the randomised split of the stepping-out budget B = 2 max_stepout (Neal 2003, sec. 4.1): J = min(B, floor(v (B + 1))) steps to
    the left, K = B - J to the right; v is a 24-bit uniform, so the product is exact in float64"""
    B = 2 * int(max_stepout)
    J = np.minimum(B, np.floor(np.asarray(v, np.float64) * (B + 1))).astype(np.int64)
    return J, B - J


def slice_update(rng, x, width, max_stepout, inside=None, rule='budget', max_shrink=32):
    """one univariate slice-sampling update of every row of x (float64, identity flow) along a random direction, on the uniform target
    of A = {x in [-1, 1]^D : inside(x)}: bracket [-u0, 1 - u0] in units of width * eps, stepping out, then shrinkage.  Stepping out,
    rule 'budget' (the kernels'): to the first point outside on each side if that takes at most B = 2 max_stepout expansions in all,
    else restarted with B split at random, J / B - J steps at most; rule 'cap' (their earlier one): at most max_stepout per side.
    Returns the new x."""
    N, D = x.shape
    e = rng.standard_normal((N, D))
    u0 = rng.uniform(size=N)
    v = np.floor(rng.uniform(size=N) * (1 << 24)) / (1 << 24)

    def ok(t, rows):
        xp = x[rows] + (t * width)[:, None] * e[rows]
        r = np.all(np.abs(xp) <= 1.0, axis=1)
        if inside is not None:
            r &= inside(xp)
        return r

    def step_out(tl, tr, nl, nr):   # at most nl / nr expansions, each side to its first point outside
        for t, n, sgn in ((tl, nl, -1.0), (tr, nr, 1.0)):
            live = n > 0
            j = 0
            while live.any():
                rows = np.flatnonzero(live)
                good = ok(t[rows], rows)
                t[rows[good]] += sgn
                j += 1
                live[rows[~good]] = False
                live &= n > j
        return tl, tr

    B = 2 * int(max_stepout)
    if rule == 'cap':
        tl, tr = step_out(-u0, 1.0 - u0, np.full(N, B // 2), np.full(N, B // 2))
    else:
        tl, tr = step_out(-u0, 1.0 - u0, np.full(N, B + 1), np.full(N, B + 1))
        over = (tr - tl - 1.0) > B + 0.5   # more than B expansions in all (a side that reached B + 1 counts so)
        rows = np.flatnonzero(over)
        if rows.size:
            J, K = stepout_split(v[rows], max_stepout)
            sub_tl, sub_tr = np.full(N, np.nan), np.full(N, np.nan)
            nl, nr = np.zeros(N, np.int64), np.zeros(N, np.int64)
            sub_tl[rows], sub_tr[rows] = -u0[rows], 1.0 - u0[rows]
            nl[rows], nr[rows] = J, K
            sub_tl, sub_tr = step_out(sub_tl, sub_tr, nl, nr)
            tl[rows], tr[rows] = sub_tl[rows], sub_tr[rows]
    out = x.copy()
    live = np.ones(N, bool)
    for _ in range(max_shrink):
        rows = np.flatnonzero(live)
        if rows.size == 0:
            break
        t = tl[rows] + (tr[rows] - tl[rows]) * rng.uniform(size=rows.size)
        good = ok(t, rows)
        g = rows[good]
        out[g] = x[g] + (t[good] * width)[:, None] * e[g]
        live[g] = False
        b = rows[~good]
        tb = t[~good]
        neg = tb < 0
        tl[b[neg]] = tb[neg]
        tr[b[~neg]] = tb[~neg]
    return out
