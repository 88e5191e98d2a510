"""The likelihoods of the fused ensemble, random-walk and importance kernels (nnest_ensemble_*, nnest_ensemble_x_*, nnest_mcmc_steps,
nnest_importance_evidence and their spline counterparts), checked as a kernel against ITSELF plus an exact function of its own
output: logL of a row against the float64 oracle on T(x) of the x the kernel stored beside it, lp - logL against the oracle's
log-det.  The flow's conditioning therefore never enters a likelihood tolerance.  numpy only: no GPU, no torch device.

LIKES: per likelihood its id, the parameters the tests give it, the x_dim it takes and the recipes affine(D, seed) -> (t_std, t_mean)
that put T(x) where the likelihood is informative for x ~ 0.5 N(0, 1).  `restated32` restates the kernels' float32 term arithmetic in
the two register layouts (solo_loglike.h, flow_tile.h loglike_tile); the CPU suite (tests/test_fused_like_check.py) uses it to show
that each bound can be met -- worst error at most half of it -- and to plant the faults the checks must catch.  The GPU tests do not
call it.

BOUND on logL: 2e-5 + 1e-6 |v|, the figure in force for this evaluator (tests/test_gpu_ensemble.py, tests/test_gpu_mcmc_walk.py).  The
restatement's worst error over the GPU tables' x_dim, both layouts, 2000 rows each, as a share of the bound, stands beside each entry
of LIKES (`restated`); none needs more than half, so every likelihood keeps the figure."""
import numpy as np

from tests.ensemble_check import latent_target, split_sets, stretch_step   # noqa: F401  (re-exported for the GPU tests)
from tests.ensemble_moves_check import DE, STRETCH, de_gamma0, moves_step
from tests.mcmc_walk_check import _counters, philox4x32_10

SAFE = -1e100   # sampler.py:128: logl[~isfinite] = -1e100


def logl_bound(v):
    return 2e-5 + 1e-6 * np.abs(np.asarray(v, np.float64))


# ---- the recipes -------------------------------------------------------------------------------------------------------------------
def _wide(D, seed, x_sd=0.5):
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D) * (0.5 / x_sd), r.uniform(-0.3, 0.3, D)


def _valley(D, seed, x_sd=0.5):
    r = np.random.RandomState(seed)
    return 0.15 * r.uniform(0.5, 1.5, D) * (0.5 / x_sd), 1.0 + 0.09 * r.uniform(-1.0, 1.0, D)


def _scaled(scale):
    def affine(D, seed, x_sd=0.5):
        r = np.random.RandomState(seed)
        return scale * r.uniform(0.5, 1.5, D) * (0.5 / x_sd), r.uniform(-0.3, 0.3, D)
    return affine


def _on_shell(radius, centre):
    """|T(x) - centre 1| about `radius`: |x| is about 0.5 sqrt(D)"""
    def affine(D, seed, x_sd=0.5):
        r = np.random.RandomState(seed)
        c = centre if np.isscalar(centre) else centre[seed & 1]
        return radius / (x_sd * np.sqrt(D)) * r.uniform(0.9, 1.1, D), c + r.uniform(-0.03, 0.03, D)
    return affine


def _f32pair(fn):
    def affine(D, seed, x_sd=0.5):
        sd, mu = fn(D, seed, x_sd)
        return np.asarray(sd, np.float32), np.asarray(mu, np.float32)
    return affine


# id: _lib.LIKE_IDS (tests/test_fused_like_check.py holds the two together); dims: the x_dim the likelihood takes;
# restated: the float32 restatement's worst error / bound (solo layout, tile layout) measured by tests/test_fused_like_check.py
LIKES = {
    'rosenbrock': dict(id=0, params=(), dims=lambda D: D >= 2, recipes=dict(wide=_f32pair(_wide), valley=_f32pair(_valley)),
                       restated=(0.23, 0.28)),
    'gaussmix': dict(id=1, params=(), dims=lambda D: D >= 2, recipes=dict(main=_f32pair(_scaled(10.0))), restated=(0.14, 0.13)),
    'himmelblau': dict(id=2, params=(), dims=lambda D: D >= 2 and D % 2 == 0, recipes=dict(main=_f32pair(_scaled(5.0))),
                       restated=(0.28, 0.28)),
    'gaussian': dict(id=3, params=(0.5,), dims=lambda D: D >= 1, recipes=dict(main=_f32pair(_wide)), restated=(1e-7, 1e-7)),
    'eggbox': dict(id=4, params=(), dims=lambda D: D == 2, recipes=dict(main=_f32pair(_scaled(15.0))), restated=(0.34, 0.34)),
    'shell': dict(id=5, params=(0.1, 2.0, 0.0), dims=lambda D: D >= 1, recipes=dict(main=_f32pair(_on_shell(2.0, 0.0))),
                  restated=(1e-7, 1e-7)),
    # (the recipe sits on the first shell for an even seed, on the second for an odd one)
    'double_shell': dict(id=6, params=(0.1, 2.0, -1.0, 0.2, 1.5, 1.0), dims=lambda D: D >= 1,
                         recipes=dict(main=_f32pair(_on_shell(1.75, (-1.0, 1.0)))), restated=(1e-7, 1e-7)),
}

# the GPU tables (tests/test_gpu_fused_likes.py): every (likelihood, recipe, x_dim).  Rosenbrock: both edges of U = 1 .. 4 and the
# full-tile wrap (x_dim = 32 U: position 15's last term would read position 0).  U = NT = ceil(ceil(x_dim / 2) / 16).
TABLE = ([('rosenbrock', r, D) for D in (2, 3, 32, 33, 64, 65, 96, 97, 128) for r in ('wide', 'valley')]
         + [('gaussmix', 'main', D) for D in (2, 20, 81)] + [('himmelblau', 'main', D) for D in (2, 32, 66)]
         + [('gaussian', 'main', D) for D in (1, 7, 100)] + [('shell', 'main', D) for D in (5, 40)]
         + [('double_shell', 'main', D) for D in (5, 97)] + [('eggbox', 'main', 2)])


def units(D):
    """U of the solo layout (2 U dims per position) = NT of the tile layout (32 NT dims per walker)"""
    return ((D + 1) // 2 + 15) // 16


def affine(name, recipe, D, seed, x_sd=0.5):
    return LIKES[name]['recipes'][recipe](D, seed, x_sd)


def box_for(sd, mu, share=0.7, x_sd=0.5):
    """lo, hi on T(x), |x_d| <= k x_sd in every dimension, k such that about `share` of the rows x ~ x_sd N(0, 1) are inside"""
    from scipy.special import ndtri
    D = len(sd)
    k = float(ndtri(1.0 - 0.5 * (1.0 - share ** (1.0 / D))))
    h = np.abs(np.asarray(sd, np.float64)) * k * x_sd
    return (np.asarray(mu, np.float64) - h).astype(np.float32), (np.asarray(mu, np.float64) + h).astype(np.float32)


def T32(x, sd, mu):
    """T(x) as ens_T under fp contract(off): two rounded float32 operations"""
    return (np.asarray(x, np.float32) * np.asarray(sd, np.float32)) + np.asarray(mu, np.float32)


def in_box(tx, lo, hi):
    """the kernels' box test on T(x): a NaN coordinate counts as inside (UniformPrior, priors.py)"""
    tx = np.asarray(tx, np.float32)
    if lo is None:
        return np.ones(len(tx), bool)
    return ~np.any((tx < np.asarray(lo, np.float32)) | (tx > np.asarray(hi, np.float32)), axis=1)


def exact_logl(name, tx32, params=None):
    """the float64 oracle on the float32 T(x), with the safe rule (sampler.py:128): non-finite -> -1e100"""
    from oracle import oracle as orc
    tx = np.atleast_2d(np.asarray(tx32, np.float32)).astype(np.float64)
    out = np.asarray(orc.loglike(name, tx, 1.0, list(params) if params else None), np.float64)
    return np.where(np.isfinite(out), out, SAFE)


# ---- the kernels' float32 term arithmetic, restated ------------------------------------------------------------------------------
_F = np.float32
_MU0, _MU1 = np.array([0, 0, 4, -4], _F), np.array([4, -4, 0, 0], _F)
_LW = np.array([-0.916290731874155, -1.203972804325936, -1.6094379124341003, -2.302585092994046])
_HALF_LOG_2PI = 0.9189385332046727


def _row_sum32(v):
    """solo_row_sum: v + ror8, + ror4, + ror2, + ror1 over the 16 positions (lane p <- lane p - N); every lane ends with the same bits"""
    for n in (8, 4, 2, 1):
        v = v + np.roll(v, n, axis=1)
    return v[:, 0]


def _xor_sum64(v):
    for o in (1, 2, 4, 8):
        v = v + v[:, np.arange(16) ^ o]
    return v[:, 0]


def _wide_sum(v32):
    """group_sum_wide / group_sum as lane group 0 sees it: (v0 + v1) + (v2 + v3) in float64"""
    v = v32.astype(np.float64)
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def _rosen_term(a0, a1):
    a = a0 * a0
    b = a1 - a
    c = b * b
    e = _F(100.0) * c
    f = _F(1.0) - a0
    return e + f * f


def _himmel_term(x0, x1):
    a = x0 * x0 + x1 - _F(11.0)
    b = x0 + x1 * x1 - _F(7.0)
    return -(a * a) - b * b


def _mix_tail(base, t0, t1, D):
    l = np.empty((4, len(base)))
    for k in range(4):
        a, b = t0 - _MU0[k], t1 - _MU1[k]
        s = base + (a * a).astype(np.float64) + ((b * b).astype(np.float64) if D > 1 else 0.0)
        l[k] = -(s * 0.5) - _HALF_LOG_2PI * D + _LW[k]
    mx = l.max(0)
    se = np.zeros(len(base), _F)
    for k in range(4):
        se = se + np.exp((l[k] - mx).astype(_F))
    return mx + np.log(se).astype(np.float64)


def _moments_tail(name, s1, s2, D, p):
    Dd = float(D)
    with np.errstate(all='ignore'):
        if name == 'gaussian':
            c = float(p[0])
            quad = (s2 - c * s1 * s1 / (1.0 + (Dd - 1.0) * c)) / (1.0 - c)
            logdet = (Dd - 1.0) * np.log(1.0 - c) + np.log(1.0 + (Dd - 1.0) * c)
            return -0.5 * quad - 0.5 * logdet - _HALF_LOG_2PI * Dd
        sh = []
        for k in range(2):
            sig, rs, cen = float(p[3 * k]), float(p[3 * k + 1]), float(p[3 * k + 2])
            r2 = s2 - 2.0 * cen * s1 + Dd * cen * cen
            rad = np.sqrt(np.where(r2 < 0.0, 0.0, r2))
            sh.append(-((rad - rs) * (rad - rs)) / (2.0 * sig * sig))
        if name == 'shell':
            return sh[0]
        mx, mn = np.where(sh[0] > sh[1], sh[0], sh[1]), np.where(sh[0] > sh[1], sh[1], sh[0])
        return mx + np.log1p(np.exp(mn - mx))


FAULTS = ('boundary', 'mask', 'base', 'last_pair', 'corr', 'triple', 'nan')


def restated32(name, tx32, params=None, layout='solo', fault=None):
    """logL [N] float64 of T(x) rows tx32 [N, D] float32 in the kernels' arithmetic: the terms float32 with every operation rounded,
    summed in the layout's order.  layout 'solo' (solo_loglike.h): position m of 16 holds dims 2 U m .. 2 U m + 2 U - 1, sums them
    one after the other, then the rotate tree over the positions (the float64 moments: the xor tree).  layout 'tile' (flow_tile.h
    loglike_tile): lane group g of 4 holds dims 32 tau + 8 g .. + 7 of every tile tau, sums them one after the other, the four
    partials are added in float64.  Padded dims hold T = 0 x + 0 = 0.
    fault (FAULTS; the CPU suite's planted faults): 'boundary' drops Rosenbrock's term that reads the next position / lane group;
    'mask' sums it for i < D instead of i + 1 < D (x_dim 33: a padded neighbour; x_dim 32 U: the wrap to position 0);
    'base' lets GaussianMix's base sum take dims 0 and 1; 'last_pair' drops Himmelblau's last pair; 'corr' ignores corr; 'triple'
    reads the shells' parameters from the wrong place (shell: the second triple; double_shell: the centres exchanged -- the
    whole triples exchanged is the same function); 'nan' leaves a non-finite row as it is."""
    assert layout in ('solo', 'tile') and fault in (None,) + FAULTS
    tx = np.atleast_2d(np.asarray(tx32, _F))
    N, D = tx.shape
    U = units(D)
    p = np.zeros(6)
    p[:len(params or ())] = params or ()
    pad = np.zeros((N, 32 * U), _F)
    pad[:, :D] = tx
    if layout == 'solo':
        th = pad.reshape(N, 16, 2 * U)                      # [row, position, k]
        dim = (2 * U * np.arange(16)[:, None] + np.arange(2 * U)[None, :])[None]
        nxt = np.roll(th[:, :, 0], -1, axis=1)              # solo_ror<15>: position m reads position m + 1 (15 wraps to 0)
        lanes, per_lane = 16, 2 * U
        part = lambda k: (th[:, :, k], dim[:, :, k], th[:, :, k + 1] if k + 1 < 2 * U else nxt, k + 1 == 2 * U)
        sum32 = _row_sum32
        sum64 = _xor_sum64
        first = th[:, 0, 0], th[:, 0, 1]
    else:
        th4 = pad.reshape(N, U, 4, 8)                       # [row, tile, lane group, j]
        lanes, per_lane = 4, 8 * U
        dim4 = (32 * np.arange(U)[:, None, None] + 8 * np.arange(4)[None, :, None] + np.arange(8)[None, None, :])[None]

        def part(k):
            tau, j = divmod(k, 8)
            if j < 7:
                nb = th4[:, tau, :, j + 1]
            else:   # the next 8-block: lane group g + 1 of this tile, or group 0 of the next tile (0 behind the last)
                nb = np.concatenate([th4[:, tau, 1:, 0], th4[:, tau + 1, :1, 0] if tau + 1 < U else np.zeros((N, 1), _F)], axis=1)
            return th4[:, tau, :, j], dim4[:, tau, :, j], nb, j == 7
        sum32 = _wide_sum
        sum64 = lambda v: (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
        first = th4[:, 0, 0, 0], th4[:, 0, 0, 1]
    with np.errstate(all='ignore'):
        if name == 'rosenbrock':
            facc = np.zeros((N, lanes), _F)
            for k in range(per_lane):
                a0, i, a1, crosses = part(k)
                term = _rosen_term(a0, a1)
                keep = (i < D) if fault == 'mask' else (i + 1 < D)
                if fault == 'boundary' and crosses:
                    keep = keep & False
                facc = facc + np.where(keep, term, _F(0.0))
            acc = -np.asarray(sum32(facc), np.float64)
        elif name == 'gaussmix':
            facc = np.zeros((N, lanes), _F)
            for k in range(per_lane):
                a0, d, _, _ = part(k)
                keep = (d < D) if fault == 'base' else ((d >= 2) & (d < D))
                facc = facc + np.where(keep, a0 * a0, _F(0.0))
            acc = _mix_tail(np.asarray(sum32(facc), np.float64), first[0], first[1], D)
        elif name == 'himmelblau':
            facc = np.zeros((N, lanes), _F)
            for k in range(0, per_lane, 2):
                x0, _, x1, _ = part(k)
                d1 = part(k + 1)[1]
                keep = (d1 < D - 2) if fault == 'last_pair' else (d1 < D)
                facc = facc + np.where(keep, _himmel_term(x0, x1), _F(0.0))
            acc = np.asarray(sum32(facc), np.float64)
        elif name == 'eggbox':
            chi = np.cos(first[0] / _F(2.0)) * np.cos(first[1] / _F(2.0))
            b = _F(2.0) + chi
            b2 = b * b
            acc = (b2 * b2 * b).astype(np.float64)
        else:
            s1, s2 = np.zeros((N, lanes)), np.zeros((N, lanes))
            for k in range(per_lane):
                a0, d, _, _ = part(k)
                t = np.where(d < D, a0.astype(np.float64), 0.0)
                s1 = s1 + t
                s2 = s2 + t * t
            if fault == 'corr':
                p[0] = 0.0
            if fault == 'triple':
                p = np.concatenate([p[3:], p[:3]]) if name == 'shell' else p[[0, 1, 5, 3, 4, 2]]
            acc = _moments_tail(name, sum64(s1), sum64(s2), D, p)
    acc = np.asarray(acc, np.float64)
    return acc if fault == 'nan' else np.where(np.isfinite(acc), acc, SAFE)


# ---- the checks ----------------------------------------------------------------------------------------------------------------------
def check_logl_of_own_x(logl_kernel, x_kernel, sd, mu, name, params=None, bound=logl_bound, what=''):
    """the kernel's logL against exact_logl on T32 of the x the kernel itself stored: |error| <= bound(exact value) in every row;
    a row the safe rule maps (exact value -1e100) must hold -1e100 itself.  Returns the worst error / bound."""
    got = np.asarray(logl_kernel, np.float64).reshape(-1)
    x = np.asarray(x_kernel, np.float32)
    want = exact_logl(name, T32(x.reshape(len(got), -1), sd, mu), params)
    mapped = want == SAFE
    assert np.array_equal(got[mapped], want[mapped]), '%s: %d rows of non-finite logL are not -1e100' % (what, int(mapped.sum()))
    if mapped.all():
        return 0.0
    ratio = np.abs(got[~mapped] - want[~mapped]) / bound(want[~mapped])
    bad = ~(ratio <= 1.0)   # (a NaN fails)
    assert not bad.any(), '%s: logL of the kernel\'s own x: %d of %d rows outside the bound, worst %.3g of it (value %.6g)' % (
        what, int(bad.sum()), len(ratio), float(np.nanmax(ratio)) if np.isfinite(ratio).any() else np.nan,
        float(want[~mapped][np.argmax(np.where(np.isnan(ratio), np.inf, ratio))]))
    return float(ratio.max())


def check_lp_split(lp_kernel, logl_kernel, ld_oracle, inside, bound_ld, what=''):
    """lp - logL against the oracle's log-det: |(lp - logL) - ld| <= bound_ld (an array, one figure per row) on the rows inside the
    box; a row outside it must be exactly -inf.  A row whose logL is the safe rule's -1e100 keeps no log-det in float64: it must
    hold -1e100.  Returns the worst error / bound."""
    lp, ll, ld = (np.asarray(v, np.float64).reshape(-1) for v in (lp_kernel, logl_kernel, ld_oracle))
    inside = np.asarray(inside, bool).reshape(-1)
    b = np.broadcast_to(np.asarray(bound_ld, np.float64), lp.shape)
    assert np.all(lp[~inside] == -np.inf), '%s: %d rows outside the box are not -inf' % (what, int((lp[~inside] != -np.inf).sum()))
    mapped = inside & (ll == SAFE)
    assert np.all(lp[mapped] == SAFE), '%s: rows of logL = -1e100 inside the box do not hold it' % what
    rows = inside & ~mapped
    if not rows.any():
        return 0.0
    ratio = np.abs((lp[rows] - ll[rows]) - ld[rows]) / b[rows]
    bad = ~(ratio <= 1.0)
    assert not bad.any(), '%s: lp - logL against the oracle\'s log-det: %d of %d rows outside the bound, worst %.3g of it' % (
        what, int(bad.sum()), len(ratio), float(np.nanmax(ratio)) if np.isfinite(ratio).any() else np.nan)
    return float(ratio.max())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.view(v) == b.view(v)


class Restated(object):
    """the target in the kernels' arithmetic with any likelihood of LIKES: a flow's inverse x_of_z(q) -> (x, log|det|) (None: the
    x-space run, the identity with log-det 0), T in float32, the float64 oracle likelihood with the safe rule, the box lo / hi on
    T(x) (None: no prior).  The Gaussian with corr 0.5 is the default, as the three classes this one stands beside
    (tests/test_gpu_mcmc_walk.py, tests/test_gpu_importance.py, tests/test_gpu_ensemble.py oracle_lp)."""

    def __init__(self, x_of_z, sd, mu, lo=None, hi=None, like='gaussian', params=(0.5,)):
        self.sd, self.mu, self.lo, self.hi, self.like, self.params = sd, mu, lo, hi, like, params
        self.x_of_z = x_of_z if x_of_z is not None else (lambda q: (np.asarray(q, np.float32), np.zeros(len(q))))
        self.lp = latent_target(self.x_of_z, self.logl, self.inside)

    def T(self, x):
        return T32(x, self.sd, self.mu)

    def inside(self, x):
        return in_box(self.T(x), self.lo, self.hi)

    def logl(self, x):
        return exact_logl(self.like, self.T(x), self.params)


# ---- the ensemble kernels' own draws, restated (nnest_amd/csrc/ensemble_common.h, nnest_ensemble.hip ensemble_split_kernel): the
# CPU side picks the replay seeds with them; the GPU tests hold them to nnest_ensemble_fill_noise / nnest_ensemble_fill_moves ----
def ensemble_draws(seed, C, S, D, moves=None, step0=0):
    """[(inds [C], u [C, 3] float32, move, jb [C], gamma [C] float32)] for steps step0 .. step0 + S - 1.  Philox stream 4: the split
    (Fisher-Yates from arange(C) & 1, index i from C - 1 down to 1, word i of block (i // 4, t, 0)) and the step's move (word 0 of
    block (0, t, 1) against thr = floor(p_stretch 2^24)); stream 3: the walker's uniforms (block (0, k, t)) and its DE scale
    (block (1, k, t))."""
    walkers = np.arange(C, dtype=np.uint64)
    ws, wd = (1.0, 0.0) if moves is None else (float(moves.get('stretch', 0.0)), float(moves.get('de', 0.0)))
    thr = int(np.floor(ws / (ws + wd) * (1 << 24)))
    g0 = np.float32(de_gamma0(D))
    sigma = np.float32(1e-5)
    n0 = (C + 1) // 2
    out = []
    for i in range(S):
        t = int(step0) + i
        nb = (C + 3) // 4
        words = philox4x32_10(np.stack([np.arange(nb, dtype=np.uint64), np.full(nb, t, np.uint64), np.zeros(nb, np.uint64),
                                        np.full(nb, 4 << 28, np.uint64)], -1), seed).reshape(-1)
        inds = (np.arange(C) & 1).astype(np.int32)
        for ii in range(C - 1, 0, -1):
            j = ((int(words[ii]) >> 8) * (ii + 1)) >> 24
            inds[ii], inds[j] = inds[j], inds[ii]
        mv = philox4x32_10(np.array([[0, t, 1, 4 << 28]], np.uint64), seed)[0]
        move = STRETCH if (int(mv[0]) >> 8) < thr else DE
        r = philox4x32_10(_counters(0, walkers, t, 3), seed)                       # [C, 4]
        m = (r >> np.uint64(8)).astype(np.int64)
        u = (m[:, :3].astype(np.float64) * 2.0 ** -24).astype(np.float32)
        nc = np.where(inds == 0, C - n0, n0)
        ja = (m[:, 1] * nc) >> 24
        jb = (m[:, 3] * (nc - 1)) >> 24
        jb = jb + (jb >= ja)
        r1 = philox4x32_10(_counters(1, walkers, t, 3), seed)
        m1 = (r1 >> np.uint64(8)).astype(np.float64)
        n = np.sqrt(-2.0 * np.log((m1[:, 0] + 1.0) * 2.0 ** -24)) * np.cos(6.283185307179586476925 * (m1[:, 1] * 2.0 ** -24))
        gamma = (np.float64(g0) * (1.0 + np.float64(sigma) * n)).astype(np.float32)
        out.append((inds, u, move, jb.astype(np.int32), gamma))
    return out


def move_ids(seed, S, moves, step0=0):
    """the move of every step alone (ensemble_draws' rule)"""
    ws, wd = float(moves.get('stretch', 0.0)), float(moves.get('de', 0.0))
    thr = int(np.floor(ws / (ws + wd) * (1 << 24)))
    r = philox4x32_10(np.array([[0, int(step0) + i, 1, 4 << 28] for i in range(S)], np.uint64), seed)
    return np.where((r[:, 0] >> np.uint64(8)).astype(np.int64) < thr, STRETCH, DE)


def seed_with_both_moves(first, S, moves):
    """the first seed from `first` on whose S steps hold a stretch step and a DE step"""
    seed = int(first)
    while len(set(move_ids(seed, S, moves).tolist())) < 2:
        seed += 1
    return seed


def replay_margins(x0, draws, lp_fn, bound=logl_bound):
    """the restatement alone from x0 on `draws`: every decision's distance to its threshold as a share of the replay's margin
    m = 10 bound(max |lp|) (tests/test_gpu_mcmc_walk.py's rule), and the number of accepted moves.  A seed whose smallest share is
    well above 1 has no decision that the kernel's rounding could turn."""
    x = np.asarray(x0, np.float32)
    lp = np.asarray(lp_fn(x), np.float64)
    shares, moved = [], 0
    for inds, u, move, jb, gamma in draws:
        rec = []
        x, lp_new = moves_step(x, lp, inds, u, move, jb, gamma, lp_fn, record=rec)
        for r in rec:
            shares.append(decision_shares(r, lp[r['walkers']], bound))
            moved += int(r['accept'].sum())
        lp = lp_new
    return np.concatenate(shares), moved


def decision_shares(r, lp_old, bound=logl_bound):
    """|lnpdiff - log u3| / (10 bound(max(|lp_q|, |lp_old|))) of a half-step record; inf where no rounding can turn the decision
    (a proposal outside the box, a walker at -inf)"""
    lq, lo_ = np.asarray(r['lp_q'], np.float64), np.asarray(lp_old, np.float64)
    fin = np.isfinite(lq) & np.isfinite(lo_)
    m = 10.0 * bound(np.maximum(np.abs(np.where(fin, lq, 0.0)), np.abs(np.where(fin, lo_, 0.0))))
    with np.errstate(invalid='ignore'):
        d = np.abs(r['lnpdiff'] - r['logu3'])
    return np.where(fin, d / m, np.inf)


# ---- the x-space decision replay of tests/test_gpu_fused_likes.py: Rosenbrock in the valley at x_dim 3, 33, 65, 128 ----------------
MIX = {'stretch': 0.5, 'de': 0.5}
REPLAY_C, REPLAY_S = 66, 6
# (seed by (x_dim, mixture): the first of 6000 + x_dim, 6001 + x_dim, ... for which the restatement alone, on the restated draws,
# has no decision within three times the margin, moves at least five walkers and, with the mixture, takes a step of each kind:
# pick_replay_seed; tests/test_fused_like_check.py holds every entry to that)
REPLAY_SEEDS = {(D, mix): 6000 + D for D in (3, 33, 65, 128) for mix in (False, True)}   # (the first try passes at each)


def replay_case(D):
    """the start x0 [REPLAY_C, D] (x ~ 0.5 N(0, 1), row 1 put outside the box), T and the box of the replay at x_dim D"""
    sd, mu = affine('rosenbrock', 'valley', D, D)
    lo, hi = box_for(sd, mu)
    x0 = (np.random.RandomState(D).normal(size=(REPLAY_C, D)) * 0.5).astype(np.float32)
    x0[1, D - 1] = (hi[D - 1] + 1.0 - mu[D - 1]) / sd[D - 1]
    return x0, sd, mu, lo, hi


def pick_replay_seed(D, mix, tries=200):
    x0, sd, mu, lo, hi = replay_case(D)
    rs = Restated(None, sd, mu, lo, hi, 'rosenbrock', ())
    for seed in range(6000 + D, 6000 + D + tries):
        draws = ensemble_draws(seed, REPLAY_C, REPLAY_S, D, MIX if mix else None)
        if mix and {d[2] for d in draws} != {STRETCH, DE}:
            continue
        shares, moved = replay_margins(x0, draws, rs.lp)
        if shares.min() > 3.0 and moved >= 5:
            return seed
    raise RuntimeError('no seed')
