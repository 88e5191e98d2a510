"""The CPU side of tests/test_gpu_walk_likes.py and tests/test_gpu_tile_data_likes.py.  numpy and the oracle only: no GPU.

1. A float32 restatement of the two likelihoods of user data in the spline flow's TEAM TILE (nnest_amd/csrc/mcmc_gdata.h
   gdata_tile_loglike, nnest_amd/csrc/glm_data.h glm_tile_loglike) in the tile's block order: row blocks of 16, column blocks from
   rb // 2, K-steps (tau, j) of four columns 32 tau + 8 k + j, the GLM's row blocks dealt to four waves whose partials are added in
   wave order.  A K-step is restated as four fused multiply-adds in the order of k; the matrix cores' own order inside a K-step is not
   documented, so the restatement is held to the a-priori bounds of tests/gdata_check.py and tests/glm_check.py like the kernels, not
   to their bits.  tests/test_tile_like_check.py shows that it meets them with half to spare at every table entry, and that each of
   the planted FAULTS misses them.
     Two faults concern a column c >= D, where the tile holds t = 0 and d = 0: a finite operand there changes nothing.  They are
   stated as what such a read does.  gdata 'pad_col': the lane that holds column D - 1 masks its 8 columns as one, so its columns
   c >= D are read from the flat [D, D] array -- the next row, and behind the last row past the array's end, which is poison (NaN).
   glm 'last_col': the same lane repeats its last live column, operand and all, in the column behind it.
2. The cases of the two GPU files that are not tests/test_gpu_fused_likes.py's own, the walk's parameters, and the seeds, which were
   chosen with the restatement of the walk (tests/mcmc_adapt_check.py) through the oracle's flows: tools/walk_like_cases.py."""
import numpy as np

from tests import fused_like_check as fl
from tests import gdata_check as gc
from tests import glm_check as gk
from tests import mcmc_adapt_check as ac

_F = np.float32
SPL_TOL = 3e-5

# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# GaussianData: both sides of every 16-row block and every 32-column block at hidden 16; hidden 32 at NT = 1 and 2
GDATA_CASES = [(D, 16) for D in (1, 2, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128)] + [(8, 32), (33, 32), (64, 32)]
GLM_DIMS = [(2, 16), (33, 16), (65, 16), (97, 16), (128, 16), (8, 32), (40, 32)]
GLM_NS = (1, 17, 49, 65, 200)   # 1, 2, 4, 5 and 13 row blocks
GLM_CASES = [(D, H, fam, n) for D, H in GLM_DIMS for fam in gk.FAMILIES for n in GLM_NS]
HALF = 2.5      # the box on T(x) of the data cases
C_DATA = 40     # walkers of the data cases and of every spline case: a last tile of 8


def key(D, H):
    """10 NT + NH of spl_tile_for_shape"""
    return 10 * fl.units(D) + H // 16


def affine(D, seed):
    """tests/test_gpu_mcmc_mixed.affine"""
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)


def data_start_x(D, C=C_DATA):
    """x ~ 0.5 N(0, 1); row 1 has T(x) = 5 in its last coordinate (outside the box); row 2, well inside, holds a NaN"""
    sd, mu = affine(D, D)
    x0 = (np.random.RandomState(D).normal(size=(C, D)) * 0.5).astype(np.float32)
    x0[1, D - 1] = (2.0 * HALF - mu[D - 1]) / sd[D - 1]
    x0[2] = x0[2] * _F(0.25)
    x0[2, 0] = np.nan
    return x0


# ---- the tile evaluators, restated ---------------------------------------------------------------------------------------------------
GDATA_FAULTS = ('col_start', 'strict', 'break', 'pad_col', 'mu_shift')
GLM_FAULTS = ('rows', 'wave3', 'acc2', 'last_col', 'offset')


def _fma32(acc, a, b):
    """fmaf: the product of two float32 is exact in float64; one rounding to float32 (the double rounding through float64 is beyond
    what the bounds resolve)"""
    return (acc.astype(np.float64) + np.asarray(a, _F).astype(np.float64) * np.asarray(b, _F).astype(np.float64)).astype(_F)


def _group_sum(v4):
    """group_sum of four float64 partials [N, 4]: (v0 + v1) + (v2 + v3)"""
    return (v4[:, 0] + v4[:, 1]) + (v4[:, 2] + v4[:, 3])


def gdata_tile32(data, t, fault=None):
    """logL [N] float64 of the rows t [N, D] float32 as gdata_tile_loglike<NT> forms it"""
    assert fault in (None,) + GDATA_FAULTS
    mu, R = np.asarray(data['mu'], _F).reshape(-1), np.asarray(data['R'], _F)
    t = np.atleast_2d(np.asarray(t, _F))
    N, D = t.shape
    NT = fl.units(D)
    W = 32 * NT
    tp, mp = np.zeros((N, W), _F), np.zeros(W, _F)
    tp[:, :D], mp[:D] = t, mu
    if fault == 'mu_shift':   # lane group g reads lane group g + 1's eight
        mp = mp.reshape(NT, 4, 8)[:, [1, 2, 3, 0], :].reshape(W)
    with np.errstate(invalid='ignore', over='ignore'):
        d = tp - mp
        r, c = np.arange(W)[:, None], np.arange(W)[None, :]
        c_end = 8 * ((D + 7) // 8) if fault == 'pad_col' else D
        flat = np.concatenate([R.reshape(-1), np.full(W * W, np.nan, _F)])   # (past the end of [D, D]: poison)
        keep = (r < D) & ((c > r) if fault == 'strict' else (c >= r)) & (c < c_end)
        A = np.where(keep, flat[np.minimum(r * D + c, len(flat) - 1)], _F(0.0)).astype(_F)
        q4 = np.zeros((N, 4))
        for rb in range(2 * NT):
            if (16 * (rb + 1) > D) if fault == 'break' else (16 * rb >= D):
                break
            rows = 16 * rb + np.arange(16)
            acc = np.zeros((N, 16), _F)
            for tau in range(rb // 2 + (1 if fault == 'col_start' else 0), NT):
                for j in range(8):
                    for k in range(4):
                        col = 32 * tau + 8 * k + j
                        acc = _fma32(acc, A[rows, col][None, :], d[:, col][:, None])
            y = acc.astype(np.float64)
            for g in range(4):
                for v in range(4):
                    q4[:, g] = q4[:, g] + y[:, 4 * g + v] * y[:, 4 * g + v]
        return gc.finish(data['logl0'], _group_sum(q4))


def glm_tile32(data, t, fault=None):
    """logL [N] float64 of the rows t [N, D] float32 as glm_tile_loglike<NT, FAM> forms it; reads the PADDED arrays, as the kernel does"""
    assert fault in (None,) + GLM_FAULTS
    n = int(data['n'])
    at, y, o = np.asarray(data['at'], _F), np.asarray(data['y'], _F).reshape(-1), np.asarray(data['o'], _F).reshape(-1)
    t = np.atleast_2d(np.asarray(t, _F))
    N, D = t.shape
    NT = fl.units(D)
    W = 32 * NT
    tp = np.zeros((N, W), _F)
    tp[:, :D] = t
    nrb = (n + 15) >> 4
    RB = 2 if NT == 1 else 1
    part = np.zeros((4, N))
    with np.errstate(invalid='ignore', over='ignore'):
        for wv in range(4):
            s4 = np.zeros((N, 4))
            for rb in range(wv, nrb, 4 * RB):
                for q in range(RB):
                    b = rb + 4 * q
                    if b >= nrb or (fault == 'acc2' and q == 1):
                        continue
                    rows = 16 * b + np.arange(16)
                    acc = np.broadcast_to(_F(0.0) if fault == 'offset' else o[rows], (N, 16)).astype(_F)
                    for tau in range(NT):
                        for j in range(8):
                            for k in range(4):
                                col = 32 * tau + 8 * k + j
                                a = at[min(col, D - 1), rows] if col < D else np.zeros(16, _F)
                                tc = tp[:, col]
                                if fault == 'last_col' and col == D and D % 8:
                                    a, tc = at[D - 1, rows], tp[:, D - 1]
                                acc = _fma32(acc, a[None, :], tc[:, None])
                    l = gk.terms(data['family'], acc.astype(np.float64), y[rows].astype(np.float64)[None, :])
                    live = np.ones(16, bool) if fault == 'rows' else rows < n
                    l = np.where(live[None, :], l, 0.0)
                    for g in range(4):
                        for v in range(4):
                            s4[:, g] = s4[:, g] + l[:, 4 * g + v]
            part[wv] = _group_sum(s4)
        tot = (part[0] + part[1]) + part[2]
        if fault != 'wave3':
            tot = tot + part[3]
        return gk.finish(data['logl0'], tot)


def logl_ratio(got, t, exact, bound):
    """worst |got - float64| / B over the rows of t; inf where a row the safe rule maps does not hold -1e100, or a ratio is NaN"""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(exact(t), np.float64)
    mapped = want == fl.SAFE
    if not np.array_equal(got[mapped], want[mapped]):
        return np.inf
    if mapped.all():
        return 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        ratio = np.abs(got[~mapped] - want[~mapped]) / np.asarray(bound(t), np.float64)[~mapped]
    return float(ratio.max()) if np.all(ratio == ratio) else np.inf


def gdata_ratio(got, data, t):
    return logl_ratio(got, t, lambda v: gc.exact(data, v)[0], lambda v: gc.bound(data, v))


def glm_ratio(got, data, t):
    return logl_ratio(got, t, lambda v: gk.exact(data, v)[0], lambda v: gk.bound(data, v))


# ---- the walk of both GPU files ------------------------------------------------------------------------------------------------------
S, K, A, RATE, TARGET = 6, 3, 4, 1.0, 0.234
BETA, BETA_DATA = 0.3, 0.5
# (beta, global_every, adapt_steps, a step of the walker's own)
CONFIGS = {'tempered': (BETA, 0, 0, False), 'mixed': (BETA, K, 0, False), 'adaptive': (BETA, K, A, True)}
DATA_CONFIG = (BETA_DATA, K, A, True)


def step_spread(C, D):
    """step_in [C] float64: a factor 16 around 1 / sqrt(D), from a quarter of it to four times it"""
    return 4.0 ** np.linspace(-1.0, 1.0, C) / np.sqrt(D)


class Target(object):
    """the tempered latent target in the kernels' arithmetic: the oracle's inverse (float32), T in float32 (two roundings), the box on
    T(x), logL in float64 from the float32 row: lp = ((beta logL) + log|det|) + prior"""

    def __init__(self, o, sd, mu, lo, hi, logl_of_t, bound_of_t, beta, flow_tol):
        self.o, self.sd, self.mu, self.lo, self.hi, self.beta = o, sd, mu, lo, hi, beta
        self.logl_of_t, self.bound_of_t, self.flow_tol = logl_of_t, bound_of_t, flow_tol

    def tx(self, q):
        x, ld = self.o.inverse(np.asarray(q, _F))
        return fl.T32(x, self.sd, self.mu), np.asarray(ld, np.float64)

    def lp(self, q):
        t, ld = self.tx(q)
        prior = np.where(fl.in_box(t, self.lo, self.hi), 0.0, -np.inf)
        return ((self.beta * np.asarray(self.logl_of_t(t), np.float64)) + ld) + prior

    def tol(self, q, lp_q):
        """the tolerance in force on lp at the rows q: the flow's at |lp| plus the likelihood's bound"""
        t, _ = self.tx(q)
        v = np.abs(np.where(np.isfinite(lp_q), lp_q, 0.0))
        with np.errstate(invalid='ignore', over='ignore'):
            b = np.asarray(self.bound_of_t(t), np.float64)
        return self.flow_tol(v) + np.where(np.isfinite(b), b, 0.0)


def walk_stats(target, z0, seed, config):
    """the restatement alone from z0 (rows with a NaN left out; the draws keep the walkers' indices) on the restated draws.  Over the
    walkers that start inside the box: how many global proposals are accepted / refused with every decision of the walker up to and
    including that one further than ten times the tolerance in force from its threshold (so that no rounding of the kernel's turns
    it), and how many local steps moved, of how many"""
    beta, k, adapt, spread = config
    z0 = np.asarray(z0, _F)
    C, D = z0.shape
    rows = ~np.isnan(z0).any(1)
    eps, u = ac.mcmc_draws(seed, 0, C, 0, S, D)
    sigma0 = ac.clamp(step_spread(C, D))[rows] if spread else float(_F(1.0 / np.sqrt(D)))
    z, lp0 = z0[rows], target.lp(z0[rows])
    recs = []
    out = ac.adapt_run(z, lp0, [(eps[i][rows], u[i][rows]) for i in range(S)], sigma0, target.lp, k, adapt, RATE, TARGET, records=recs)
    hz, hl = out[2], out[3]
    inside = np.isfinite(lp0)
    firm = inside.copy()
    acc_g = ref_g = moved = local = 0
    for i, rec in enumerate(recs):
        z_prev, lp_prev = (z, lp0) if i == 0 else (hz[:, i - 1], hl[:, i - 1])
        m = 10.0 * np.maximum(target.tol(rec['q'], rec['lp_q']), target.tol(z_prev, lp_prev))
        with np.errstate(invalid='ignore'):
            firm &= ~(np.abs(rec['margin']) <= m)   # (a NaN margin -- from -inf to -inf -- is refused on both sides)
        if ac.kind(i, k):
            acc_g += int((firm & rec['accept']).sum())
            ref_g += int((firm & ~rec['accept'] & np.isfinite(rec['margin'])).sum())
        else:
            moved += int(rec['accept'][inside].sum())
            local += int(inside.sum())
    return acc_g, ref_g, moved, local


def seed_is_fair(target_of_beta, z0, seed, configs):
    """the seed condition of both GPU files on the restatement alone: under every configuration some but not all local steps move,
    and under each with global steps one is accepted and one is refused (finite on both sides) beyond ten times the tolerance"""
    for config in configs:
        acc_g, ref_g, moved, local = walk_stats(target_of_beta(config[0]), z0, seed, config)
        if not 0 < moved < local:
            return False
        if config[1] > 0 and (acc_g < 1 or ref_g < 1):
            return False
    return True


# ---- the cases' flows and targets on the CPU: the initialisations the GPU tests use (default_init needs no device) ----------------------
def nvp_oracle(D):
    """the oracle's RealNVP on HipNVP(D, 16, 3, 1, seed=D)'s weights (tests/test_gpu_fused_likes.nvp_flow)"""
    from nnest_amd.flow import HipNVP
    from oracle import oracle as orc
    h = object.__new__(HipNVP)
    h.D, h.H, h.B, h.L, h.scale = D, 16, 3, 1, ''
    h.num_params = 2 * 3 * (16 * D + 16 + (16 * 16 + 16) + D * 16 + D)
    return orc.NVP(D, 16, 3, 1, h.default_init(D))


def spline_oracle(D, H, C=C_DATA):
    """the oracle's spline on HipSpline(D, H, 3, seed=D + H)'s weights with the ActNorm layers set as tests/test_gpu_fused_likes.spline_flow
    sets them (the oracle's data-dependent initialisation stands in for the device's: equal to rounding)"""
    from nnest_amd.spline import HipSpline
    from oracle import oracle as orc
    s = object.__new__(HipSpline)
    s.D, s.H, s.B, s.K = D, H, 3, 8
    s.nu = D // 2
    s.nl = D - s.nu
    w, P = s.default_init(D + H)
    o = orc.Spline(D, H, 3, 8, 3.0, w, P)
    o.forward((np.random.RandomState(D + H).normal(size=(C, D)) * 0.5).astype(_F), data_init=True)
    return o


def spline_tol_cpu(o, D, H, z):
    """tests/test_gpu_fused_likes.spline_tols' figure from the oracle alone"""
    tol = SPL_TOL
    if key(D, H) not in (11, 21):
        z = z[~np.isnan(z).any(1)]
        (x32, ld32), (x64, ld64) = o.inverse(z), o.inverse(z, f64=True)
        rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b) / (1.0 + np.abs(b))))
        tol = max(SPL_TOL, 5.0 * max(rel(x32, x64), rel(ld32, ld64)))
    return lambda v: tol * (1.0 + np.abs(v))


def nvp_tol_cpu(D):
    """tests/test_gpu_fused_likes.nvp_tols; x_dim > 50 has no recorded figure -- the GPU test measures it --: 1e-4 stands in for it, as
    in tools/mcmc_mixed_cases.py"""
    return (lambda v: 2e-5 + 1e-6 * np.abs(v)) if D <= 50 else (lambda v: 1e-4 + 0.0 * v)


def _forward_rows(o, x0):
    z0 = np.full(x0.shape, np.nan, _F)
    rows = ~np.isnan(x0).any(1)
    z0[rows] = o.forward(x0[rows])[0]
    return z0


def walk_start_x(start_x, D, C, sd, mu, lo, hi, x_sd):
    """tests/test_gpu_fused_likes.start_x (x ~ 0.5 N(0, 1), row 1 outside the box, row 2 with a NaN) at the scale x_sd the transform and
    the box are made for, so that the start is spread as the global proposals are: x ~ x_sd N(0, 1).  From a start at half that
    scale in a box made for N(0, 1) no global proposal is accepted at x_dim 128 (Rosenbrock: lp -2000 against -500)"""
    return start_x(D, C, sd, mu, lo, hi, nan=True) * _F(x_sd / 0.5)


def analytic_case(flow, name, recipe, D, H=16):
    """(target_of_beta, z0) of a row of NVP_TABLE / SPLINE_TABLE as tests/test_gpu_walk_likes.py runs it"""
    from tests.test_gpu_fused_likes import C_ENS, setup, start_x
    x_sd, C = (1.0, C_ENS) if flow == 'nvp' else (0.5, C_DATA)
    _, params, sd, mu, lo, hi = setup(name, recipe, D, x_sd=x_sd)
    o = nvp_oracle(D) if flow == 'nvp' else spline_oracle(D, H)
    z0 = _forward_rows(o, walk_start_x(start_x, D, C, sd, mu, lo, hi, x_sd))
    ftol = nvp_tol_cpu(D) if flow == 'nvp' else spline_tol_cpu(o, D, H, z0)
    logl = lambda t: fl.exact_logl(name, t, params)
    return (lambda beta: Target(o, sd, mu, lo, hi, logl, lambda t: fl.logl_bound(logl(t)), beta, ftol)), z0


def data_like(kind, D, fam=None, n=None):
    """the descriptor of a data case: tests/gdata_check.replay_target, tests/glm_check.replay_target"""
    return gc.replay_target(D) if kind == 'gdata' else gk.replay_target(D, n, fam)


def data_case(kind, D, H, fam=None, n=None):
    """(target_of_beta, z0, data) of a case of tests/test_gpu_tile_data_likes.py"""
    data = data_like(kind, D, fam, n)
    sd, mu = affine(D, D)
    box = np.full(D, HALF, _F)
    o = spline_oracle(D, H)
    z0 = _forward_rows(o, data_start_x(D))
    ftol = spline_tol_cpu(o, D, H, z0)
    mod = gc if kind == 'gdata' else gk
    logl, bound = (lambda t: mod.exact(data, t)[0]), (lambda t: mod.bound(data, t))
    return (lambda beta: Target(o, sd, mu, -box, box, logl, bound, beta, ftol)), z0, data


def pick_seed(target_of_beta, z0, configs, first, tries=80):
    """the first seed from `first` on that is fair"""
    for seed in range(first, first + tries):
        if seed_is_fair(target_of_beta, z0, seed, configs):
            return seed
    raise RuntimeError('no fair seed in %d .. %d' % (first, first + tries - 1))


# the seeds: the first fair one from 9000 + x_dim on (tools/walk_like_cases.py prints these tables)
WALK_SEEDS = {
    ('nvp', 'rosenbrock', 'valley', 5): 9005, ('nvp', 'rosenbrock', 'wide', 33): 9033, ('nvp', 'rosenbrock', 'valley', 70): 9070,
    ('nvp', 'rosenbrock', 'wide', 128): 9128, ('nvp', 'gaussmix', 'main', 20): 9020, ('nvp', 'himmelblau', 'main', 66): 9066,
    ('nvp', 'gaussian', 'main', 100): 9102, ('nvp', 'shell', 'main', 40): 9040, ('nvp', 'double_shell', 'main', 97): 9097, ('nvp',
    'eggbox', 'main', 2): 9002, ('spline', 'rosenbrock', 'valley', 5, 16): 9005, ('spline', 'rosenbrock', 'valley', 40, 16): 9040,
    ('spline', 'rosenbrock', 'valley', 70, 16): 9070, ('spline', 'rosenbrock', 'valley', 128, 16): 9128, ('spline', 'rosenbrock',
    'valley', 8, 32): 9008, ('spline', 'rosenbrock', 'valley', 40, 32): 9040, ('spline', 'rosenbrock', 'wide', 128, 16): 9128,
    ('spline', 'eggbox', 'main', 2, 16): 9002, ('spline', 'gaussmix', 'main', 5, 16): 9005, ('spline', 'shell', 'main', 40, 16):
    9040, ('spline', 'himmelblau', 'main', 70, 16): 9070, ('spline', 'gaussian', 'main', 128, 16): 9129, ('spline', 'double_shell',
    'main', 8, 32): 9008, ('spline', 'gaussian', 'main', 40, 32): 9040,
}
DATA_SEEDS = {
    ('gdata', 2, 16): 9002, ('gdata', 16, 16): 9016, ('gdata', 17, 16): 9017, ('gdata', 31, 16): 9031, ('gdata', 32, 16): 9032,
    ('gdata', 33, 16): 9033, ('gdata', 48, 16): 9048, ('gdata', 49, 16): 9049, ('gdata', 64, 16): 9064, ('gdata', 65, 16): 9065,
    ('gdata', 80, 16): 9080, ('gdata', 81, 16): 9081, ('gdata', 96, 16): 9096, ('gdata', 97, 16): 9097, ('gdata', 112, 16): 9112,
    ('gdata', 113, 16): 9113, ('gdata', 128, 16): 9129, ('gdata', 8, 32): 9008, ('gdata', 33, 32): 9033, ('gdata', 64, 32): 9064,
    ('glm', 2, 16, 'logistic', 1): 9002, ('glm', 2, 16, 'logistic', 17): 9002, ('glm', 2, 16, 'logistic', 49): 9002, ('glm', 2, 16,
    'logistic', 65): 9002, ('glm', 2, 16, 'logistic', 200): 9002, ('glm', 2, 16, 'poisson', 1): 9002, ('glm', 2, 16, 'poisson', 17):
    9002, ('glm', 2, 16, 'poisson', 49): 9002, ('glm', 2, 16, 'poisson', 65): 9002, ('glm', 2, 16, 'poisson', 200): 9002, ('glm',
    33, 16, 'logistic', 1): 9033, ('glm', 33, 16, 'logistic', 17): 9033, ('glm', 33, 16, 'logistic', 49): 9033, ('glm', 33, 16,
    'logistic', 65): 9033, ('glm', 33, 16, 'logistic', 200): 9033, ('glm', 33, 16, 'poisson', 1): 9033, ('glm', 33, 16, 'poisson',
    17): 9033, ('glm', 33, 16, 'poisson', 49): 9033, ('glm', 33, 16, 'poisson', 65): 9033, ('glm', 33, 16, 'poisson', 200): 9033,
    ('glm', 65, 16, 'logistic', 1): 9065, ('glm', 65, 16, 'logistic', 17): 9065, ('glm', 65, 16, 'logistic', 49): 9065, ('glm', 65,
    16, 'logistic', 65): 9065, ('glm', 65, 16, 'logistic', 200): 9065, ('glm', 65, 16, 'poisson', 1): 9065, ('glm', 65, 16,
    'poisson', 17): 9065, ('glm', 65, 16, 'poisson', 49): 9065, ('glm', 65, 16, 'poisson', 65): 9065, ('glm', 65, 16, 'poisson',
    200): 9065, ('glm', 97, 16, 'logistic', 1): 9097, ('glm', 97, 16, 'logistic', 17): 9097, ('glm', 97, 16, 'logistic', 49): 9097,
    ('glm', 97, 16, 'logistic', 65): 9097, ('glm', 97, 16, 'logistic', 200): 9097, ('glm', 97, 16, 'poisson', 1): 9097, ('glm', 97,
    16, 'poisson', 17): 9097, ('glm', 97, 16, 'poisson', 49): 9097, ('glm', 97, 16, 'poisson', 65): 9097, ('glm', 97, 16, 'poisson',
    200): 9097, ('glm', 128, 16, 'logistic', 1): 9128, ('glm', 128, 16, 'logistic', 17): 9128, ('glm', 128, 16, 'logistic', 49):
    9128, ('glm', 128, 16, 'logistic', 65): 9128, ('glm', 128, 16, 'logistic', 200): 9128, ('glm', 128, 16, 'poisson', 1): 9128,
    ('glm', 128, 16, 'poisson', 17): 9128, ('glm', 128, 16, 'poisson', 49): 9128, ('glm', 128, 16, 'poisson', 65): 9128, ('glm',
    128, 16, 'poisson', 200): 9128, ('glm', 8, 32, 'logistic', 1): 9008, ('glm', 8, 32, 'logistic', 17): 9008, ('glm', 8, 32,
    'logistic', 49): 9008, ('glm', 8, 32, 'logistic', 65): 9008, ('glm', 8, 32, 'logistic', 200): 9008, ('glm', 8, 32, 'poisson',
    1): 9008, ('glm', 8, 32, 'poisson', 17): 9008, ('glm', 8, 32, 'poisson', 49): 9008, ('glm', 8, 32, 'poisson', 65): 9008, ('glm',
    8, 32, 'poisson', 200): 9008, ('glm', 40, 32, 'logistic', 1): 9040, ('glm', 40, 32, 'logistic', 17): 9040, ('glm', 40, 32,
    'logistic', 49): 9040, ('glm', 40, 32, 'logistic', 65): 9040, ('glm', 40, 32, 'logistic', 200): 9040, ('glm', 40, 32, 'poisson',
    1): 9040, ('glm', 40, 32, 'poisson', 17): 9040, ('glm', 40, 32, 'poisson', 49): 9040, ('glm', 40, 32, 'poisson', 65): 9040,
    ('glm', 40, 32, 'poisson', 200): 9040,
}
