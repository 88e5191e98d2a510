"""GPU checks of the likelihoods inside the fused ensemble, random-walk and importance kernels (include/nnest_hip.h nnest_ensemble_steps,
nnest_ensemble_moves_steps, nnest_ensemble_x_steps, nnest_ensemble_x_moves_steps, nnest_mcmc_steps, nnest_importance_evidence,
nnest_spline_ensemble_steps, nnest_spline_mcmc_steps, nnest_spline_importance_evidence) with EVERY likelihood they embed, at every
register shape: through the Python entry points only, each kernel against itself plus an exact function of its own output
(tests/fused_like_check.py): logL of a row against the float64 oracle on T(x) of the x stored beside it, lp - logL against the
oracle's log-det of the z stored beside it, a moved walker's stored lp against the kernel's own acceptance inequality on the exported
draws, an unmoved row bit for bit.  The x-space kernel also replays decision for decision (Rosenbrock in the valley).

Instantiations.  The NVP and x-space kernels are <U, LK, ...>: U = ceil(ceil(x_dim / 2) / 16) (x_dim <= 32, 64, 96, 128: U = 1 .. 4),
LK = 0 for Rosenbrock and -1 (the id read at run time) for every other likelihood, MIX for a run with a DE step.  The spline kernels
are <NT, NH>, key 10 NT + NH: NT = U of x_dim, NH = hidden / 16.  The library has no query for either, so the tables derive them
(fused_like_check.units) and each test prints the instantiation it ran beside its figures: RATIO lines, worst error / bound.

Tolerances (none is this file's): logL of the kernel's own x, hist_lp of the x-space kernel included: 2e-5 + 1e-6 |v|
(fused_like_check.logl_bound).  lp - logL and x against the oracle: NVP at x_dim <= 50: 2e-5 + 1e-6 |v| and 5e-5; NVP at wider
x_dim: twice the error of nnest_ensemble_steps with the Gaussian likelihood at that width against the same oracle, measured here
(tests/test_gpu_mcmc_walk.py's procedure); spline keys 11, 21: 3e-5 (1 + |v|); spline keys 31, 41, 12, 22: max(3e-5, 5 x the float32
oracle's own error against the float64 oracle on the same rows) (1 + |v|), tests/test_gpu_shapes.py's rule.  Where a kernel
does not export logL (the latent ensembles) it is taken as the exact logL of the kernel's own x and lp - logL is held to the sum of
the two bounds."""
import numpy as np
import pytest
import torch

from tests import fused_like_check as fl
from tests import importance_check as ic
from tests.ensemble_moves_check import DE, moves_step

pytestmark = pytest.mark.gpu

C_ENS, C_SPL, S_ENS, S_MCMC, M_IMP = 66, 40, 6, 4, 2003   # (66: a last workgroup of 2 walkers; 40: a last tile of 8; 2003: a ragged tail)
MIX = fl.MIX
GAUSS, CORR = 3, 0.5
SPL_TOL = 3e-5


def cpu(t):
    return t.cpu().numpy()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def case_id(c):
    return '-'.join(str(v) for v in c)


def note(kernel, inst, name, recipe, D, **ratios):
    print('RATIO %-34s %-22s %-12s %-6s x_dim %3d  %s' % (kernel, inst, name, recipe, D, '  '.join('%s %.3g' % kv for kv in ratios.items())))


def setup(name, recipe, D, x_sd=0.5):
    e = fl.LIKES[name]
    sd, mu = fl.affine(name, recipe, D, D, x_sd)
    lo, hi = fl.box_for(sd, mu, x_sd=x_sd)
    return e['id'], e['params'], sd, mu, lo, hi


def start_x(D, C, sd, mu, lo, hi, nan=False):
    """x ~ 0.5 N(0, 1); row 1 outside the box; with `nan` row 2, well inside the box in every other coordinate, holds a NaN"""
    x0 = (np.random.RandomState(D).normal(size=(C, D)) * 0.5).astype(np.float32)
    x0[1, D - 1] = (hi[D - 1] + (hi[D - 1] - lo[D - 1]) - mu[D - 1]) / sd[D - 1]
    if nan:
        x0[2] = x0[2] * np.float32(0.25)
        x0[2, 0] = np.nan
    return x0


def lk(name):
    return 0 if name == 'rosenbrock' else -1


def check_moves(pos, lp, u, move, D, what, extra=()):
    """pos [C, S + 1, D] and lp [C, S + 1]: the start, then the state after every step, as the kernel stored them.  A row a step did
    not move is the previous row bit for bit (lp and every array of `extra` too); a moved walker's stored lp satisfy the kernel's own
    acceptance inequality in float64, factor + lp_new - lp_old > log u3 (factor: (D - 1) log zz of a stretch step, 0 of a DE step and
    of the random walk -- move None: every step a stretch step; move 'rw': u [S, C] is the step's uniform).  Returns moved [C, S]."""
    moved = ~np.all(fl.bits_equal(pos[:, 1:], pos[:, :-1]), axis=2)
    for name, a in (('lp', lp),) + tuple(extra):
        same = fl.bits_equal(a[:, 1:], a[:, :-1])
        same = same.reshape(same.shape[0], same.shape[1], -1).all(axis=2)
        assert np.all(same[~moved]), '%s: an unmoved row\'s %s changed' % (what, name)
    if isinstance(move, str):
        factor, logu = 0.0, np.log(u.T.astype(np.float64))
    else:
        u1, u3 = u[:, :, 0].T, u[:, :, 2].T
        s = np.float32(1.0) * u1 + np.float32(1.0)
        zz = (s * s) / np.float32(2.0)
        factor = (D - 1.0) * np.log(zz.astype(np.float64))
        if move is not None:
            factor = np.where(np.asarray(move)[None, :] == DE, 0.0, factor)
        with np.errstate(divide='ignore'):
            logu = np.log(u3.astype(np.float64))
    with np.errstate(invalid='ignore'):
        ok = factor + lp[:, 1:] - lp[:, :-1] > logu
    assert np.all(ok[moved]), '%s: %d moved walkers whose stored lp do not satisfy the acceptance inequality' % (what, int((~ok[moved]).sum()))
    return moved


def ens_draws(C, D, S, seed, moves):
    from nnest_amd.ensemble_rounds import fill_moves, fill_noise
    inds, u = (cpu(t) for t in fill_noise(C, S, seed=seed))
    if moves is None:
        return inds, u, None, None, None
    move, jb, gamma = (cpu(t) for t in fill_moves(C, D, S, moves=moves, seed=seed))
    return inds, u, move, jb, gamma


# ---- (a) the x-space ensemble: no flow, lp = safe logL(T(x)) + prior -----------------------------------------------------------------
@pytest.mark.parametrize('mix', [False, True], ids=['stretch', 'mix'])
@pytest.mark.parametrize('name,recipe,D', fl.TABLE, ids=[case_id(c) for c in fl.TABLE])
def test_x_space_ensemble(name, recipe, D, mix):
    from nnest_amd import flow
    like_id, params, sd, mu, lo, hi = setup(name, recipe, D)
    C, S, seed, moves = C_ENS, S_ENS, 7000 + D, MIX if mix else None
    x0 = start_x(D, C, sd, mu, lo, hi, nan=True)
    kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, seed=seed, like_params=params)
    begin = flow.ensemble_x_steps(like_id, x0, 0, **kw)
    res = flow.ensemble_x_steps(like_id, x0, S, moves=moves, **kw)
    inds, u, move, jb, gamma = ens_draws(C, D, S, seed, moves)
    if mix:
        assert set(move.tolist()) == {0, 1}, 'the seed must give a step of each kind'
    X = np.concatenate([x0[:, None], cpu(res['hist_x'])], axis=1)
    LP = np.concatenate([cpu(begin['lp'])[:, None], cpu(res['hist_lp'])], axis=1)
    assert np.all(fl.bits_equal(cpu(begin['x']), x0))
    what = 'x-space %s %s x_dim %d %s' % (name, recipe, D, 'mix' if mix else 'stretch')
    # every lp against the exact logL of its own row; -inf exactly where T(x) leaves the box
    rows, lps = X.reshape(-1, D), LP.reshape(-1)
    inside = fl.in_box(fl.T32(rows, sd, mu), lo, hi)
    assert np.all(lps[~inside] == -np.inf) and np.all(lps[inside] > -np.inf), what
    r_ll = fl.check_logl_of_own_x(lps[inside], rows[inside], sd, mu, name, params, what=what)
    # the out-of-box start and the NaN start
    assert LP[1, 0] == -np.inf and LP[2, 0] == fl.SAFE, (what, LP[1, 0], LP[2, 0])
    moved = check_moves(X, LP, u, move, D, what)
    # (a walker at -1e100 -- the NaN start, and at x_dim 1 a walker that left -inf for a proposal drawn through it -- takes
    # proposals that hold a NaN too: at x_dim 1 with the same bits, a move the rows cannot show)
    ok = ~np.isnan(X).any(axis=(1, 2))
    np.testing.assert_array_equal(cpu(res['n_accept'])[ok], moved.sum(1)[ok])
    assert np.all(cpu(res['n_accept'])[~ok] >= moved.sum(1)[~ok])
    assert np.all(fl.bits_equal(cpu(res['x']), X[:, -1])) and np.all(fl.bits_equal(cpu(res['lp']), LP[:, -1]))
    assert np.all(fl.bits_equal(cpu(res['tx']), fl.T32(X[:, -1], sd, mu)))
    assert 0 < moved.sum() < C * S
    note('ensemble_x_kernel', '<%d, %d, %s>' % (fl.units(D), lk(name), str(mix).lower()), name, recipe, D, logL=r_ll)


@pytest.mark.parametrize('mix', [False, True], ids=['stretch', 'mix'])
@pytest.mark.parametrize('D', [3, 33, 65, 128])
def test_x_space_ensemble_replays_rosenbrock(D, mix):
    """the decision replay of tests/test_gpu_bootstrap.py with the likelihood passed in, every step from the kernel's own previous row:
    a decision is compared unless |lnpdiff - log u3| < m, m = ten times the lp bound (tests/test_gpu_mcmc_walk.py's margin rule); at
    most 1 % may be excluded.  The seeds were picked on the CPU (fused_like_check.REPLAY_SEEDS) so that the restatement alone has no
    decision within three times the margin: nothing should be excluded."""
    from nnest_amd import flow
    x0, sd, mu, lo, hi = fl.replay_case(D)
    C, S, seed, moves = fl.REPLAY_C, fl.REPLAY_S, fl.REPLAY_SEEDS[D, mix], MIX if mix else None
    rs = fl.Restated(None, sd, mu, lo, hi, 'rosenbrock', ())
    kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, seed=seed)
    lp0 = cpu(flow.ensemble_x_steps(0, x0, 0, **kw)['lp'])   # (steps = 0: the kernel's own lp of the start)
    res = flow.ensemble_x_steps(0, x0, S, moves=moves, **kw)
    inds, u, move, jb, gamma = ens_draws(C, D, S, seed, moves)
    # the restated draws that picked the seed are the exported ones
    for i, (r_inds, r_u, r_move, r_jb, r_gamma) in enumerate(fl.ensemble_draws(seed, C, S, D, moves)):
        assert np.array_equal(r_inds, inds[i]) and np.all(fl.bits_equal(r_u, u[i])), 'step %d: the restated split or uniforms differ' % i
        if mix:
            assert r_move == move[i] and np.array_equal(r_jb, jb[i])
            np.testing.assert_allclose(r_gamma, gamma[i], rtol=3e-7, atol=0)
    hx, hl = cpu(res['hist_x']), cpu(res['hist_lp'])
    want0 = rs.lp(x0)
    fin0 = np.isfinite(want0)
    assert np.array_equal(lp0[~fin0], want0[~fin0]) and lp0[1] == -np.inf
    excluded, n_moved, worst = 0, 0, float(np.max(np.abs(lp0[fin0] - want0[fin0]) / fl.logl_bound(want0[fin0])))
    for i in range(S):
        x_prev = x0 if i == 0 else hx[:, i - 1]
        lp_prev = lp0 if i == 0 else hl[:, i - 1]
        rec = []
        if mix:
            moves_step(x_prev, lp_prev, inds[i], u[i], move[i], jb[i], gamma[i], rs.lp, record=rec)
        else:
            fl.stretch_step(x_prev, lp_prev, inds[i], u[i], rs.lp, record=rec)
        for r in rec:
            k, acc = r['walkers'], r['accept']
            border = fl.decision_shares(r, lp_prev[k]) < 1.0
            excluded += int(border.sum())
            moved = ~np.all(fl.bits_equal(hx[k, i], x_prev[k]), axis=1)
            assert np.array_equal(moved[~border], acc[~border]), 'step %d half %d: decisions differ' % (i, r['half'])
            both = moved & acc
            assert np.all(fl.bits_equal(hx[k[both], i], r['q'][both])), 'step %d half %d: proposals not bit-equal' % (i, r['half'])
            fin = both & np.isfinite(r['lp_q'])
            if fin.any():
                worst = max(worst, float(np.max(np.abs(hl[k[fin], i] - r['lp_q'][fin]) / fl.logl_bound(r['lp_q'][fin]))))
            n_moved += int(moved.sum())
            assert np.all(fl.bits_equal(hl[k[~moved], i], lp_prev[k[~moved]])), 'step %d: an unmoved lp changed' % i
    note('ensemble_x_kernel replay', '<%d, 0, %s>' % (fl.units(D), str(mix).lower()), 'rosenbrock', 'valley', D, logL=worst)
    print('x_dim %d %s: %d of %d decisions excluded, %d moved' % (D, 'mix' if mix else 'stretch', excluded, C * S, n_moved))
    assert excluded <= 0.01 * C * S
    assert worst <= 1.0 and 0 < n_moved < C * S


# ---- the flows ---------------------------------------------------------------------------------------------------------------------------
def nvp_flow(D):
    from nnest_amd import flow
    from oracle import oracle as orc
    net = flow.HipNVP(D, 16, 3, 1, seed=D)
    return net, orc.NVP(D, 16, 3, 1, net.store_packed())


def spline_flow(D, H, C):
    """a HipSpline at its random initialisation with the ActNorm layers set by its first forward, from clean points x ~ 0.5 N(0, 1)"""
    from nnest_amd.spline import HipSpline
    from oracle import oracle as orc
    sp = HipSpline(D, H, 3, seed=D + H)
    sp.forward((np.random.RandomState(D + H).normal(size=(C, D)) * 0.5).astype(np.float32))
    return sp, orc.Spline(D, H, 3, 8, 3.0, sp.store_packed(), sp.P)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / (1.0 + np.abs(b))))


_NVP_WIDE = {}


def nvp_tols(D, net, o, z0, tag='walk'):
    """(tolerance on the log-det, tolerance on x) as functions of the oracle's value; z0: the points the measurement at a wide x_dim
    starts from -- the case's own start, or (tag 'draws') the first of an importance run's own draws"""
    if D <= 50:
        return (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    if (D, tag) not in _NVP_WIDE:
        # the evaluator's error in nnest_ensemble_steps with the Gaussian likelihood at this width: twice that is allowed
        sd, mu = fl.affine('gaussian', 'main', D, D)
        box = np.full(D, 2.5, np.float32)
        ens = net.ensemble_steps(GAUSS, z0, S_ENS, t_std=sd, t_mean=mu, lo=-box, hi=box, seed=4000 + D, like_params=(CORR,))
        ez, ex, elp = cpu(ens['hist_z']).reshape(-1, D), cpu(ens['hist_x']).reshape(-1, D), cpu(ens['hist_lp']).reshape(-1)
        ok = ~np.isnan(ez).any(1)
        rs = fl.Restated(lambda q: o.inverse(np.asarray(q, np.float32)), sd, mu, -box, box)
        want = rs.lp(ez[ok])
        fin = np.isfinite(want) & np.isfinite(elp[ok])
        e_lp = float(np.max(np.abs(elp[ok][fin] - want[fin])))
        e_x = float(np.max(np.abs(ex[ok] - o.inverse(ez[ok])[0])))
        print('x_dim %d (%s): nnest_ensemble_steps with the Gaussian against the oracle: lp %.3g, x %.3g' % (D, tag, e_lp, e_x))
        assert e_lp > 0.0 and e_x > 0.0
        _NVP_WIDE[D, tag] = (e_lp, e_x)
    e_lp, e_x = _NVP_WIDE[D, tag]
    return (lambda v: 2.0 * e_lp + 0.0 * v), (lambda v: 2.0 * e_x + 0.0 * v)


def spline_tols(key, o, z):
    """one relative figure for the log-det and x: 3e-5 at the keys with a recorded figure, else tests/test_gpu_shapes.py's rule"""
    tol = SPL_TOL
    if key not in (11, 21):
        z = z[~np.isnan(z).any(1)]
        x32, ld32 = o.inverse(z)
        x64, ld64 = o.inverse(z, f64=True)
        own = max(rel(x32, x64), rel(ld32, ld64))
        tol = max(SPL_TOL, 5.0 * own)
        print('spline key %d: the float32 oracle against the float64 oracle on these rows: %.3g -> tolerance %.3g (1 + |v|)' % (key, own, tol))
    return (lambda v: tol * (1.0 + np.abs(v))), (lambda v: tol * (1.0 + np.abs(v)))


def check_rows(what, o, z, x, lp, logl, name, params, sd, mu, lo, hi, ld_tol, x_tol):
    """rows of one kernel: z [n, D], the x [n, D] and lp [n] it stored beside them, logl [n] where it exports it (else None).  x and
    lp - logL against the oracle's inverse of the kernel's own z; logL against the exact function of the kernel's own x; the box by
    the kernel's own x.  A row whose z holds a NaN has no log-det: its logL must be -1e100.  Returns the worst error / bound of x,
    logL (0 where it is not exported) and lp - logL."""
    z, x = np.asarray(z, np.float32), np.asarray(x, np.float32)
    lp = np.asarray(lp, np.float64)
    nan = np.isnan(z).any(1)
    r_ll = 0.0
    if logl is not None:
        r_ll = fl.check_logl_of_own_x(logl, x, sd, mu, name, params, what=what)
        assert np.all(np.asarray(logl)[nan] == fl.SAFE), what
    z, x, lp = z[~nan], x[~nan], lp[~nan]
    xo, ldo = o.inverse(z)
    r_x = float(np.max(np.abs(x - xo) / x_tol(xo)))
    assert r_x <= 1.0, '%s: x against the oracle: %.3g of the bound' % (what, r_x)
    exact = fl.exact_logl(name, fl.T32(x, sd, mu), params)
    ll = exact if logl is None else np.asarray(logl, np.float64)[~nan]
    bound = ld_tol(ldo) + (fl.logl_bound(exact) if logl is None else 0.0)
    r_ld = fl.check_lp_split(lp, ll, ldo, fl.in_box(fl.T32(x, sd, mu), lo, hi), bound, what=what)
    return r_x, r_ll, r_ld


def start_z(net, D, C, sd, mu, lo, hi, nan=False):
    z0, _ = net.forward(start_x(D, C, sd, mu, lo, hi, nan=nan))
    return z0.contiguous()


def run_latent_ensemble(kernel, inst, net, o, name, recipe, D, C, moves, ld_tol_of):
    like_id, params, sd, mu, lo, hi = setup(name, recipe, D)
    S = S_ENS
    seed = 7100 + D if moves is None else fl.seed_with_both_moves(7100 + D, S, moves)
    z0 = start_z(net, D, C, sd, mu, lo, hi)
    ld_tol, x_tol = ld_tol_of(z0)
    kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, seed=seed, like_params=params)
    begin = net.ensemble_steps(like_id, z0, 0, **kw)
    res = net.ensemble_steps(like_id, z0, S, moves=moves, **kw)
    inds, u, move, jb, gamma = ens_draws(C, D, S, seed, moves)
    if moves is not None:
        assert set(move.tolist()) == {0, 1}, 'the seed must give a step of each kind'
    Z = np.concatenate([cpu(z0)[:, None], cpu(res['hist_z'])], axis=1)
    X = np.concatenate([cpu(begin['x'])[:, None], cpu(res['hist_x'])], axis=1)
    LP = np.concatenate([cpu(begin['lp'])[:, None], cpu(res['hist_lp'])], axis=1)
    what = '%s %s %s x_dim %d' % (kernel, name, recipe, D)
    r_x, _, r_ld = check_rows(what, o, Z.reshape(-1, D), X.reshape(-1, D), LP.reshape(-1), None, name, params, sd, mu, lo, hi, ld_tol, x_tol)
    assert LP[1, 0] == -np.inf, what   # the out-of-box start
    moved = check_moves(Z, LP, u, move, D, what, extra=(('x', X),))
    np.testing.assert_array_equal(cpu(res['n_accept']), moved.sum(1))
    for key, a in (('z', Z), ('x', X), ('lp', LP)):
        assert np.all(fl.bits_equal(cpu(res[key]), a[:, -1])), key
    assert 0 < moved.sum() < C * S
    note(kernel, inst, name, recipe, D, x=r_x, lp_minus_logL=r_ld)


# Rosenbrock at both recipes and U = 1 .. 4, the other six at one width each, together U = 1 .. 4 of the generic instantiation
NVP_TABLE = [('rosenbrock', 'valley', 5), ('rosenbrock', 'wide', 33), ('rosenbrock', 'valley', 70), ('rosenbrock', 'wide', 128),
             ('gaussmix', 'main', 20), ('himmelblau', 'main', 66), ('gaussian', 'main', 100), ('shell', 'main', 40),
             ('double_shell', 'main', 97), ('eggbox', 'main', 2)]
# (x_dim, hidden) -> key 10 NT + NH; Rosenbrock at every key, the other six spread over them
SPLINE_KEYS = {(5, 16): 11, (40, 16): 21, (70, 16): 31, (128, 16): 41, (8, 32): 12, (40, 32): 22, (2, 16): 11}
SPLINE_TABLE = ([('rosenbrock', 'valley', D, H) for D, H in SPLINE_KEYS if D > 2] + [('rosenbrock', 'wide', 128, 16), ('eggbox', 'main', 2, 16)]
                + [('gaussmix', 'main', 5, 16), ('shell', 'main', 40, 16), ('himmelblau', 'main', 70, 16), ('gaussian', 'main', 128, 16),
                   ('double_shell', 'main', 8, 32), ('gaussian', 'main', 40, 32)])


def test_tables_reach_every_instantiation():
    assert {(fl.units(D), lk(n)) for n, _, D in NVP_TABLE} == {(U, k) for U in (1, 2, 3, 4) for k in (0, -1)}
    assert {(fl.units(D), lk(n)) for n, _, D in fl.TABLE} == {(U, k) for U in (1, 2, 3, 4) for k in (0, -1)}
    for (D, H), key in SPLINE_KEYS.items():
        assert 10 * fl.units(D) + H // 16 == key
    assert {SPLINE_KEYS[D, H] for n, _, D, H in SPLINE_TABLE if n == 'rosenbrock'} == {11, 21, 31, 41, 12, 22}
    assert {SPLINE_KEYS[D, H] for n, _, D, H in SPLINE_TABLE if n != 'rosenbrock'} == {11, 21, 31, 41, 12, 22}
    assert {n for n, _, _, _ in SPLINE_TABLE} == set(fl.LIKES) == {n for n, _, _ in NVP_TABLE}


# ---- (b) the latent NVP ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mix', [False, True], ids=['stretch', 'mix'])
@pytest.mark.parametrize('name,recipe,D', NVP_TABLE, ids=[case_id(c) for c in NVP_TABLE])
def test_nvp_ensemble(name, recipe, D, mix):
    net, o = nvp_flow(D)
    run_latent_ensemble('ensemble_kernel', '<%d, %d, %s>' % (fl.units(D), lk(name), str(mix).lower()), net, o, name, recipe, D, C_ENS,
                        MIX if mix else None, lambda z0: nvp_tols(D, net, o, z0))


# ---- (e) the spline ensemble ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,recipe,D,H', SPLINE_TABLE, ids=[case_id(c) for c in SPLINE_TABLE])
def test_spline_ensemble(name, recipe, D, H):
    key = SPLINE_KEYS[D, H]
    sp, o = spline_flow(D, H, C_SPL)
    run_latent_ensemble('spline_ensemble_kernel_team', 'key %d' % key, sp, o, name, recipe, D, C_SPL, None,
                        lambda z0: spline_tols(key, o, cpu(z0)))


# ---- (c) random-walk Metropolis ------------------------------------------------------------------------------------------------------------
def run_mcmc(kernel, inst, net, o, name, recipe, D, C, tols_of):
    from nnest_amd import flow
    like_id, params, sd, mu, lo, hi = setup(name, recipe, D)
    S, seed, step = S_MCMC, 7200 + D, 1.0 / np.sqrt(D)
    z0 = start_z(net, D, C, sd, mu, lo, hi, nan=True)
    ld_tol, x_tol = tols_of(z0)
    kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, seed=seed, like_params=params)
    what = '%s %s %s x_dim %d' % (kernel, name, recipe, D)
    # steps = 0: the evaluator
    begin = net.mcmc_steps(like_id, z0, 0, step, **kw)
    r0 = check_rows(what + ' start', o, cpu(z0), cpu(begin['x']), cpu(begin['lp']), cpu(begin['logl']), name, params, sd, mu, lo, hi, ld_tol, x_tol)
    assert float(begin['lp'][1]) == -np.inf and float(begin['logl'][2]) == fl.SAFE, what   # the out-of-box start, the NaN start
    # the steps, one launch each, so that lp after every step comes back; and in one launch: the same run, bit for bit
    Z, X, LL, LP = [cpu(z0)], [cpu(begin['x'])], [cpu(begin['logl'])], [cpu(begin['lp'])]
    z, lp, logl, n_acc = z0, begin['lp'], begin['logl'], 0
    for i in range(S):
        r = net.mcmc_steps(like_id, z, 1, step, lp=lp, logl=logl, step0=i, **kw)
        z, lp, logl = r['z'], r['lp'], r['logl']
        n_acc = n_acc + cpu(r['n_accept'])
        Z.append(cpu(r['hist_z'])[:, 0]); X.append(cpu(r['hist_x'])[:, 0]); LL.append(cpu(r['hist_logl'])[:, 0]); LP.append(cpu(lp))
    Z, X, LL, LP = (np.stack(v, axis=1) for v in (Z, X, LL, LP))
    one = net.mcmc_steps(like_id, z0, S, step, **kw)
    ok = ~np.isnan(cpu(z0)).any(1)   # (NaN != NaN bit patterns aside, the NaN walker never moves)
    for key, a in (('hist_z', Z[:, 1:]), ('hist_x', X[:, 1:]), ('hist_logl', LL[:, 1:])):
        assert np.all(fl.bits_equal(cpu(one[key])[ok], a[ok])), key
    assert np.all(fl.bits_equal(cpu(one['lp'])[ok], LP[ok, -1]))
    np.testing.assert_array_equal(cpu(one['n_accept']), n_acc)
    r1 = check_rows(what, o, Z[:, 1:].reshape(-1, D), X[:, 1:].reshape(-1, D), LP[:, 1:].reshape(-1), LL[:, 1:].reshape(-1), name, params,
                    sd, mu, lo, hi, ld_tol, x_tol)
    _, u = (cpu(t) for t in flow.mcmc_fill_noise(S, C, D, seed=seed))
    moved = check_moves(Z[ok], LP[ok], u[:, ok], 'rw', D, what, extra=(('x', X[ok]), ('logL', LL[ok])))
    # (the NaN walker: through the NVP its log-det and so its lp are NaN and it never moves; the spline's log-det of a NaN is the
    # tails' 0, its lp stays -1e100 and it takes every proposal, NaN for NaN: either way no other walker sees it)
    np.testing.assert_array_equal(n_acc[ok], moved.sum(1))
    assert 0 < moved.sum() < C * S
    note(kernel, inst, name, recipe, D, x=max(r0[0], r1[0]), logL=max(r0[1], r1[1]), lp_minus_logL=max(r0[2], r1[2]))


@pytest.mark.parametrize('name,recipe,D', NVP_TABLE, ids=[case_id(c) for c in NVP_TABLE])
def test_nvp_mcmc(name, recipe, D):
    net, o = nvp_flow(D)
    run_mcmc('mcmc_kernel', '<%d, %d>' % (fl.units(D), lk(name)), net, o, name, recipe, D, C_ENS, lambda z0: nvp_tols(D, net, o, z0))


@pytest.mark.parametrize('name,recipe,D,H', SPLINE_TABLE, ids=[case_id(c) for c in SPLINE_TABLE])
def test_spline_mcmc(name, recipe, D, H):
    key = SPLINE_KEYS[D, H]
    sp, o = spline_flow(D, H, C_SPL)
    run_mcmc('spline_mcmc_kernel_team', 'key %d' % key, sp, o, name, recipe, D, C_SPL, lambda z0: spline_tols(key, o, cpu(z0)))


# ---- (d) importance sampling ---------------------------------------------------------------------------------------------------------------
def run_importance(kernel, inst, net, o, name, recipe, D, x_sd, tols_of):
    like_id, params, sd, mu, lo, hi = setup(name, recipe, D, x_sd=x_sd)
    M, seed = M_IMP, 7300 + D
    res = net.importance_evidence(like_id, M, t_std=sd, t_mean=mu, lo=lo, hi=hi, seed=seed, like_params=params, want_samples=True)
    z, x, logl, logw = (cpu(res[k]) for k in ('z', 'x', 'logl', 'logw'))
    ld_tol, x_tol = tols_of(z)
    what = '%s %s %s x_dim %d' % (kernel, name, recipe, D)
    # logw = lp - logb(z) with logb in float64 on both sides: lp comes back to a rounding of float64
    with np.errstate(invalid='ignore'):
        lp = logw + ic.logb(z)
    r_x, r_ll, r_ld = check_rows(what, o, z, x, lp, logl, name, params, sd, mu, lo, hi, ld_tol, x_tol)
    live = ic.is_live(logw)
    print('%s: %d of %d samples live' % (what, int(live.sum()), M))
    assert live.sum() > 0
    # the reduction: the sums against float64 sums of the kernel's own logw
    a, s1, s2, n = (float(v) for v in cpu(res['sums']))
    ra, rs1, rs2, rn = ic.sums(logw)
    assert a == ra and n == rn, (what, a, ra, n, rn)
    assert s1 == pytest.approx(rs1, rel=1e-12) and s2 == pytest.approx(rs2, rel=1e-12), what
    note(kernel, inst, name, recipe, D, x=r_x, logL=r_ll, lp_minus_logL=r_ld)


@pytest.mark.parametrize('name,recipe,D', NVP_TABLE, ids=[case_id(c) for c in NVP_TABLE])
def test_nvp_importance(name, recipe, D):
    net, o = nvp_flow(D)
    run_importance('importance_kernel', '<%d, %d>' % (fl.units(D), lk(name)), net, o, name, recipe, D, 1.0,
                   lambda z: nvp_tols(D, net, o, cuda(z[:C_ENS]), tag='draws'))


@pytest.mark.parametrize('name,recipe,D,H', SPLINE_TABLE, ids=[case_id(c) for c in SPLINE_TABLE])
def test_spline_importance(name, recipe, D, H):
    key = SPLINE_KEYS[D, H]
    sp, o = spline_flow(D, H, C_SPL)
    run_importance('spline_importance_kernel_team', 'key %d' % key, sp, o, name, recipe, D, 0.5, lambda z: spline_tols(key, o, z))


# ---- the front ends' wiring of hip_like_id / hip_like_params into the fused routes ----------------------------------------------------------
def like_classes():
    from nnest_amd import likelihoods as L
    return {'rosenbrock': (lambda: L.Rosenbrock(4), 'valley'), 'gaussmix': (lambda: L.GaussianMix(4), 'main'),
            'himmelblau': (lambda: L.Himmelblau(4), 'main'), 'gaussian': (lambda: L.Gaussian(4, 0.5), 'main'),
            'eggbox': (lambda: L.Eggbox(2), 'main'), 'shell': (lambda: L.GaussianShell(4, sigma=0.1, rshell=2.0, center=0.0), 'main'),
            'double_shell': (lambda: L.DoubleGaussianShell(4, sigmas=(0.1, 0.2), rshells=(2.0, 1.5), centers=(-1.0, 1.0)), 'main')}


def class_logl(like, tx32):
    """the class's own float64 loglike of the float32 T(x), with the safe rule"""
    v = np.asarray(like.loglike_rows(np.asarray(tx32, np.float32).astype(np.float64)), np.float64)
    return np.where(np.isfinite(v), v, fl.SAFE)


@pytest.mark.parametrize('name', sorted(fl.LIKES))
def test_front_ends_hand_the_likelihood_to_the_fused_routes(tmp_path, name):
    """EnsembleSampler and MCMCSampler.run(route='fused') on an untrained NVP flow with every likelihood class that has a
    hip_like_id: the fused route is taken, and what it reports is the class's own float64 loglike of T(x) of the samples it reports
    beside it -- a wrong id, parameter order or scale in sampler.py is off by O(1).  The transform is the run's own, x * std + mean of
    the training samples, in the float32 the kernels apply it in."""
    import nnest_amd
    from oracle import oracle as orc
    make, recipe = like_classes()[name]
    like = make()
    D = like.x_dim
    assert like.hip_like_id == fl.LIKES[name]['id']
    t_sd, t_mu = fl.affine(name, recipe, D, D, 1.0)
    train = np.random.RandomState(5).normal(size=(500, D)) * t_sd + t_mu
    sd32, mu32 = np.std(train, axis=0).astype(np.float32), np.mean(train, axis=0).astype(np.float32)
    np.random.seed(3)
    torch.manual_seed(3)
    kept = {}

    def spy(s, attr):
        run = getattr(s, attr)

        def wrapped(*a, **kw):
            kept[attr] = run(*a, **kw)
            return kept[attr]
        setattr(s, attr, wrapped)

    # the ensemble: loglikes is the latent target, lp = logL + log|det| (no prior): lp - logL against the oracle's log-det
    s = nnest_amd.EnsembleSampler(D, like, log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, jitter=0.0, **kw: None   # (the flow stays at its initialisation)
    spy(s, '_ensemble_sample')
    s.run(8, 32, train)
    assert s.ensemble_route == 'fused'
    x, z, _, lp, _ = kept['_ensemble_sample']
    np.testing.assert_array_equal(s.samples[:, :, :D], s.transform(x))
    np.testing.assert_array_equal(s.loglikes, lp)
    o = orc.NVP(D, 16, 3, 1, s.trainer.netG.store_packed())
    xo, ldo = o.inverse(z.reshape(-1, D))
    assert np.max(np.abs(x.reshape(-1, D) - xo)) <= 5e-5
    ll = class_logl(like, fl.T32(x.reshape(-1, D), sd32, mu32))
    r_ens = fl.check_lp_split(lp.reshape(-1), ll, ldo, np.ones(len(ll), bool), fl.logl_bound(ldo) + fl.logl_bound(ll), what='EnsembleSampler ' + name)
    assert 0 < s.total_accepted < 32 * 8
    # random-walk Metropolis: loglikes is logL
    s = nnest_amd.MCMCSampler(D, like, log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, jitter=0.0, **kw: None
    spy(s, '_mcmc_sample_device')
    s.run(8, 32, train, route='fused', seed=4)
    assert s.mcmc_route == 'fused'
    x, _, _, logl, _, _ = kept['_mcmc_sample_device']
    np.testing.assert_array_equal(s.samples[:, :, :D], s.transform(x))
    np.testing.assert_array_equal(s.loglikes, logl)
    ll = class_logl(like, fl.T32(x.reshape(-1, D), sd32, mu32))
    r_mcmc = float(np.max(np.abs(logl.reshape(-1) - ll) / fl.logl_bound(ll)))
    assert r_mcmc <= 1.0, (name, r_mcmc)
    assert 0 < s.total_accepted < 32 * 8
    note('front ends', 'EnsembleSampler/MCMCSampler', name, recipe, D, lp_minus_logL=r_ens, logL=r_mcmc)
