"""GPU checks of the seven analytic likelihoods inside the TEMPERED, MIXED and ADAPTIVE walk kernels (include/nnest_hip.h
nnest_mcmc_tempered_steps, nnest_mcmc_mixed_steps, nnest_mcmc_adapt_steps and their spline counterparts) at every register shape:
mcmc_kernel<U, LK, true>, mcmc_mixed_kernel<U, LK>, mcmc_adapt_kernel<U, LK> (U = 1 .. 4, LK = 0 Rosenbrock, -1 the id read at run
time) and spline_mcmc_kernel_team<NT, NH, true>, spline_mcmc_mixed_kernel_team<NT, NH>, spline_mcmc_adapt_kernel_team<NT, NH> (keys
10 NT + NH = 11, 21, 31, 41, 12, 22).  The protocol and every tolerance are tests/test_gpu_fused_likes.py's: its tables, flows,
nvp_tols / spline_tols, check_rows and check_moves, imported.

(a) The chain.  On the same start, seed and S the plain nnest_mcmc_steps -- held to float64 on every likelihood by
    tests/test_gpu_fused_likes.py -- is, bit for bit, the tempered entry at beta = 1, the mixed entry at global_every = 0 and the
    adaptive entry with the adaptation off; at beta = 0.3 mixed(k = 0) is the tempered run and adapt(off, k = 3) the mixed one.
(b) The rich runs (tile_like_check.CONFIGS), where bit-equality cannot reach: one step a launch with lp, logL, step0 and the
    walkers' steps carried, and once in one launch -- the same bits; then every stored logL against float64 on T(x) of the x beside
    it, lp - beta logL against the oracle's log-det of the stored z, x against the oracle's inverse, a moved row's z against the
    exported draws and its stored lp against the kernel's own acceptance inequality, an unmoved row bit for bit, the counters against
    the moved rows and hist_step against the rule replayed from the kernel's own decisions.

Start: tests/test_gpu_fused_likes.start_x at the scale the transform and the box are made for (tile_like_check.walk_start_x).  Seeds:
tile_like_check.WALK_SEEDS, chosen on the CPU (tools/walk_like_cases.py) so that the restatement alone has an accepted and a refused
global proposal beyond ten times the tolerance in force.  A global step's inequality is allowed s = 1e-10 (1 + |logb_new| +
|logb_old|): the kernel adds at most 128 exact float64 squares in another order than mcmc_mixed_check.logb."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fused_like_check as fl
from tests import mcmc_adapt_check as ac
from tests import tile_like_check as tl
from tests.mcmc_mixed_check import logb
from tests.test_gpu_fused_likes import (C_ENS, C_SPL, NVP_TABLE, SPLINE_KEYS, SPLINE_TABLE, case_id, check_moves, check_rows, cpu, lk, note,
                                        nvp_flow, nvp_tols, setup, spline_flow, spline_tols, start_x)

pytestmark = pytest.mark.gpu

S, K, A, RATE, TARGET, BETA = tl.S, tl.K, tl.A, tl.RATE, tl.TARGET, tl.BETA
HIST = ('hist_z', 'hist_x', 'hist_logl')
ENDS = ('z', 'x', 'lp', 'logl')
assert C_SPL == tl.C_DATA


def test_tables_reach_every_instantiation():
    """every configuration runs every row of both tables: all eight <U, LK>, all six keys and every likelihood in each family"""
    for config in tl.CONFIGS:
        nvp = [c[1:] for c in RICH if c[0] == config]
        spl = [c[1:] for c in RICH_SPL if c[0] == config]
        assert {(fl.units(D), lk(n)) for n, _, D in nvp} == {(U, k) for U in (1, 2, 3, 4) for k in (0, -1)}, config
        assert {SPLINE_KEYS[D, H] for n, _, D, H in spl if n == 'rosenbrock'} == {11, 21, 31, 41, 12, 22}, config
        assert {SPLINE_KEYS[D, H] for n, _, D, H in spl if n != 'rosenbrock'} == {11, 21, 31, 41, 12, 22}, config
        assert {n for n, _, _, _ in spl} == set(fl.LIKES) == {n for n, _, _ in nvp}, config
    assert len(NVP_TABLE) == 10 and len(SPLINE_TABLE) == 14   # (the chain runs both tables whole)
    for (D, H), key in SPLINE_KEYS.items():
        assert tl.key(D, H) == key
    assert set(tl.WALK_SEEDS) == {('nvp',) + c for c in NVP_TABLE} | {('spline',) + c for c in SPLINE_TABLE}


def same_bits(a, b, rows=None):
    a, b = (cpu(v) if torch.is_tensor(v) else np.asarray(v) for v in (a, b))
    if rows is not None:
        a, b = a[rows], b[rows]
    return bool(np.all(fl.bits_equal(a, b)))


def raw_entry(net, like_id, params, z0, steps, step, sd, mu, lo, hi, seed, beta, k, adapt=None):
    """the mixed entry (adapt None) or the adaptive entry (adapt: dict(step_in, adapt_steps)) itself, at arguments mcmc_steps keeps on
    the older entries: tests/test_gpu_mcmc_mixed._mixed_entry and tests/test_gpu_mcmc_adapt._adapt_entry with the likelihood passed in"""
    from nnest_amd import _lib
    from nnest_amd.flow import target_vectors
    dev = z0.device
    C, D = z0.shape
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    t_std, t_mean, lo_t, hi_t = target_vectors('mcmc_steps', dev, sd, mu, lo, hi, D=D)
    out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64), logl=torch.empty(C, **f64),
               hist_z=torch.empty(C, steps, D, **f32), hist_x=torch.empty(C, steps, D, **f32), hist_logl=torch.empty(C, steps, **f64),
               n_accept=torch.empty(C, dtype=torch.int32, device=dev), n_accept_global=torch.empty(C, dtype=torch.int32, device=dev))
    tail = ()
    if adapt is not None:
        out['step'], out['hist_step'] = torch.empty(C, **f64), torch.empty(C, steps, **f64)
        tail = (_lib.ptr(adapt.get('step_in')), _lib.ptr(out['step']), _lib.ptr(out['hist_step']), ctypes.c_uint32(adapt.get('adapt_steps', 0)),
                ctypes.c_double(RATE), ctypes.c_double(TARGET))
    spec = _lib.like_spec(like_id, 1.0, params)
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc_mixed' if adapt is None else 'mcmc_adapt'](
            net._h, ctypes.byref(spec), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo_t), _lib.ptr(hi_t), _lib.ptr(z0), None, None,
            _lib.ptr(out['z']), _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']), _lib.ptr(out['hist_z']),
            _lib.ptr(out['hist_x']), _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, steps, ctypes.c_float(step), 0, seed, 0,
            ctypes.c_double(beta), k, _lib.ptr(out['n_accept_global']), *tail, _lib.current_stream(dev)))
    return out


def make_case(flow, name, recipe, D, H=16):
    x_sd, C = (1.0, C_ENS) if flow == 'nvp' else (0.5, C_SPL)
    like_id, params, sd, mu, lo, hi = setup(name, recipe, D, x_sd=x_sd)
    if flow == 'nvp':
        net, o = nvp_flow(D)
        inst = '<%d, %d>' % (fl.units(D), lk(name))
    else:
        net, o = spline_flow(D, H, C)
        inst = 'key %d' % SPLINE_KEYS[D, H]
    z0, _ = net.forward(tl.walk_start_x(start_x, D, C, sd, mu, lo, hi, x_sd))
    seed = tl.WALK_SEEDS[(flow, name, recipe, D) if flow == 'nvp' else (flow, name, recipe, D, H)]
    kw = dict(t_std=sd, t_mean=mu, lo=lo, hi=hi, seed=seed, like_params=params)
    return dict(flow=flow, net=net, o=o, inst=inst, z0=z0.contiguous(), kw=kw, like_id=like_id, params=params, sd=sd, mu=mu, lo=lo, hi=hi,
                seed=seed, name=name, recipe=recipe, D=D, H=H, C=C, step=1.0 / np.sqrt(D))


# ---- (a) the chain ---------------------------------------------------------------------------------------------------------------------
def run_chain(c):
    net, z0, kw, like_id, step = c['net'], c['z0'], c['kw'], c['like_id'], c['step']
    raw = lambda beta, k, adapt=None: raw_entry(net, like_id, c['params'], z0, S, step, c['sd'], c['mu'], c['lo'], c['hi'], c['seed'], beta, k, adapt)
    ok = ~np.isnan(cpu(z0)).any(1)   # (the NaN walker: NaN bit patterns aside, as tests/test_gpu_fused_likes.run_mcmc sets it aside)
    keys = HIST + ENDS + ('n_accept',)
    plain = net.mcmc_steps(like_id, z0, S, step, **kw)
    assert 0 < int(plain['n_accept'].sum()) < c['C'] * S
    links = [('tempered at beta = 1', plain, net.mcmc_steps(like_id, z0, S, step, beta=1.0, **kw)),
             ('mixed at global_every = 0', plain, raw(1.0, 0)),
             ('adaptive, off', plain, raw(1.0, 0, {}))]
    tempered = net.mcmc_steps(like_id, z0, S, step, beta=BETA, **kw)
    mixed = net.mcmc_steps(like_id, z0, S, step, beta=BETA, global_every=K, **kw)
    links += [('mixed at global_every = 0, beta = 0.3', tempered, raw(BETA, 0)), ('adaptive, off, k = 3, beta = 0.3', mixed, raw(BETA, K, {}))]
    for what, want, got in links:
        for key in keys + (('n_accept_global',) if want is mixed else ()):
            assert same_bits(got[key], want[key], ok), '%s %s %s x_dim %d: %s differs from the older entry: %s' % (
                c['inst'], c['name'], c['recipe'], c['D'], what, key)
        assert bool((got['logl'][~torch.from_numpy(ok).to(z0.device)] == fl.SAFE).all())
    assert int(mixed['n_accept_global'].sum()) > 0


@pytest.mark.parametrize('name,recipe,D', NVP_TABLE, ids=[case_id(c) for c in NVP_TABLE])
def test_nvp_chain(name, recipe, D):
    run_chain(make_case('nvp', name, recipe, D))


@pytest.mark.parametrize('name,recipe,D,H', SPLINE_TABLE, ids=[case_id(c) for c in SPLINE_TABLE])
def test_spline_chain(name, recipe, D, H):
    run_chain(make_case('spline', name, recipe, D, H))


# ---- (b) the rich runs -----------------------------------------------------------------------------------------------------------------
def walk_history(net, like, z0, step, kw, beta, k, adapt, spread):
    """the run one step a launch (lp, logL, step0 and the walkers' steps carried) and in one launch: the same bits.  Returns the start and
    the state after every step, Z, X [C, S + 1, D], LL, LP, SIG [C, S + 1] (SIG: the walker's step after the step; column 0 as loaded),
    the counters, and the rows compared (no NaN in the start)"""
    C, D = z0.shape
    cfg = dict(kw, beta=beta)
    if k:
        cfg['global_every'] = k
    adaptive = adapt > 0 or spread
    if adaptive:
        cfg.update(adapt_steps=adapt, adapt_rate=RATE, target_accept=TARGET)
    step_in = torch.from_numpy(tl.step_spread(C, D)).to(z0.device) if spread else None
    more = lambda s: dict(step_in=s) if adaptive and s is not None else {}
    begin = net.mcmc_steps(like, z0, 0, step, **dict(cfg, **more(step_in)))
    sigma0 = ac.clamp(cpu(step_in)) if spread else np.full(C, float(np.float32(step)))
    Z, X, LL, LP, SIG = [cpu(z0)], [cpu(begin['x'])], [cpu(begin['logl'])], [cpu(begin['lp'])], [sigma0]
    z, lp, logl, sigma = z0, begin['lp'], begin['logl'], step_in
    n_acc, n_glob = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for i in range(S):
        r = net.mcmc_steps(like, z, 1, step, lp=lp, logl=logl, step0=i, **dict(cfg, **more(sigma)))
        z, lp, logl = r['z'], r['lp'], r['logl']
        if adaptive:
            sigma = r['step']
            assert same_bits(r['hist_step'][:, 0], sigma)
        n_acc += cpu(r['n_accept'])
        n_glob += cpu(r['n_accept_global']) if k else 0
        Z.append(cpu(r['hist_z'])[:, 0]); X.append(cpu(r['hist_x'])[:, 0]); LL.append(cpu(r['hist_logl'])[:, 0]); LP.append(cpu(lp))
        SIG.append(cpu(sigma) if adaptive else sigma0)
        for key, a in (('z', Z), ('x', X), ('logl', LL)):
            assert np.all(fl.bits_equal(cpu(r[key]), a[-1]) | np.isnan(a[-1])), key
    Z, X, LL, LP, SIG = (np.stack(v, axis=1) for v in (Z, X, LL, LP, SIG))
    one = net.mcmc_steps(like, z0, S, step, **dict(cfg, **more(step_in)))
    ok = ~np.isnan(cpu(z0)).any(1)
    for key, a in (('hist_z', Z[:, 1:]), ('hist_x', X[:, 1:]), ('hist_logl', LL[:, 1:]), ('z', Z[:, -1]), ('x', X[:, -1]), ('logl', LL[:, -1]),
                   ('lp', LP[:, -1])) + ((('hist_step', SIG[:, 1:]), ('step', SIG[:, -1])) if adaptive else ()):
        assert same_bits(one[key], a, ok), 'one launch against one step a launch: %s' % key
    np.testing.assert_array_equal(cpu(one['n_accept']), n_acc)
    if k:
        np.testing.assert_array_equal(cpu(one['n_accept_global']), n_glob)
    return Z, X, LL, LP, SIG, n_acc, n_glob, ok


def check_walk(what, Z, X, LL, LP, SIG, n_acc, n_glob, ok, eps, u, k, adapt, sigma_given):
    """the steps of a run against the exported draws (eps [S, C, D], u [S, C]) on the rows `ok`; returns (local moved, local steps,
    global accepted, global proposals) over the walkers that start inside the box"""
    Z, X, LL, LP, SIG, n_acc, n_glob, eps, u = Z[ok], X[ok], LL[ok], LP[ok], SIG[ok], n_acc[ok], n_glob[ok], eps[:, ok], u[:, ok]
    D = Z.shape[2]
    moved = ~np.all(fl.bits_equal(Z[:, 1:], Z[:, :-1]), axis=2)
    for nm, a in (('x', X), ('logL', LL), ('lp', LP)):
        same = fl.bits_equal(a[:, 1:], a[:, :-1])
        same = same.reshape(same.shape[0], same.shape[1], -1).all(axis=2)
        assert np.all(same[~moved]), '%s: an unmoved row\'s %s changed' % (what, nm)
    inside = np.isfinite(LP[:, 0])
    loc = np.zeros(S, bool)
    for i in range(S):
        m = moved[:, i]
        with np.errstate(divide='ignore', invalid='ignore'):
            logu = np.log(u[i].astype(np.float64))
            if ac.kind(i, k):
                assert np.all(fl.bits_equal(Z[m, i + 1], eps[i][m])), '%s step %d: a global move is not the exported draw' % (what, i)
                b_new, b_old = logb(Z[:, i + 1]), logb(Z[:, i])
                slack = 1e-10 * (1.0 + np.abs(b_new) + np.abs(b_old))
                fine = (LP[:, i + 1] - b_new) - (LP[:, i] - b_old) > logu - slack
            else:
                loc[i] = True
                q = Z[:, i] + SIG[:, i].astype(np.float32)[:, None] * eps[i]
                assert q.dtype == np.float32
                assert np.all(fl.bits_equal(Z[m, i + 1], q[m])), '%s step %d: a local move is not z + float32(sigma) eps' % (what, i)
                fine = LP[:, i + 1] - LP[:, i] > logu
        assert np.all(fine[m]), '%s step %d: %d moved walkers whose stored lp do not satisfy the acceptance inequality' % (what, i, int((~fine[m]).sum()))
    np.testing.assert_array_equal(n_acc, moved.sum(1))
    np.testing.assert_array_equal(n_glob, moved[:, ~loc].sum(1))
    # the walkers' steps: the rule on the kernel's own decisions, to the bit; frozen from step `adapt` on
    want = ac.adapt_replay(SIG[:, 0], moved, k, adapt, RATE, TARGET)
    assert np.all(fl.bits_equal(SIG[:, 1:], want)), '%s: hist_step differs from the replayed rule' % what
    if adapt:
        assert np.all(fl.bits_equal(SIG[:, adapt:], np.repeat(SIG[:, adapt:adapt + 1], S + 1 - adapt, 1))) and np.unique(SIG[:, -1]).size > 4
        assert not np.all(fl.bits_equal(SIG[:, -1], SIG[:, 0]))
    elif not sigma_given:
        assert np.unique(SIG).size == 1
    return int(moved[inside][:, loc].sum()), int(inside.sum()) * int(loc.sum()), int(moved[inside][:, ~loc].sum()), int(inside.sum()) * int((~loc).sum())


def run_rich(c, config, tols_of):
    from nnest_amd import flow
    beta, k, adapt, spread = tl.CONFIGS[config]
    net, o, z0, D, C = c['net'], c['o'], c['z0'], c['D'], c['C']
    what = '%s %s %s %s x_dim %d' % (config, c['inst'], c['name'], c['recipe'], D)
    ld_tol, x_tol = tols_of(z0)
    Z, X, LL, LP, SIG, n_acc, n_glob, ok = walk_history(net, c['like_id'], z0, c['step'], c['kw'], beta, k, adapt, spread)
    assert LP[1, 0] == -np.inf and LL[2, 0] == fl.SAFE, what   # the out-of-box start, the NaN start
    # lp - beta logL, formed in float64 from the exported logL, in lp's place (a row at -1e100 or -inf keeps its value)
    with np.errstate(invalid='ignore'):
        lp1 = np.where(np.isfinite(LP), (LP - beta * LL) + LL, LP)
    r_x, r_ll, r_ld = check_rows(what, o, Z.reshape(-1, D), X.reshape(-1, D), lp1.reshape(-1), LL.reshape(-1), c['name'], c['params'],
                                 c['sd'], c['mu'], c['lo'], c['hi'], ld_tol, x_tol)
    eps, u = (cpu(t) for t in flow.mcmc_fill_noise(S, C, D, seed=c['seed']))
    if k == 0 and not spread:   # every step local at one step size: tests/test_gpu_fused_likes.check_moves as it stands
        check_moves(Z[ok], LP[ok], u[:, ok], 'rw', D, what, extra=(('x', X[ok]), ('logL', LL[ok])))
    local_moved, local, glob_acc, glob = check_walk(what, Z, X, LL, LP, SIG, n_acc, n_glob, ok, eps, u, k, adapt, spread)
    print('%s: local steps moved %d of %d, global proposals accepted %d of %d (walkers that start inside the box)' % (
        what, local_moved, local, glob_acc, glob))
    note({'tempered': 'mcmc_kernel<.., true>', 'mixed': 'mcmc_mixed_kernel', 'adaptive': 'mcmc_adapt_kernel'}[config] if c['flow'] == 'nvp'
         else {'tempered': 'spline_mcmc_kernel_team<.., true>', 'mixed': 'spline_mcmc_mixed_kernel_team', 'adaptive': 'spline_mcmc_adapt_kernel_team'}[config],
         c['inst'], c['name'], c['recipe'], D, x=r_x, logL=r_ll, lp_minus_logL=r_ld)
    assert 0 < local_moved < local, what
    if k:
        assert 1 <= glob_acc <= glob - 1, what


RICH = [(cfg,) + c for c in NVP_TABLE for cfg in tl.CONFIGS]
RICH_SPL = [(cfg,) + c for c in SPLINE_TABLE for cfg in tl.CONFIGS]


@pytest.mark.parametrize('config,name,recipe,D', RICH, ids=[case_id(c) for c in RICH])
def test_nvp_rich(config, name, recipe, D):
    c = make_case('nvp', name, recipe, D)
    run_rich(c, config, lambda z0: nvp_tols(D, c['net'], c['o'], z0, tag='walk at the box\'s scale'))


@pytest.mark.parametrize('config,name,recipe,D,H', RICH_SPL, ids=[case_id(c) for c in RICH_SPL])
def test_spline_rich(config, name, recipe, D, H):
    c = make_case('spline', name, recipe, D, H)
    run_rich(c, config, lambda z0: spline_tols(SPLINE_KEYS[D, H], c['o'], cpu(z0)))
