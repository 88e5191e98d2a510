"""GPU checks of the adaptive walk (include/nnest_hip.h nnest_mcmc_adapt_steps, nnest_spline_mcmc_adapt_steps; HipNVP.mcmc_steps and
HipSpline.mcmc_steps with step_in / adapt_steps, Sampler._mcmc_sample_device and MCMCSampler.run with adapt_steps, SMCSampler.run with
adapt_fraction): with the adaptation off the kernels are the mixed walk's bit for bit, at a common step and at per-walker steps; with
it on, both kernels against the numpy restatement (tests/mcmc_adapt_check.py) on their exported draws, step by step from the
kernel's own previous row, and the walkers' steps against the rule replayed from the kernel's own decisions, bit for bit; a run cut
into launches (the steps handed on) or into shards is the same run; the rule finds the target acceptance, the frozen chains keep an
exactly sampled target and jump further than at the fixed start step; the front ends.

Tolerances on lp, logL and x are tests/test_gpu_mcmc_mixed.py's, for the same evaluators at the same shapes and boxes (its docstring
has them): NVP x_dim <= 50 rtol 1e-6, atol 2e-5 on lp and logL, 5e-5 on x; NVP x_dim 70 and 100 twice the error the test measures
of nnest_ensemble_steps at that width (logL of the start rows outside the box: the same kernel's error with the box off); spline
3e-5 in |a - b| / (1 + |b|).  A decision is compared unless its margin is within ten times the lp tolerance; at most 1 % of the 560
may be excluded.  The seeds were chosen on the CPU (tools/mcmc_adapt_cases.py): the restatement alone leaves at most 0.25 % that
close."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mcmc_adapt_check as ac
from tests.slice_invariance import assert_invariant, stationarity_pvalues
from tests.test_gpu_mcmc_mixed import (CORR, ENDS, GAUSS, HIST, REPLAY as MIXED_REPLAY, ROSEN2_LOGZ, SPL_TOL, TRAIN_EPOCHS, Restated,
                                       _flow_and_start, _mixed_entry, _train, affine, err, exact_gauss_box, in_box, spline_and_start)

pytestmark = pytest.mark.gpu

BOTH = ('n_accept', 'n_accept_global')


def _adapt_entry(net, z0, S, step, k, beta, sd, mu, half, seed, step_in=None, adapt_steps=0, rate=1.0, target=0.234, history=True,
                 hist_step=True, step0=0, offset=0):
    """the adaptive entry itself, at any arguments (mcmc_steps keeps adapt_steps = 0 without a step_in on the existing entries)"""
    from nnest_amd import _lib
    from nnest_amd.flow import target_vectors
    dev = z0.device
    C, D = z0.shape
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    t_std, t_mean, lo, hi = target_vectors('mcmc_steps', dev, sd, mu, -np.full(D, half), np.full(D, half), D=D)
    out = dict(z=torch.empty(C, D, **f32), x=torch.empty(C, D, **f32), lp=torch.empty(C, **f64), logl=torch.empty(C, **f64),
               hist_z=torch.empty(C, S, D, **f32) if history else None, hist_x=torch.empty(C, S, D, **f32) if history else None,
               hist_logl=torch.empty(C, S, **f64) if history else None, n_accept=torch.empty(C, dtype=torch.int32, device=dev),
               n_accept_global=torch.empty(C, dtype=torch.int32, device=dev), step=torch.full((C,), -3.0, **f64),
               hist_step=torch.full((C, S), -3.0, **f64) if hist_step else None)
    lk = _lib.like_spec(GAUSS, 1.0, (CORR,))
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc_adapt'](
            net._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(z0), None, None,
            _lib.ptr(out['z']), _lib.ptr(out['x']), _lib.ptr(out['lp']), _lib.ptr(out['logl']), _lib.ptr(out['hist_z']),
            _lib.ptr(out['hist_x']), _lib.ptr(out['hist_logl']), _lib.ptr(out['n_accept']), C, S, ctypes.c_float(step), step0, seed, offset,
            ctypes.c_double(beta), k, _lib.ptr(out['n_accept_global']), _lib.ptr(step_in), _lib.ptr(out['step']), _lib.ptr(out['hist_step']),
            ctypes.c_uint32(adapt_steps), ctypes.c_double(rate), ctypes.c_double(target), _lib.current_stream(dev)))
    return out


# ---- 1. with the adaptation off the kernels are the mixed walk's ------------------------------------------------------------------
@pytest.mark.parametrize('name,D', [('nvp', 5), ('nvp', 70), ('spline', 5)])
def test_off_is_the_mixed_walk_bit_for_bit(name, D):
    C, S, step, half = 70, 6, 1.0 / np.sqrt(D), 2.5
    net, z0 = _flow_and_start(name, D, C, D)
    sd, mu = affine(D, D)
    step64 = float(np.float32(step))   # (double)step_size
    for k, beta in ((0, 1.0), (2, 0.5)):
        old = _mixed_entry(net, z0, S, step, k, beta, sd, mu, half, 77)
        assert 0 < int(old['n_accept'].sum()) < C * S
        for step_in in (None, torch.full((C,), step64, dtype=torch.float64, device=z0.device)):
            new = _adapt_entry(net, z0, S, step, k, beta, sd, mu, half, 77, step_in=step_in)
            for key in HIST + ENDS + BOTH:
                assert torch.equal(new[key], old[key]), (key, k, beta, step_in is None)
            assert bool((new['step'] == step64).all()) and bool((new['hist_step'] == step64).all())
    # mcmc_steps without the new keywords is the existing call: no new key
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=77, like_params=(CORR,))
    plain = net.mcmc_steps(GAUSS, z0, 2, step, adapt_steps=0, step_in=None, **kw)
    assert 'step' not in plain and 'hist_step' not in plain and 'n_accept_global' not in plain


# ---- 2. frozen per-walker steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_frozen_steps_of_their_own(name):
    """step_in holds three values, adapt_steps = 0: every group of rows runs as the same rows of a mixed launch of the whole batch at
    that step"""
    D, C, S, k, beta, half = 5, 70, 6, 2, 0.5, 2.5
    net, z0 = _flow_and_start(name, D, C, D)
    sd, mu = affine(D, D)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=78, like_params=(CORR,), global_every=k, beta=beta)
    values = [float(np.float32(v)) for v in (0.15, 0.45, 1.3)]
    group = np.arange(C) % 3
    step_in = torch.tensor([values[g] for g in group], dtype=torch.float64, device=z0.device)
    new = net.mcmc_steps(GAUSS, z0, S, 99.0, step_in=step_in, **kw)   # (step_size is not used where step_in is given)
    assert torch.equal(new['step'], step_in) and torch.equal(new['hist_step'], step_in[:, None].expand(C, S))
    seen = []
    for g, v in enumerate(values):
        old = net.mcmc_steps(GAUSS, z0, S, v, **kw)
        rows = torch.from_numpy(group == g).to(z0.device)
        for key in HIST + ENDS + BOTH:
            assert torch.equal(new[key][rows], old[key][rows]), (key, v)
        seen.append(int(old['n_accept'][rows].sum()) - int(old['n_accept_global'][rows].sum()))
    assert seen[0] > seen[2] > 0   # (the steps matter: the small one is accepted more often)


# ---- 3. the replay on the kernel's own draws ----------------------------------------------------------------------------------------
S_REPLAY, K_REPLAY, A_REPLAY, RATE, TARGET = 8, 3, 5, 1.0, 0.234
# (flow, x_dim, walker_offset): seed -- tools/mcmc_adapt_cases.py; box and start scale are the mixed walk's replay's
REPLAY_SEED = {('nvp', 5, 0): 7005, ('nvp', 50, 1000): 7050, ('nvp', 70, 0): 7071, ('nvp', 100, 0): 7100, ('spline', 5, 0): 7005,
               ('spline', 40, 0): 7043}


def check_adapt_replay(net, rs, z0, step, seed, offset, tol, x_tol, what, tol_outside=None):
    """every step replayed from the kernel's own previous row and the kernel's own steps, which are first held, bit for bit, to the
    rule replayed from the kernel's own decisions (row moved or not).  tol, x_tol, tol_outside: as tests/test_gpu_mcmc_mixed.py's
    check_replay takes them"""
    from nnest_amd import flow
    C, D = z0.shape
    S, k, A = S_REPLAY, K_REPLAY, A_REPLAY
    kw = dict(t_std=rs.sd, t_mean=rs.mu, lo=-np.full(D, rs.half), hi=np.full(D, rs.half), seed=seed, walker_offset=offset,
              like_params=(CORR,))
    begin = net.mcmc_steps(GAUSS, z0, 0, step, **kw)
    res = net.mcmc_steps(GAUSS, z0, S, step, global_every=k, adapt_steps=A, adapt_rate=RATE, target_accept=TARGET, **kw)
    eps, u = (t.cpu().numpy() for t in flow.mcmc_fill_noise(S, C, D, seed=seed, walker_offset=offset))
    z0n = z0.cpu().numpy()
    hz, hx, hl, hs = (res[key].cpu().numpy() for key in ('hist_z', 'hist_x', 'hist_logl', 'hist_step'))
    # the steps: the rule on the kernel's own decisions, to the bit
    z_before = np.concatenate([z0n[:, None], hz[:, :-1]], 1)
    moved_all = np.any(hz != z_before, axis=2)
    sigma0 = np.full(C, float(np.float32(step)))
    want = ac.adapt_replay(sigma0, moved_all, k, A, RATE, TARGET)
    diff = hs.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), '%s: hist_step differs from the replayed rule at %d entries, first (row, step) %s: %r against %r' % (
        what, int(diff.sum()), tuple(np.argwhere(diff)[0]), hs[diff][0], want[diff][0])
    np.testing.assert_array_equal(res['step'].cpu().numpy(), hs[:, -1])
    assert np.unique(hs[:, A - 1]).size > 4 and np.array_equal(hs[:, A - 1:], np.repeat(hs[:, A - 1:A], S - A + 1, 1))

    x0o, _ = rs.x_of_z(z0n)
    worst_lp = err(begin['lp'].cpu().numpy(), rs.lp(z0n), tol)
    inb0 = in_box(rs.T(x0o), rs.half)
    ll0, ll0o = begin['logl'].cpu().numpy(), rs.logl(x0o)
    worst_ll = max(err(ll0[inb0], ll0o[inb0], tol), err(ll0[~inb0], ll0o[~inb0], tol_outside or tol))
    worst_x = err(begin['x'].cpu().numpy(), x0o, x_tol)
    excluded = 0
    n_moved, n_moved_g = np.zeros(C, np.int64), np.zeros(C, np.int64)
    outside_local = 0
    for i in range(S):
        g = ac.kind(i, k)
        z_prev = z_before[:, i]
        x_prev = begin['x'].cpu().numpy() if i == 0 else hx[:, i - 1]
        l_prev = begin['logl'].cpu().numpy() if i == 0 else hl[:, i - 1]
        sigma_prev = sigma0 if i == 0 else hs[:, i - 1]
        lp_prev = rs.lp(z_prev)
        rec = {}
        ac.mixed_step(i, k, z_prev, lp_prev, eps[i], u[i], ac.step_f32(sigma_prev)[:, None], rs.lp, record=rec)
        if g:   # a global proposal IS the exported draw
            assert np.array_equal(rec['q'].view(np.uint32), eps[i].view(np.uint32))
        else:   # a local one is z + float32(sigma) * eps on it
            assert np.array_equal(rec['q'], z_prev + sigma_prev.astype(np.float32)[:, None] * eps[i])
        moved = moved_all[:, i]
        with np.errstate(invalid='ignore'):
            m = 10.0 * tol(np.maximum(np.abs(np.where(np.isfinite(rec['lp_q']), rec['lp_q'], 0.0)),
                                      np.abs(np.where(np.isfinite(lp_prev), lp_prev, 0.0))))
            border = np.abs(rec['margin']) < m   # (a NaN margin -- from -inf to -inf -- is no borderline case: both refuse)
        excluded += int(border.sum())
        assert np.array_equal(moved[~border], rec['accept'][~border]), '%s step %d: decisions differ' % (what, i)
        # moved rows: the proposal, bit for bit; x and logL against the restatement
        assert np.array_equal(hz[moved, i].view(np.uint32), rec['q'][moved].view(np.uint32)), '%s step %d: proposals not bit-equal' % (what, i)
        xq_all, _ = rs.x_of_z(rec['q'])
        if not g:
            outside_local += int((~in_box(rs.T(xq_all), rs.half)).sum())
        if moved.any():
            worst_x = max(worst_x, err(hx[moved, i], xq_all[moved], x_tol))
            worst_ll = max(worst_ll, err(hl[moved, i], rs.logl(xq_all[moved]), tol))
        # unmoved rows: the previous row, bit for bit
        for nm, now, prev in (('z', hz[:, i], z_prev), ('x', hx[:, i], x_prev)):
            assert np.array_equal(now[~moved].view(np.uint32), prev[~moved].view(np.uint32)), '%s step %d: unmoved %s changed' % (what, i, nm)
        assert np.array_equal(hl[~moved, i].view(np.uint64), l_prev[~moved].view(np.uint64)), '%s step %d: unmoved logL changed' % (what, i)
        n_moved += moved
        if g:
            n_moved_g += moved
    for key, h in (('z', hz), ('x', hx), ('logl', hl)):
        np.testing.assert_array_equal(res[key].cpu().numpy(), h[:, -1])
    np.testing.assert_array_equal(res['n_accept'].cpu().numpy(), n_moved)
    np.testing.assert_array_equal(res['n_accept_global'].cpu().numpy(), n_moved_g)
    worst_lp = max(worst_lp, err(res['lp'].cpu().numpy(), rs.lp(hz[:, -1]), tol))
    print('%s: %d of %d decisions excluded; lp %+.3g, logL %+.3g, x %+.3g over the tolerance (negative: inside); moved %d of %d, by a '
          'global step %d; local proposals outside the box %d; steps after the adapting phase %.4g .. %.4g, %d distinct'
          % (what, excluded, C * S, worst_lp, worst_ll, worst_x, int(n_moved.sum()), C * S, int(n_moved_g.sum()), outside_local,
             hs[:, -1].min(), hs[:, -1].max(), np.unique(hs[:, -1]).size))
    assert excluded <= 0.01 * C * S
    assert worst_lp <= 0.0 and worst_ll <= 0.0 and worst_x <= 0.0
    assert outside_local > 0 and 0 < int(n_moved_g.sum()) < 2 * C


def measured_tolerances(nvp, rs, z0, sd, mu, half, seed, offset):
    """x_dim 70 and 100: the tolerances tests/test_gpu_mcmc_mixed.py::test_nvp_kernel_replays_on_its_draws measures for the shape --
    twice the error of nnest_ensemble_steps against the same restatement on the start and the run's draws of 16 steps (6 ensemble
    steps), and, for logL of the start rows outside the box, twice the same kernel's error with the box off on the rows outside"""
    from nnest_amd import flow
    C, D = z0.shape
    eps, _ = flow.mcmc_fill_noise(16, C, D, seed=seed, walker_offset=offset)
    walkers = torch.cat([z0, eps.reshape(-1, D)])
    walkers = walkers[:min(len(walkers), nvp.ensemble_max_walkers(GAUSS))].contiguous()
    assert len(walkers) >= 1024
    ens = nvp.ensemble_steps(GAUSS, walkers, 6, t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=seed, like_params=(CORR,))
    ez, ex = (ens[key].cpu().numpy().reshape(-1, D) for key in ('hist_z', 'hist_x'))
    e_lp = err(ens['hist_lp'].cpu().numpy().reshape(-1), rs.lp(ez), lambda v: 0.0 * v)
    e_x = float(np.max(np.abs(ex - rs.x_of_z(ez)[0])))
    rs_open = Restated(rs.o, sd, mu, np.inf)
    ens = nvp.ensemble_steps(GAUSS, walkers, 6, t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,))
    ez = ens['hist_z'].cpu().numpy().reshape(-1, D)
    out = ~in_box(rs.T(rs.x_of_z(ez)[0]), half)
    e_out = err(ens['hist_lp'].cpu().numpy().reshape(-1)[out], rs_open.lp(ez[out]), lambda v: 0.0 * v)
    print('x_dim %d: nnest_ensemble_steps against the restatement: lp %.3g, x %.3g; without the box, on the %d rows outside it: lp %.3g'
          % (D, e_lp, e_x, int(out.sum()), e_out))
    assert e_lp > 0.0 and e_x > 0.0 and e_out > 0.0
    return (lambda v: 2.0 * e_lp + 0.0 * v), (lambda v: 2.0 * e_x + 0.0 * v), (lambda v: 2.0 * e_out + 0.0 * v)


@pytest.mark.parametrize('D,offset', [(5, 0), (50, 1000), (70, 0), (100, 0)])
def test_nvp_kernel_replays_on_its_draws(D, offset):
    from oracle import oracle as orc
    C = 70
    half, scale, _ = MIXED_REPLAY[('nvp', D, offset)]
    seed = REPLAY_SEED[('nvp', D, offset)]
    nvp, z0 = _flow_and_start('nvp', D, C, D, scale)
    sd, mu = affine(D, D)
    rs = Restated(orc.NVP(D, 16, 3, 1, nvp.store_packed()), sd, mu, half)
    if D <= 50:
        tol, x_tol, tol_outside = (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v), None
    else:
        tol, x_tol, tol_outside = measured_tolerances(nvp, rs, z0, sd, mu, half, seed, offset)
    check_adapt_replay(nvp, rs, z0, 1.0 / np.sqrt(D), seed, offset, tol, x_tol, 'nvp x_dim %d' % D, tol_outside=tol_outside)


@pytest.mark.parametrize('D', [5, 40])
def test_spline_kernel_replays_on_its_draws(D):
    C = 70
    half, scale, _ = MIXED_REPLAY[('spline', D, 0)]
    sp, o, z0 = spline_and_start(D, C, D, scale)
    sd, mu = affine(D, D)
    rs = Restated(o, sd, mu, half)
    t = lambda v: SPL_TOL * (1.0 + np.abs(v))
    check_adapt_replay(sp, rs, z0, 1.0 / np.sqrt(D), REPLAY_SEED[('spline', D, 0)], 0, t, t, 'spline x_dim %d' % D)


# ---- 4. cuts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_cuts_are_bit_exact(name):
    from nnest_amd import _lib
    D, C, k, A, half = 20, 70, 3, 5, 3.0
    net, z0 = _flow_and_start(name, D, C, 8, 1.0)
    sd, mu = affine(D, 8)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=42, like_params=(CORR,), global_every=k, adapt_steps=A)
    hist = HIST + ('hist_step',)
    ends = ENDS + ('step',)
    one = net.mcmc_steps(GAUSS, z0, 7, 0.2, **kw)
    # adapt_steps spans the cut: steps 0 .. 2 | 3 .. 6, the walkers' steps handed on
    a = net.mcmc_steps(GAUSS, z0, 3, 0.2, **kw)
    b = net.mcmc_steps(GAUSS, a['z'], 4, 0.2, lp=a['lp'], logl=a['logl'], step0=3, step_in=a['step'], **kw)
    for key in hist:
        assert torch.equal(torch.cat([a[key], b[key]], 1), one[key]), key
    for key in ends:
        assert torch.equal(b[key], one[key]), key
    for key in BOTH:
        assert torch.equal(a[key] + b[key], one[key]), key
    hs = one['hist_step']
    assert not torch.equal(a['step'], one['step']) and torch.unique(one['step']).numel() > 4   # (the second launch adapted on)
    assert torch.equal(hs[:, 2], hs[:, 1]) and torch.equal(hs[:, A:], hs[:, A - 1:A].expand(C, 7 - A))   # (step 2 global; frozen from 5)
    assert 0 < int(one['n_accept_global'].sum()) < int(one['n_accept'].sum()) < 7 * C
    # a shard
    part = net.mcmc_steps(GAUSS, z0[24:].contiguous(), 7, 0.2, walker_offset=24, **kw)
    for key in hist + ends + BOTH:
        assert torch.equal(part[key], one[key][24:]), key
    # the ends alone (no history) are the same run
    bare = net.mcmc_steps(GAUSS, z0, 7, 0.2, history=False, **kw)
    assert bare['hist_z'] is None and bare['hist_step'] is None
    for key in ends + BOTH:
        assert torch.equal(bare[key], one[key]), key
    # hist_step alone, without the history trio
    alone = _adapt_entry(net, z0, 7, 0.2, k, 1.0, sd, mu, half, 42, adapt_steps=A, history=False, hist_step=True)
    for key in ends + BOTH + ('hist_step',):
        assert torch.equal(alone[key], one[key]), key
    # steps = 0 through the C entry with every optional buffer given: z_out, the counters and step_out keep their contents
    dev = z0.device
    z_out = torch.full((C, D), 123.0, device=dev)
    n_acc = torch.full((C,), -7, dtype=torch.int32, device=dev)
    n_glob = torch.full((C,), -9, dtype=torch.int32, device=dev)
    step_out = torch.full((C,), -5.0, dtype=torch.float64, device=dev)
    step_in = torch.full((C,), 0.3, dtype=torch.float64, device=dev)
    x_out = torch.empty(C, D, device=dev)
    lp_out, ll_out = torch.empty(C, dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)
    lk = _lib.like_spec(GAUSS, 1.0, (CORR,))
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc_adapt'](net._h, ctypes.byref(lk), None, None, None, None, _lib.ptr(z0), None, None, _lib.ptr(z_out),
                                          _lib.ptr(x_out), _lib.ptr(lp_out), _lib.ptr(ll_out), None, None, None, _lib.ptr(n_acc), C, 0,
                                          ctypes.c_float(0.2), 0, 0, 0, ctypes.c_double(1.0), k, _lib.ptr(n_glob), _lib.ptr(step_in),
                                          _lib.ptr(step_out), None, ctypes.c_uint32(A), ctypes.c_double(1.0), ctypes.c_double(0.234),
                                          _lib.current_stream(dev)))
    torch.cuda.synchronize()
    assert bool((z_out == 123.0).all()) and bool((n_acc == -7).all()) and bool((n_glob == -9).all()) and bool((step_out == -5.0).all())
    start = net.mcmc_steps(GAUSS, z0, 0, 0.2, like_params=(CORR,))
    for key, t in (('x', x_out), ('lp', lp_out), ('logl', ll_out)):
        assert torch.equal(t, start[key]), key
    zero = net.mcmc_steps(GAUSS, z0, 0, 0.2, **kw)
    assert int(zero['n_accept'].sum()) == 0 and torch.equal(zero['z'], z0) and zero['hist_step'] is None
    assert bool((zero['step'] == float(np.float32(0.2))).all())
    for key in ('x', 'lp', 'logl'):
        assert torch.equal(zero[key], net.mcmc_steps(GAUSS, z0, 0, 0.2, **dict(kw, adapt_steps=0))[key]), key
    # a step_in out of range or NaN is loaded clamped
    odd = torch.tensor([float('nan'), -1.0, 1e-12, 1e5] + [0.2] * (C - 4), dtype=torch.float64, device=dev)
    got = net.mcmc_steps(GAUSS, z0, 1, 0.2, step_in=odd, **dict(kw, adapt_steps=0))['step'].cpu().numpy()
    assert np.array_equal(got[:5], [1e-8, 1e-8, 1e-8, 1e2, 0.2])


# ---- 5. it adapts, and stays exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,beta', [('nvp', None), ('spline', None), ('nvp', 0.5)])
def test_it_adapts_and_stays_exact(name, beta):
    """2000 walkers started from exact draws of N(0, Sigma / beta) in the box [-1, 1]^5, seen through T and a random flow: 100 adapting
    and 100 frozen steps, from the steps 0.02 and 5.0.  The frozen acceptance is within 0.05 of target_accept (the offsets seen on
    N(0, I) were at most 0.014; the binomial error of 2000 x 100 decisions is 0.001); the ends pass test_invariance's statistic; the
    mean squared jump of the frozen phase exceeds that of the same run at the fixed start step"""
    from nnest_amd import flow
    from nnest_amd.spline import HipSpline
    D, N, A, S, target = 5, 2000, 100, 200, 0.234
    net = flow.HipNVP(D, 16, 3, 1, seed=21) if name == 'nvp' else HipSpline(D, 16, 3, seed=21)
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(61)
    tx0 = exact_gauss_box(rng, N, D, beta or 1.0)
    z0, _ = net.forward(((tx0 - mu) / sd).astype(np.float32))   # (the spline's first forward sets the ActNorm layers from these points)
    z0 = z0.contiguous()
    kw = dict(t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=5, like_params=(CORR,))
    if beta is not None:
        kw['beta'] = beta

    def jump(first, hist_x):   # the mean squared jump in T(x) over a launch's steps
        x = torch.cat([first[:, None], hist_x], 1).double() * torch.as_tensor(sd, device=first.device).double()
        return float(((x[:, 1:] - x[:, :-1]) ** 2).sum(2).mean())

    for start in (0.02, 5.0):
        a = net.mcmc_steps(GAUSS, z0, A, start, adapt_steps=A, target_accept=target, history=False, **kw)
        b = net.mcmc_steps(GAUSS, a['z'], S - A, start, lp=a['lp'], logl=a['logl'], step0=A, step_in=a['step'], adapt_steps=A,
                           target_accept=target, **kw)
        assert torch.equal(b['step'], a['step'])   # frozen
        frozen = int(b['n_accept'].sum()) / float(N * (S - A))
        fa = net.mcmc_steps(GAUSS, z0, A, start, history=False, **kw)
        fb = net.mcmc_steps(GAUSS, fa['z'], S - A, start, lp=fa['lp'], logl=fa['logl'], step0=A, **kw)
        j_adapt, j_fixed = jump(a['x'], b['hist_x']), jump(fa['x'], fb['hist_x'])
        sig = a['step'].cpu().numpy()
        print('%s beta=%s start %g: frozen acceptance %.4f (fixed step: %.4f); geometric-mean step %.4f, sd of log step %.3f; mean squared '
              'jump %.4g (fixed step: %.4g)' % (name, beta, start, frozen, int(fb['n_accept'].sum()) / float(N * (S - A)),
                                               np.exp(np.log(sig).mean()), np.log(sig).std(), j_adapt, j_fixed))
        assert abs(frozen - target) <= 0.05
        assert j_adapt > j_fixed
        tx = b['x'].cpu().numpy() * sd + mu
        assert np.all(in_box(tx, 1.0))
        assert_invariant(stationarity_pvalues(tx, exact_gauss_box(rng, N, D, beta or 1.0)),
                         what='adaptive walk, fused, %s beta=%s start %g' % (name, beta, start))


# ---- 6. the front ends --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_front_end(tmp_path, flow_name):
    import logging
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian

    class Lines(logging.Handler):
        def __init__(self):
            logging.Handler.__init__(self)
            self.lines = []

        def emit(self, record):
            self.lines.append(record.getMessage())

    train = _train()
    like = Gaussian(2, 0.8)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(2, like, log_dir=str(tmp_path), log_level=logging.INFO, flow=flow_name)
    init = (train[:50] - train.mean(0)) / train.std(0)
    N, S, A = 50, 400, 100
    seen = Lines()
    s.logger.addHandler(seen)
    try:
        s.run(S, N, train, init_samples=init, route='fused', seed=1, adapt_steps=A)
    finally:
        s.logger.removeHandler(seen)
    assert s.mcmc_route == 'fused'
    assert s.samples.shape == (N, S + 1, 2) and s.loglikes.shape == (N, S + 1) and s.latent_samples.shape == (N, S + 1, 2)
    assert s.total_calls == N * (S + 1)
    # the books: one step a chain; the two acceptances add up to the counters
    assert s.step_sizes.shape == (N,) and np.all(np.isfinite(s.step_sizes)) and np.all(s.step_sizes > 0) and np.unique(s.step_sizes).size > N // 2
    assert s.total_accepted + s.total_rejected == N * S
    assert round(s.adapt_acceptance * N * A) + round(s.frozen_acceptance * N * (S - A)) == s.total_accepted
    moved = np.any(s.latent_samples[:, 1:] != s.latent_samples[:, :-1], axis=2)
    assert s.adapt_acceptance == moved[:, :A].mean() and s.frozen_acceptance == moved[:, A:].mean()
    print('%s: steps %.3f .. %.3f, adapting acceptance %.3f, frozen acceptance %.3f (trained flow, 2-D correlated Gaussian)' % (
        flow_name, s.step_sizes.min(), s.step_sizes.max(), s.adapt_acceptance, s.frozen_acceptance))
    assert abs(s.frozen_acceptance - 0.234) < 0.1
    assert [line for line in seen.lines if 'step adapted over' in line and 'frozen acceptance' in line]
    np.testing.assert_allclose(s.loglikes.reshape(-1), like(s.samples.reshape(-1, 2)), rtol=1e-5, atol=1e-4)
    flat = s.samples[:, 100:, :].reshape(-1, 2)
    assert np.all(np.abs(flat.mean(0)) < 0.25)
    c = np.cov(flat.T)
    assert abs(c[0, 0] - 1) < 0.3 and abs(c[1, 1] - 1) < 0.3 and abs(c[0, 1] - 0.8) < 0.3
    # the cut into launches does not change the run
    first, steps, books = s.samples.copy(), s.step_sizes.copy(), (s.adapt_acceptance, s.frozen_acceptance)
    s.trainer.train = lambda samples, jitter=0.0, **kw: None
    s.ENSEMBLE_HISTORY_BYTES = N * 24 * 37   # (37 steps a launch: adapt_steps falls inside the third)
    s.run(S, N, train, init_samples=init, route='fused', seed=1, adapt_steps=A)
    np.testing.assert_array_equal(s.samples, first)
    np.testing.assert_array_equal(s.step_sizes, steps)
    assert (s.adapt_acceptance, s.frozen_acceptance) == books


def test_front_end_refusals(tmp_path):
    import nnest_amd
    from nnest_amd.distributions import GeneralisedNormal
    from nnest_amd.likelihoods import Gaussian
    train = _train()
    s = nnest_amd.MCMCSampler(2, Gaussian(2, 0.8), log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, jitter=0.0, **k: pytest.fail('refused before training')
    for route in (None, 'host'):
        with pytest.raises(ValueError, match="adapt_steps=5 needs route='fused'"):
            s.run(5, 8, train, route=route, adapt_steps=5)
    with pytest.raises(ValueError, match='adapt_steps=-1'):
        s.run(5, 8, train, route='fused', adapt_steps=-1)
    with pytest.raises(ValueError, match='target_accept'):
        s.run(5, 8, train, route='fused', adapt_steps=5, target_accept=0.0)
    for flow_name in ('nvp', 'spline'):
        base = GeneralisedNormal(torch.zeros(2), torch.ones(2), torch.tensor(8.0))
        g = nnest_amd.MCMCSampler(2, Gaussian(2, 0.8), log_dir=str(tmp_path), log_level=30, flow=flow_name, base_dist=base)
        g.trainer.train = lambda samples, jitter=0.0, **k: pytest.fail('refused before training')
        with pytest.raises(ValueError, match='mcmc adapt: GeneralisedNormal base .*the kernel draws from N\\(0, I\\) only'):
            g.run(5, 8, train, route='fused', adapt_steps=5)
        assert 'GeneralisedNormal' in g.trainer.netG.mcmc_adapt_refusal(GAUSS)
    net = s.trainer.netG
    assert net.mcmc_adapt_refusal(GAUSS) is None
    z = torch.zeros(4, 2).cuda()
    with pytest.raises(ValueError, match='adapt_steps=-1'):
        net.mcmc_steps(GAUSS, z, 2, 0.1, adapt_steps=-1)
    from nnest_amd._lib import NnestHipError
    with pytest.raises(NnestHipError, match='adapt_rate=1.5'):
        net.mcmc_steps(GAUSS, z, 2, 0.1, adapt_steps=2, adapt_rate=1.5, like_params=(CORR,))
    with pytest.raises(NnestHipError, match='target_accept=1 '):
        net.mcmc_steps(GAUSS, z, 2, 0.1, adapt_steps=2, target_accept=1.0, like_params=(CORR,))


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_smc_with_adapted_steps(tmp_path, flow_name):
    """SMCSampler at adapt_fraction = 0.5 (the sampler's attribute: tests/test_smc_check.py pins run's argument list) on Rosenbrock
    x_dim 2: N = 512, 10 steps a stage, 6 seeds, every retraining capped.  The bound is test_smc_with_global_steps's: the mean log Z
    over the seeds within 4 of its standard errors of the exact value.  One population step is recorded for every stage."""
    import nnest_amd
    from nnest_amd.likelihoods import Rosenbrock
    from nnest_amd.priors import UniformPrior
    s = nnest_amd.SMCSampler(2, Rosenbrock(2), prior=UniformPrior(2, -5.0, 5.0), log_dir=str(tmp_path), log_level=30, flow=flow_name)
    train = s.trainer.train
    s.trainer.train = lambda samples, **kw: train(samples, max_iters=TRAIN_EPOCHS, **kw)
    logz, steps = [], []
    s.adapt_fraction = 0.5
    for seed in range(6):
        np.random.seed(seed)
        torch.manual_seed(seed)
        s.run(seed=seed, num_particles=512, mcmc_steps=10)
        assert s.smc_route == 'fused' and s.betas[-1] == 1.0
        assert len(s.step_sizes) == len(s.betas) == len(s.acceptance)
        assert all(np.isfinite(v) and v > 0.0 for v in s.step_sizes), s.step_sizes
        assert s.step_sizes[0] != s.step_sizes[-1]
        assert sum(s.logz_steps) == pytest.approx(s.logz, rel=1e-12)
        logz.append(s.logz)
        steps.append(list(s.step_sizes))
    v = np.asarray(logz)
    mean, se = float(v.mean()), float(v.std(ddof=1) / np.sqrt(len(v)))
    print('%s: log Z %.4f +- %.4f over 6 seeds (exact %.4f); population step per stage, last seed: %s; acceptance per stage: %s'
          % (flow_name, mean, se, ROSEN2_LOGZ, ['%.3f' % g for g in steps[-1]], ['%.3f' % a for a in s.acceptance]))
    assert abs(mean - ROSEN2_LOGZ) <= 4.0 * se
    assert s.samples.shape == (512, 2) and np.all(np.abs(s.samples) <= 5.0)
    # adapt_fraction = 0 leaves no step behind
    s.adapt_fraction = 0.0
    s.run(seed=0, num_particles=512, mcmc_steps=10)
    assert s.step_sizes == []


def test_smc_host_loop_refuses_adapted_steps(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Rosenbrock
    from nnest_amd.priors import UniformPrior
    like = Rosenbrock(2)
    python_like = lambda x: like(x)   # (no hip_like_id: a likelihood the kernels do not know -- the host loop's configuration)
    s = nnest_amd.SMCSampler(2, python_like, prior=UniformPrior(2, -5.0, 5.0), log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, **kw: pytest.fail('refused before training')
    s.adapt_fraction = 0.5
    for route in (None, 'host'):
        with pytest.raises(ValueError, match='adapt_fraction=0.5 needs the fused route'):
            s.run(num_particles=64, mcmc_steps=4, route=route)
    s.adapt_fraction = 1.5
    with pytest.raises(ValueError, match='adapt_fraction=1.5'):
        s.run(num_particles=64, mcmc_steps=4)
