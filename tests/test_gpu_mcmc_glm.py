"""GPU checks of the regression likelihoods of user data in the fused Metropolis runs (include/nnest_hip.h nnest_loglike_glm,
nnest_mcmc_glm_steps, nnest_spline_mcmc_glm_steps; flow.loglike_glm, HipNVP.mcmc_steps and HipSpline.mcmc_steps with like_glm,
Sampler._device_target, MCMCSampler.run and SMCSampler.run on a likelihoods.GLMData):
  1. the likelihood alone against float64, within the a-priori bound B of tests/glm_check.py, and its bit-exact properties;
  2. both walk kernels replayed on their exported draws, step by step from the kernel's own previous row, as
     tests/test_gpu_mcmc_gdata.py replays the Gaussian sibling;
  3. a run cut into launches or into shards is the same run, bit for bit;
  4. walkers drawn exactly from the posterior under a box stay exact;
  5. the front ends, against a float64 grid quadrature of the posterior;
  6. the argument errors.

Data: tests/glm_check.make_data -- A uniform in +-1/sqrt(x_dim), y drawn from the model at a theta in +-1, an offset in +-0.2 --,
logl_const = -3.25.

Tolerances of the replay.  logL at the kernel's own x (hist_x, with T applied as affine_on_device applies it) is held to float64
within B alone.  The flow's part -- lp - logL against the restated log-determinant, x against the restated inverse -- takes
tests/test_gpu_mcmc_mixed.py's tolerances for the flow and width: NVP x_dim <= 50 rtol 1e-6, atol 2e-5 on lp, 5e-5 on x; NVP x_dim
70 and 100 twice the error the test measures of nnest_ensemble_steps at that width (tests/test_gpu_mcmc_adapt.py
measured_tolerances, which doubles the measured figure); spline 3e-5 in |a - b| / (1 + |b|).  A decision is compared unless the
restated margin is within ten times the lp tolerance in force: the flow's, plus B, plus the sensitivity of logL to the x tolerance
(tests/glm_check.sensitivity); at most 1 % of the 560 may be excluded.  Box, start scale and seed of each case were chosen on the
CPU (tools/mcmc_glm_cases.py): the restatement alone leaves at most 0.25 % that close, local proposals fall outside the box, and
between 15 % and 85 % of the global proposals are accepted.  The rows n of the replay are 40 and 70, not more: the bound B adds
magnitudes over the rows and the spline's lp tolerance is relative to |lp|, so with a few hundred rows ten times their sum is no
longer small beside the accept rule's margins and no seed leaves 0.25 %; cuts and shards (3.) run n = 200.

Measured on the MI355X: nnest_loglike_glm uses at most 0.155 of B (x_dim 1 and 2) down to 0.005 (logistic) and 0.007 (poisson) of B
at x_dim 128; in the replays logL is at most 0.0084 (NVP) and 0.0081 (spline) of B off float64, at most 1 of 560 decisions is
excluded per case, lp - logL and x stay inside the flows' tolerances; MCMCSampler's means are within 0.7 and its covariances within
2.8 standard errors of the quadrature; SMCSampler's log Z over 8 seeds is low by 0.04 to 0.05 on all four cases, 1.2 to 1.9 of its
standard errors, inside its bound."""
import ctypes

import numpy as np
import pytest
import torch

from tests import glm_check as gk
from tests import mcmc_adapt_check as ac
from tests.slice_invariance import assert_invariant, stationarity_pvalues
from tests.test_gpu_mcmc_mixed import ENDS, HIST, SPL_TOL, TRAIN_EPOCHS, Restated as GaussRestated, _flow_and_start, affine, err, spline_and_start

pytestmark = pytest.mark.gpu

BOTH = ('n_accept', 'n_accept_global')
LOGL0 = gk.LOGL0


# ---- 1. the likelihood alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', [1, 2, 31, 32, 33, 64, 65, 100, 128])
def test_loglike_glm(family, D):
    from nnest_amd import flow
    r = np.random.RandomState(D)
    N = 300
    t = (r.normal(size=(N, D)) * r.uniform(0.1, 3.0, size=(N, 1))).astype(np.float32)
    t[0] = 0.0
    t[1, D - 1] = np.nan
    t[2, 0] = np.inf
    worst_all = 0.0
    for n in (1, 15, 16, 17, 63, 64, 65, 200):
        like = gk.make_like(D, n, family, 1000 * D + n)
        data = dict(like.hip_like_glm)
        t[3] = 3.0e4 * np.where(data['at'][:, 0] >= 0, 1.0, -1.0)   # eta_0 = 3e4 sum_c |A[0, c]|: exp overflows float64 (poisson)
        # what lies beyond row n in the padded arrays must not matter
        ld = data['at'].shape[1]
        dirty = dict(data, at=data['at'].copy(), y=data['y'].copy(), o=data['o'].copy())
        dirty['at'][:, n:] = r.normal(size=(D, ld - n)) * 1e6
        dirty['y'][n:] = 7.0
        dirty['o'][n:] = np.nan
        got = flow.loglike_glm(dirty, t).cpu().numpy()
        want, _, _ = gk.exact(data, t)
        B = gk.bound(data, t)
        fin = np.arange(N) >= (4 if family == 'poisson' else 3)
        fin[0] = True
        assert np.all(np.isfinite(want[fin])) and np.all(want[fin] != gk.SAFE)
        worst = float(np.max(np.abs(got[fin] - want[fin]) / B[fin]))
        worst_all = max(worst_all, worst)
        assert np.all(np.abs(got[fin] - want[fin]) <= B[fin]), (n, worst)
        if family == 'logistic':
            assert np.all(got <= like.logl0)
            assert got[0] <= like.logl0 - 0.3 * n          # (softplus is log 2 at eta = 0 and at least 0.59 at |eta| <= 0.2: every row counts)
        else:
            assert got[3] == -1e100 and want[3] == gk.SAFE
        assert got[1] == -1e100 and got[2] == -1e100
        clean = flow.loglike_glm(data, t).cpu().numpy()
        assert np.array_equal(clean.view(np.uint64), got.view(np.uint64)), 'rows beyond n are not masked'
        # the same rows in another position of another launch: the same bits
        back = flow.loglike_glm(data, t[::-1].copy()).cpu().numpy()[::-1]
        assert np.array_equal(back.view(np.uint64), got.view(np.uint64))
        part = flow.loglike_glm(data, t[7:18].copy()).cpu().numpy()
        assert np.array_equal(part.view(np.uint64), got[7:18].view(np.uint64))
    print('%s x_dim %d: |logL - float64| at most %.3g of the bound B' % (family, D, worst_all))


# ---- 2. the replay on the kernel's own draws ----------------------------------------------------------------------------------------
S_REPLAY, K_REPLAY, A_REPLAY, RATE, TARGET = 8, 3, 5, 1.0, 0.234
# (flow, x_dim, walker_offset, n, family): box, start scale, seed -- tools/mcmc_glm_cases.py
REPLAY = {('nvp', 5, 0, 40, 'logistic'): (2.5, 0.5, 8005), ('nvp', 5, 0, 70, 'poisson'): (2.5, 0.5, 8005),
          ('nvp', 50, 1000, 70, 'poisson'): (3.0, 0.5, 8107), ('nvp', 50, 1000, 40, 'logistic'): (3.0, 0.5, 8051),
          ('nvp', 70, 0, 70, 'logistic'): (3.0, 0.5, 8070), ('nvp', 70, 0, 40, 'poisson'): (3.0, 1.0, 8074),
          ('nvp', 100, 0, 40, 'poisson'): (3.0, 1.0, 8150), ('nvp', 100, 0, 70, 'logistic'): (3.0, 1.0, 8130),
          ('spline', 5, 0, 40, 'poisson'): (2.5, 0.5, 8026), ('spline', 5, 0, 70, 'logistic'): (2.5, 0.5, 8005),
          ('spline', 40, 0, 70, 'logistic'): (2.5, 1.0, 8044), ('spline', 40, 0, 40, 'poisson'): (2.5, 1.0, 8043)}
# n = 40: a ragged 64-row pass and three row blocks, so that the spline's wave 3 has none; n = 70: two passes and five row blocks,
# the last of each ragged, the spline's waves holding 2, 1, 1 and 1 blocks


def check_glm_replay(net, rs, z0, step, seed, offset, tol, x_tol, what):
    """tests/test_gpu_mcmc_gdata.py check_gdata_replay on this likelihood.  tol(v): the flow's lp tolerance at value v; x_tol(v): its
    x tolerance at |x| = v"""
    from nnest_amd import flow
    from nnest_amd.device_target import affine_on_device
    C, D = z0.shape
    S, k, A = S_REPLAY, K_REPLAY, A_REPLAY
    logistic = rs.data['family'] == 'logistic'
    kw = dict(t_std=rs.sd, t_mean=rs.mu, lo=-np.full(D, rs.half), hi=np.full(D, rs.half), seed=seed, walker_offset=offset,
              like_glm=rs.data)
    begin = net.mcmc_steps(None, z0, 0, step, **kw)
    res = net.mcmc_steps(None, z0, S, step, global_every=k, adapt_steps=A, adapt_rate=RATE, target_accept=TARGET, **kw)
    eps, u = (t.cpu().numpy() for t in flow.mcmc_fill_noise(S, C, D, seed=seed, walker_offset=offset))
    z0n = z0.cpu().numpy()
    hz, hx, hl, hs = (res[key].cpu().numpy() for key in ('hist_z', 'hist_x', 'hist_logl', 'hist_step'))
    # the steps: the rule on the kernel's own decisions, to the bit
    z_before = np.concatenate([z0n[:, None], hz[:, :-1]], 1)
    moved_all = np.any(hz != z_before, axis=2)
    sigma0 = np.full(C, float(np.float32(step)))
    want = ac.adapt_replay(sigma0, moved_all, k, A, RATE, TARGET)
    diff = hs.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), '%s: hist_step differs from the replayed rule at %d entries' % (what, int(diff.sum()))
    np.testing.assert_array_equal(res['step'].cpu().numpy(), hs[:, -1])
    assert np.unique(hs[:, A - 1]).size > 4 and np.array_equal(hs[:, A - 1:], np.repeat(hs[:, A - 1:A], S - A + 1, 1))

    # logL at the kernel's own x, T applied on the device as the front ends apply it: float64 within B
    dev = z0.device
    sd_t, mu_t = torch.as_tensor(rs.sd, device=dev), torch.as_tensor(rs.mu, device=dev)
    worst_ll = -1.0
    for x_t, l_t in ((begin['x'], begin['logl']), (res['hist_x'].reshape(-1, D), res['hist_logl'].reshape(-1)), (res['x'], res['logl'])):
        t = affine_on_device(x_t, sd_t, mu_t).cpu().numpy()
        assert np.array_equal(t, rs.T(x_t.cpu().numpy()))
        ll, B = gk.exact(rs.data, t)[0], gk.bound(rs.data, t)
        got = l_t.cpu().numpy()
        assert not logistic or np.all(got <= rs.data['logl0'])
        worst_ll = max(worst_ll, float(np.max(np.abs(got - ll) / B)))
    # lp - logL on the rows inside the box (beta = 1): the restated log-determinant, within the flow's lp tolerance
    worst_ld = -1.0
    for z_n, x_t, lp_t, l_t in ((z0n, begin['x'], begin['lp'], begin['logl']), (hz[:, -1], res['x'], res['lp'], res['logl'])):
        xo, ldo = rs.x_of_z(z_n)
        inb = rs.in_prior(xo) & rs.in_prior(x_t.cpu().numpy())
        assert inb.any()
        ld = (lp_t - l_t).cpu().numpy()[inb]
        worst_ld = max(worst_ld, err(ld, np.asarray(ldo, np.float64)[inb], tol))
    x0o, _ = rs.x_of_z(z0n)
    worst_x = err(begin['x'].cpu().numpy(), x0o, x_tol)

    def like_tol(x):
        return rs.like_tol(x, x_tol(np.max(np.abs(x), axis=1)))

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
        xq_all, _ = rs.x_of_z(rec['q'])
        xp_all, _ = rs.x_of_z(z_prev)
        like = np.maximum(like_tol(xq_all), like_tol(xp_all))
        with np.errstate(invalid='ignore'):
            m = 10.0 * (tol(np.maximum(np.abs(np.where(np.isfinite(rec['lp_q']), rec['lp_q'], 0.0)),
                                       np.abs(np.where(np.isfinite(lp_prev), lp_prev, 0.0)))) + np.where(np.isfinite(like), like, 0.0))
            border = np.abs(rec['margin']) < m   # (a NaN margin -- from -inf to -inf -- is no borderline case: both refuse)
        excluded += int(border.sum())
        assert np.array_equal(moved[~border], rec['accept'][~border]), '%s step %d: decisions differ' % (what, i)
        # moved rows: the proposal, bit for bit; x against the restatement
        assert np.array_equal(hz[moved, i].view(np.uint32), rec['q'][moved].view(np.uint32)), '%s step %d: proposals not bit-equal' % (what, i)
        if not g:
            outside_local += int((~rs.in_prior(xq_all)).sum())
        if moved.any():
            worst_x = max(worst_x, err(hx[moved, i], xq_all[moved], x_tol))
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
    print('%s: %d of %d decisions excluded; logL at most %.3g of B off float64; lp - logL %+.3g, x %+.3g over the tolerance (negative: '
          'inside); moved %d of %d, by a global step %d of %d; local proposals outside the box %d'
          % (what, excluded, C * S, worst_ll, worst_ld, worst_x, int(n_moved.sum()), C * S, int(n_moved_g.sum()), 2 * C, outside_local))
    assert excluded <= 0.01 * C * S
    assert worst_ll <= 1.0 and worst_ld <= 0.0 and worst_x <= 0.0
    assert outside_local > 0 and 0.15 * 2 * C <= int(n_moved_g.sum()) <= 0.85 * 2 * C


@pytest.mark.parametrize('D,offset,n,family', [key[1:] for key in sorted(REPLAY) if key[0] == 'nvp'])
def test_nvp_kernel_replays_on_its_draws(D, offset, n, family):
    from oracle import oracle as orc
    from tests.test_gpu_mcmc_adapt import measured_tolerances
    C = 70
    half, scale, seed = REPLAY[('nvp', D, offset, n, family)]
    nvp, z0 = _flow_and_start('nvp', D, C, D, scale)
    sd, mu = affine(D, D)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    rs = gk.Restated(o, gk.replay_target(D, n, family), sd, mu, half)
    if D <= 50:
        tol, x_tol = (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    else:   # (the flow's error at this width, measured on the kernel that shares its evaluator, on its own likelihood)
        tol, x_tol, _ = measured_tolerances(nvp, GaussRestated(o, sd, mu, half), z0, sd, mu, half, seed, offset)
    check_glm_replay(nvp, rs, z0, 1.0 / np.sqrt(D), seed, offset, tol, x_tol, 'nvp x_dim %d n %d %s' % (D, n, family))


@pytest.mark.parametrize('D,n,family', [(key[1],) + key[3:] for key in sorted(REPLAY) if key[0] == 'spline'])
def test_spline_kernel_replays_on_its_draws(D, n, family):
    C = 70
    half, scale, seed = REPLAY[('spline', D, 0, n, family)]
    sp, o, z0 = spline_and_start(D, C, D, scale)
    sd, mu = affine(D, D)
    rs = gk.Restated(o, gk.replay_target(D, n, family), sd, mu, half)
    t = lambda v: SPL_TOL * (1.0 + np.abs(v))
    check_glm_replay(sp, rs, z0, 1.0 / np.sqrt(D), seed, 0, t, t, 'spline x_dim %d n %d %s' % (D, n, family))


# ---- 3. cuts and shards ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,D,n,family', [('nvp', 5, 40, 'logistic'), ('spline', 5, 40, 'poisson'), ('nvp', 70, 200, 'poisson'),
                                             ('spline', 40, 200, 'logistic')])
def test_cuts_and_shards_are_bit_exact(name, D, n, family):
    C, k, A, half = 70, 3, 5, 3.0
    net, z0 = _flow_and_start(name, D, C, 8, 1.0)
    sd, mu = affine(D, 8)
    like = gk.make_like(D, n, family, 8)
    data = like.hip_like_glm
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=42, like_glm=data, global_every=k, adapt_steps=A)
    hist = HIST + ('hist_step',)
    ends = ENDS + ('step',)
    step = 0.5 / np.sqrt(D)
    one = net.mcmc_steps(None, z0, 7, step, **kw)
    again = net.mcmc_steps(None, z0, 7, step, **kw)
    for key in hist + ends + BOTH:
        assert torch.equal(again[key], one[key]), key
    # adapt_steps spans the cut: steps 0 .. 2 | 3 .. 6, lp, logL and the walkers' steps handed on
    a = net.mcmc_steps(None, z0, 3, step, **kw)
    b = net.mcmc_steps(None, a['z'], 4, step, lp=a['lp'], logl=a['logl'], step0=3, step_in=a['step'], **kw)
    for key in hist:
        assert torch.equal(torch.cat([a[key], b[key]], 1), one[key]), key
    for key in ends:
        assert torch.equal(b[key], one[key]), key
    for key in BOTH:
        assert torch.equal(a[key] + b[key], one[key]), key
    assert torch.unique(one['step']).numel() > 4
    assert 0 < int(one['n_accept'].sum()) < 7 * C
    # a shard
    part = net.mcmc_steps(None, z0[24:].contiguous(), 7, step, walker_offset=24, **kw)
    for key in hist + ends + BOTH:
        assert torch.equal(part[key], one[key][24:]), key
    # the ends alone (no history) are the same run
    bare = net.mcmc_steps(None, z0, 7, step, history=False, **kw)
    assert bare['hist_z'] is None and bare['hist_step'] is None
    for key in ends + BOTH:
        assert torch.equal(bare[key], one[key]), key
    # the keys follow the arguments, as without like_glm; steps = 0 evaluates the start
    base = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=42, like_glm=data)
    plain = net.mcmc_steps(None, z0, 2, step, **base)
    assert 'step' not in plain and 'hist_step' not in plain and 'n_accept_global' not in plain
    mixed = net.mcmc_steps(None, z0, 2, step, global_every=2, beta=0.5, **base)
    assert 'n_accept_global' in mixed and 'step' not in mixed
    zero = net.mcmc_steps(None, z0, 0, step, **kw)
    assert int(zero['n_accept'].sum()) == 0 and torch.equal(zero['z'], z0) and zero['hist_step'] is None
    assert torch.equal(zero['logl'], net.mcmc_steps(None, z0, 0, step, **base)['logl'])
    # global_every = 0 and no adaptation: a tempered random walk at beta = 1 is the plain one, bit for bit
    tempered = net.mcmc_steps(None, z0, 2, step, beta=1.0, **base)
    for key in HIST + ENDS + ('n_accept',):
        assert torch.equal(tempered[key], plain[key]), key


# ---- 4. an exactly drawn start stays exact ------------------------------------------------------------------------------------------
def exact_draws(rng, n, like, beta, half):
    """exact draws of the density proportional to L(theta)^beta on the box +-half: rejection from the uniform box against the
    maximum of the concave log-likelihood over the box (Newton on the host in float64, and a margin of 1e-6 above it)"""
    D = like.x_dim
    _, top = gk.posterior_mode(like, -half, half)
    top += 1e-6
    out, have = [], 0
    while have < n:
        th = rng.uniform(-half, half, size=(200000, D))
        ll = like.loglike_rows(th)
        assert np.all(ll <= top)
        keep = np.log(rng.uniform(size=len(th))) < beta * (ll - top)
        out.append(th[keep])
        have += int(keep.sum())
    return np.concatenate(out)[:n]


@pytest.mark.parametrize('beta', [1.0, 0.5])
@pytest.mark.parametrize('name', ['nvp', 'spline'])
@pytest.mark.parametrize('D,family', [(2, 'logistic'), (3, 'logistic'), (2, 'poisson'), (3, 'poisson')])
def test_exact_start_stays_exact(D, family, name, beta):
    from nnest_amd import flow
    from nnest_amd.spline import HipSpline
    N, S, half = 4096, 30, 3.0
    like = gk.make_like(D, 40, family, 77)
    net = flow.HipNVP(D, 16, 3, 1, seed=21) if name == 'nvp' else HipSpline(D, 16, 3, seed=21)
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(61)
    tx0 = exact_draws(rng, N, like, beta, half)
    z0, _ = net.forward(((tx0 - mu) / sd).astype(np.float32))   # (the spline's first forward sets the ActNorm layers from these points)
    res = net.mcmc_steps(None, z0.contiguous(), S, 0.5, t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=5, beta=beta,
                         global_every=3, like_glm=like.hip_like_glm, history=False)
    moved = int(res['n_accept'].sum())
    assert 0.05 * N * S < moved < 0.95 * N * S and int(res['n_accept_global'].sum()) > 0
    tx = res['x'].cpu().numpy().astype(np.float64) * sd + mu
    unit = lambda x: x / half                                   # the box as slice_invariance's unit box
    assert np.all(np.abs(unit(tx)) <= 1.0 + 1e-6)
    p = stationarity_pvalues(np.clip(unit(tx), -1.0, 1.0), unit(exact_draws(rng, N, like, beta, half)))
    print('%s %s x_dim %d beta=%g: moved %.3f of the steps; smallest p-value %.3g of %d' % (name, family, D, beta, moved / float(N * S), min(p.values()), len(p)))
    assert_invariant(p, what='glm walk, fused, %s %s x_dim %d beta=%g' % (name, family, D, beta))


# ---- 5. the front ends ----------------------------------------------------------------------------------------------------------------
def quadrature(like, lo, hi, m=801):
    """float64 grid quadrature (trapezoid) of L over the square [lo, hi]^2: (log integral, mean [2], covariance [2, 2])"""
    g = np.linspace(lo, hi, m)
    w1 = np.full(m, g[1] - g[0])
    w1[[0, -1]] *= 0.5
    X, Y = np.meshgrid(g, g, indexing='ij')
    th = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
    ll = np.concatenate([like.loglike_rows(th[i:i + 200000]) for i in range(0, len(th), 200000)])
    top = ll.max()
    w = np.exp(ll - top) * np.outer(w1, w1).reshape(-1)
    tot = w.sum()
    mean = (w[:, None] * th).sum(0) / tot
    d = th - mean
    cov = np.einsum('n,ni,nj->ij', w, d, d) / tot
    return float(top + np.log(tot)), mean, cov


def laplace_draws(like, rng, n):
    """training points: draws from the Gaussian at the mode with the inverse Hessian (they shape the flow, not the target)"""
    th, _ = gk.posterior_mode(like, -20.0, 20.0)
    eta = like.offset + like.A @ th
    w = np.exp(eta) if like.family == 'poisson' else 0.25 / np.cosh(0.5 * eta) ** 2
    cov = np.linalg.inv((like.A * w[:, None]).T @ like.A)
    return th + rng.normal(size=(n, len(th))) @ np.linalg.cholesky(cov).T


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_mcmc_front_end(tmp_path, flow_name):
    import nnest_amd
    like = gk.make_like(2, 40, 'logistic', 5)
    # (the likelihood alone is the target: it is integrable -- the classes are not separable -- and below e^-60 of its top at +-25)
    _, mean, cov = quadrature(like, -25.0, 25.0, 1001)
    rng = np.random.RandomState(3)
    N, S, A = 64, 600, 100
    train = laplace_draws(like, rng, 2000)
    init = (train[:N] - train.mean(0)) / train.std(0)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(2, like, log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.run(S, N, train, init_samples=init, route='fused', seed=1, adapt_steps=A, global_every=5)
    assert s.mcmc_route == 'fused'
    assert s.samples.shape == (N, S + 1, 2) and s.step_sizes.shape == (N,) and s.global_proposed == N * (S // 5)
    np.testing.assert_allclose(s.loglikes.reshape(-1), like(s.samples.reshape(-1, 2)), rtol=1e-5, atol=1e-4)
    # every component of the mean and of the covariance within five standard errors of the quadrature; the standard error is the
    # spread of the per-chain estimates over the independent chains / sqrt(chains), the adapting steps discarded.  (The per-chain
    # second moments are taken about the TRUE mean: about the chain's own they would be biased low by its autocorrelation.)
    x = s.samples[:, A + 1:, :].astype(np.float64)
    m = x.mean(1)
    d = x - mean
    c = np.einsum('nti,ntj->nij', d, d) / x.shape[1]
    for est, truth, what in ((m, mean, 'mean'), (c, cov, 'covariance')):
        se = est.std(0, ddof=1) / np.sqrt(N)
        off = np.abs(est.mean(0) - truth) / se
        print('%s: %s off by at most %.2f standard errors (largest standard error %.3g)' % (flow_name, what, off.max(), se.max()))
        assert np.all(off <= 5.0), (what, off)
    # the routes this likelihood has no kernel for answer as they did
    with pytest.raises(ValueError, match='importance_evidence: the fused route does not take a likelihood the kernels do not know'):
        s.importance_evidence(64, route='fused')


@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_smc_front_end(tmp_path, flow_name, family):
    """log Z of a 2-D regression under a uniform prior on [-4, 4]^2 against the grid quadrature.  Over 8 seeds the mean of log Z^ is
    within five standard errors of that, plus half the sample variance: the Jensen bias of the logarithm of an unbiased Z^.
    adapt_fraction = 0 and global_every = 0: the tempered walk at a fixed step keeps every stage's target and so Z^ unbiased
    (DESIGN.md 3.15 on adapting short stages)."""
    import nnest_amd
    from nnest_amd.priors import UniformPrior
    like = gk.make_like(2, 40, family, 5)
    lo, hi = -4.0, 4.0
    exact = quadrature(like, lo, hi)[0] - 2 * np.log(hi - lo)
    s = nnest_amd.SMCSampler(2, like, prior=UniformPrior(2, lo, hi), log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.adapt_fraction, s.global_every = 0.0, 0
    train = s.trainer.train
    s.trainer.train = lambda samples, **kw: train(samples, max_iters=TRAIN_EPOCHS, **kw)
    logz = []
    for seed in range(8):
        np.random.seed(seed)
        torch.manual_seed(seed)
        s.run(seed=seed, num_particles=512, mcmc_steps=10)
        assert s.smc_route == 'fused' and s.betas[-1] == 1.0 and s.step_sizes == []
        logz.append(s.logz)
    v = np.asarray(logz)
    mean_z, se, var = float(v.mean()), float(v.std(ddof=1) / np.sqrt(len(v))), float(v.var(ddof=1))
    print('%s %s: log Z %.4f +- %.4f over 8 seeds (quadrature %.4f, sample variance %.4f); %d stages' % (flow_name, family, mean_z, se, exact, var, len(s.betas)))
    assert abs(mean_z - exact) <= 5.0 * se + 0.5 * var
    assert s.samples.shape == (512, 2) and np.all(s.samples >= lo) and np.all(s.samples <= hi)
    # the mixed and the adaptive walk take the same kernel
    for attrs in (dict(global_every=4), dict(global_every=0, adapt_fraction=0.5), dict(global_every=4, adapt_fraction=0.5)):
        for key, val in attrs.items():
            setattr(s, key, val)
        s.run(seed=0, num_particles=256, mcmc_steps=6)
        assert s.smc_route == 'fused' and abs(s.logz - exact) < 1.0
        assert len(s.step_sizes) == (len(s.betas) if s.adapt_fraction else 0)
        assert len(s.global_acceptance) == (len(s.betas) if s.global_every else 0)


def test_refused_routes_and_a_disagreeing_descriptor(tmp_path):
    import logging
    import nnest_amd
    like = gk.make_like(3, 40, 'poisson', 5)
    train = laplace_draws(like, np.random.RandomState(3), 500)
    e = nnest_amd.EnsembleSampler(3, like, log_dir=str(tmp_path), log_level=30, flow='nvp')
    e.trainer.train = lambda samples, **kw: None
    with pytest.raises(ValueError, match='ensemble: the fused route does not take this flow, likelihood, population or move'):
        e.run(4, 16, train, route='fused')
    # a descriptor that does not describe the host callable is refused with a warning, not run
    bad = gk.make_like(3, 40, 'poisson', 5)
    bad.hip_like_glm['o'] = bad.hip_like_glm['o'] + np.float32(0.5)
    s = nnest_amd.MCMCSampler(3, bad, log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, **kw: pytest.fail('refused before training')
    seen = []

    class Lines(logging.Handler):
        def emit(self, record):
            seen.append((record.levelno, record.getMessage()))

    handler = Lines()
    s.logger.addHandler(handler)
    try:
        with pytest.raises(ValueError, match='MCMCSampler.run: the fused route does not take this transform, likelihood or prior'):
            s.run(4, 8, train, route='fused')
    finally:
        s.logger.removeHandler(handler)
    assert any(level == logging.WARNING and 'hip_like_glm disagrees with the host callable' in line for level, line in seen), seen
    # a descriptor of another dimension than the flow's: the library's words
    net = s.trainer.netG
    assert net.mcmc_glm_refusal() is None and net.mcmc_glm_refusal(3) is None
    assert "the likelihood's D=4 is not the flow's x_dim=3" in net.mcmc_glm_refusal(4)


# ---- 6. the argument errors -----------------------------------------------------------------------------------------------------------
def _raw_entry(net, spec, z0, outs, C, S, beta=1.0, k=0, rate=1.0, target=0.234, step=0.1, null_x=False):
    from nnest_amd import _lib
    dev = z0.device
    with torch.cuda.device(dev):
        return net._sym['mcmc_glm'](
            net._h, None if spec is None else ctypes.byref(spec), None, None, None, None, _lib.ptr(z0), None, None, _lib.ptr(outs['z']),
            None if null_x else _lib.ptr(outs['x']), _lib.ptr(outs['lp']), _lib.ptr(outs['logl']), None, None, None, _lib.ptr(outs['n_accept']),
            C, S, ctypes.c_float(step), 0, 1, 0, ctypes.c_double(beta), k, None, None, _lib.ptr(outs['step']), None, ctypes.c_uint32(2),
            ctypes.c_double(rate), ctypes.c_double(target), _lib.current_stream(dev))


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_argument_errors_leave_the_outputs_alone(name):
    from nnest_amd import _lib, flow
    D, C = 5, 8
    net, z0 = _flow_and_start(name, D, C, 3)
    dev = z0.device
    like = gk.make_like(D, 100, 'logistic', 3)
    data = like.hip_like_glm
    good, keep = flow.glm_spec(data, dev)
    other, keep4 = flow.glm_spec(gk.make_like(4, 100, 'logistic', 3).hip_like_glm, dev)
    E_ARG = 1

    def spec(**kw):
        s = _lib.GlmSpec(good.at_dev, good.y_dev, good.o_dev, good.logl0, good.n, good.ld, good.D, good.family)
        for key, val in kw.items():
            setattr(s, key, val)
        return s

    def outs():
        f64 = dict(dtype=torch.float64, device=dev)
        return dict(z=torch.full((C, D), 123.0, device=dev), x=torch.full((C, D), 123.0, device=dev), lp=torch.full((C,), 123.0, **f64),
                    logl=torch.full((C,), 123.0, **f64), n_accept=torch.full((C,), -7, dtype=torch.int32, device=dev),
                    step=torch.full((C,), 123.0, **f64))

    bad_specs = [('glm is NULL', None), ('NULL at_dev', spec(at_dev=None)), ('NULL at_dev', spec(y_dev=None)), ('NULL at_dev', spec(o_dev=None)),
                 ('D=0', spec(D=0)), ('D=129', spec(D=129)), ('n=0', spec(n=0)), ('n=65537', spec(n=65537, ld=65600)),
                 ('ld=64', spec(ld=64)), ('ld=200', spec(ld=200)), ('ld=65600', spec(ld=65600)), ('family=2', spec(family=2)),
                 ('logl0=inf', spec(logl0=float('inf'))), ('logl0=nan', spec(logl0=float('nan')))]
    cases = [(what, dict(spec=s)) for what, s in bad_specs] + [
        ("the likelihood's D=4 is not the flow's x_dim=5", dict(spec=other)),
        ("the likelihood's power", dict(beta=-1.0)), ("the likelihood's power", dict(beta=float('nan'))), ('global_every=-1', dict(k=-1)),
        ('adapt_rate=', dict(rate=1.5)), ('target_accept=', dict(target=1.0)), ('steps=-1', dict(S=-1)), ('C=0', dict(C=0)),
        ('step_size', dict(step=float('nan'))), ('NULL device buffer', dict(null_x=True))]
    for what, kw in cases:
        o = outs()
        args = dict(spec=good, C=C, S=3)
        args.update(kw)
        rc = _raw_entry(net, args.pop('spec'), z0, o, args.pop('C'), args.pop('S'), **args)
        torch.cuda.synchronize()
        words = net._lib.nnest_hip_last_error().decode()
        assert rc == E_ARG and what in words, (what, rc, words)
        for key, t in o.items():
            assert bool((t == (-7 if key == 'n_accept' else 123.0)).all()), (what, key)
    # the call with nothing wrong runs
    o = outs()
    assert _raw_entry(net, good, z0, o, C, 3) == 0
    torch.cuda.synchronize()
    assert bool((o['logl'] <= like.logl0).all()) and bool((o['n_accept'] >= 0).all())
    # nnest_loglike_glm
    t = torch.zeros(4, D, device=dev)
    out = torch.full((4,), 123.0, dtype=torch.float64, device=dev)
    lib = _lib.load()
    st = _lib.current_stream(dev)
    for what, s in bad_specs:
        rc = lib.nnest_loglike_glm(None if s is None else ctypes.byref(s), _lib.ptr(t), _lib.ptr(out), 4, D, st)
        torch.cuda.synchronize()
        assert rc == E_ARG and what in lib.nnest_hip_last_error().decode() and bool((out == 123.0).all()), what
    for what, n, d in (("the likelihood's D=5 is not D=4", 4, D - 1), ('N=-1', -1, D)):
        rc = lib.nnest_loglike_glm(ctypes.byref(good), _lib.ptr(t), _lib.ptr(out), n, d, st)
        torch.cuda.synchronize()
        assert rc == E_ARG and what in lib.nnest_hip_last_error().decode() and bool((out == 123.0).all()), what
    assert lib.nnest_loglike_glm(ctypes.byref(good), None, None, 0, D, st) == 0
    # through the Python layer: the library's words in the exception, the binding's own for what never reaches the library
    kw = dict(t_std=None, t_mean=None)
    for words, bad in (('glm: n=0', dict(data, n=0)), ('glm: n=65537', dict(data, n=65537)), ('glm: ld=128', dict(data, n=129)),
                       ('glm: family=7', dict(data, family=7)), ('glm: logl0=', dict(data, logl0=float('nan')))):
        with pytest.raises(_lib.NnestHipError, match=words):
            net.mcmc_steps(None, z0, 2, 0.1, like_glm=bad, **kw)
        with pytest.raises(_lib.NnestHipError, match=words):
            flow.loglike_glm(bad, np.zeros((2, D), np.float32))
    with pytest.raises(_lib.NnestHipError, match="the likelihood's D=4 is not the flow's x_dim=5"):
        net.mcmc_steps(None, z0, 2, 0.1, like_glm=gk.make_like(4, 100, 'logistic', 3).hip_like_glm, **kw)
    with pytest.raises(_lib.NnestHipError, match="the likelihood's D=5 is not D=4"):
        flow.loglike_glm(data, np.zeros((2, 4), np.float32))
    with pytest.raises(_lib.NnestHipError, match="the likelihood's power"):
        net.mcmc_steps(None, z0, 2, 0.1, like_glm=data, beta=-1.0, **kw)
    with pytest.raises(ValueError, match='like_glm: family'):
        flow.loglike_glm(dict(data, family='probit'), np.zeros((2, D), np.float32))
    with pytest.raises(ValueError, match='like_glm: at must be shaped'):
        flow.loglike_glm(dict(data, y=data['y'][:100]), np.zeros((2, D), np.float32))
