"""GPU checks of the Gaussian likelihood from user data in the fused Metropolis runs (include/nnest_hip.h nnest_loglike_gdata,
nnest_mcmc_gdata_steps, nnest_spline_mcmc_gdata_steps; flow.loglike_gdata, HipNVP.mcmc_steps and HipSpline.mcmc_steps with like_data,
Sampler._device_target, MCMCSampler.run and SMCSampler.run on a likelihoods.GaussianData):
  1. the likelihood alone against float64, within the a-priori bound B of tests/gdata_check.py, and its bit-exact properties;
  2. both walk kernels replayed on their exported draws, step by step from the kernel's own previous row, as
     tests/test_gpu_mcmc_adapt.py replays the adaptive walk;
  3. a run cut into launches or into shards is the same run, bit for bit;
  4. walkers drawn exactly from the target stay exact;
  5. the front ends;
  6. the argument errors.

Targets: tests/gdata_check.make_target -- P = Q diag(lambda) Q^T, lambda in [0.5, 4], Q a random rotation, mu in +-0.3 --, logl0 = -3.25.

Tolerances of the replay.  logL at the kernel's own x (hist_x, with T applied as affine_on_device applies it) is held to float64
within B alone.  The flow's part -- lp - logL against the restated log-determinant, x against the restated inverse -- takes
tests/test_gpu_mcmc_mixed.py's tolerances for the flow and width: NVP x_dim <= 50 rtol 1e-6, atol 2e-5 on lp, 5e-5 on x; NVP x_dim
70 and 100 twice the error the test measures of nnest_ensemble_steps at that width (tests/test_gpu_mcmc_adapt.py
measured_tolerances, which doubles the measured figure); spline 3e-5 in |a - b| / (1 + |b|).  A decision is compared unless the
restated margin is within ten times the lp tolerance in force: the flow's, plus B, plus the sensitivity of logL to the x tolerance
(tests/gdata_check.sensitivity); at most 1 % of the 560 may be excluded.  Box, start scale and seed of each case were chosen on the
CPU (tools/mcmc_gdata_cases.py): the restatement alone leaves at most 0.25 % that close, local proposals fall outside the box, and
between 15 % and 85 % of the global proposals are accepted.

Measured on the MI355X: nnest_loglike_gdata uses at most 0.42 of B (x_dim 1) down to 0.0015 of B (x_dim 128); in the replays logL is at
most 0.22 (NVP) and 0.18 (spline) of B off float64, at most 1 of 560 decisions is excluded per case, lp - logL and x stay inside the
flows' tolerances; MCMCSampler's means are within 0.6 and its covariances within 2.7 standard errors; SMCSampler's log Z over 8 seeds
is within its bound for both flows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gdata_check as gc
from tests import mcmc_adapt_check as ac
from tests.slice_invariance import assert_invariant, stationarity_pvalues
from tests.test_gpu_mcmc_mixed import ENDS, HIST, SPL_TOL, TRAIN_EPOCHS, Restated as GaussRestated, _flow_and_start, affine, err, spline_and_start

pytestmark = pytest.mark.gpu

BOTH = ('n_accept', 'n_accept_global')
LOGL0 = gc.LOGL0


def _like(D, seed):
    from nnest_amd.likelihoods import GaussianData
    mu, P = gc.make_target(D, seed)
    return GaussianData(mu, precision=P, logl_max=LOGL0)


# ---- 1. the likelihood alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 2, 5, 31, 32, 33, 64, 70, 100, 128])
def test_loglike_gdata(D):
    from nnest_amd import flow
    data = _like(D, D).hip_like_data
    r = np.random.RandomState(D)
    N = 300
    t = (data['mu'] + r.normal(size=(N, D)) * r.uniform(0.1, 3.0, size=(N, 1))).astype(np.float32)
    t[0] = data['mu']
    t[1, D - 1] = np.nan
    t[2, 0] = np.inf
    got = flow.loglike_gdata(data, t).cpu().numpy()
    want, _, _ = gc.exact(data, t)
    B = gc.bound(data, t)
    fin = np.arange(N) >= 3
    worst = float(np.max(np.abs(got[fin] - want[fin]) / B[fin]))
    print('x_dim %d: |logL - float64| at most %.3g of the bound B (largest B %.3g, largest |logL| %.3g)' % (D, worst, B[fin].max(), np.abs(want[fin]).max()))
    assert np.all(np.abs(got[fin] - want[fin]) <= B[fin])
    assert np.all(got <= LOGL0)
    assert got[0] == LOGL0 and got[1] == -1e100 and got[2] == -1e100
    # the same rows in another position of another launch: the same bits
    back = flow.loglike_gdata(data, t[::-1].copy()).cpu().numpy()[::-1]
    assert np.array_equal(back.view(np.uint64), got.view(np.uint64))
    part = flow.loglike_gdata(data, t[7:18].copy()).cpu().numpy()
    assert np.array_equal(part.view(np.uint64), got[7:18].view(np.uint64))
    # the tiny case, by hand
    if D == 2:
        from nnest_amd.likelihoods import GaussianData
        tiny = GaussianData([0.1, -0.2], precision=[[2.0, 1.2], [1.2, 1.0]], logl_max=LOGL0)
        x = r.normal(size=(16, 2)).astype(np.float32)
        np.testing.assert_allclose(flow.loglike_gdata(tiny.hip_like_data, x).cpu().numpy(), tiny(x.astype(np.float64)), rtol=1e-6, atol=1e-6)


# ---- 2. the replay on the kernel's own draws ----------------------------------------------------------------------------------------
S_REPLAY, K_REPLAY, A_REPLAY, RATE, TARGET = 8, 3, 5, 1.0, 0.234
# (flow, x_dim, walker_offset): box, start scale, seed -- tools/mcmc_gdata_cases.py
REPLAY = {('nvp', 5, 0): (2.5, 0.5, 8005), ('nvp', 50, 1000): (3.0, 1.0, 8050), ('nvp', 70, 0): (3.0, 1.0, 8070),
          ('nvp', 100, 0): (3.0, 1.0, 8123), ('spline', 5, 0): (2.5, 0.5, 8005), ('spline', 40, 0): (2.5, 1.0, 8089)}


def check_gdata_replay(net, rs, z0, step, seed, offset, tol, x_tol, what):
    """tests/test_gpu_mcmc_adapt.py check_adapt_replay on this likelihood.  tol(v): the flow's lp tolerance at value v; x_tol(v): its x
    tolerance at |x| = v"""
    from nnest_amd import flow
    from nnest_amd.device_target import affine_on_device
    C, D = z0.shape
    S, k, A = S_REPLAY, K_REPLAY, A_REPLAY
    kw = dict(t_std=rs.sd, t_mean=rs.mu, lo=-np.full(D, rs.half), hi=np.full(D, rs.half), seed=seed, walker_offset=offset,
              like_data=rs.data)
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
        ll, B = gc.exact(rs.data, t)[0], gc.bound(rs.data, t)
        got = l_t.cpu().numpy()
        assert np.all(got <= LOGL0)
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


@pytest.mark.parametrize('D,offset', [(5, 0), (50, 1000), (70, 0), (100, 0)])
def test_nvp_kernel_replays_on_its_draws(D, offset):
    from oracle import oracle as orc
    from tests.test_gpu_mcmc_adapt import measured_tolerances
    C = 70
    half, scale, seed = REPLAY[('nvp', D, offset)]
    nvp, z0 = _flow_and_start('nvp', D, C, D, scale)
    sd, mu = affine(D, D)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    rs = gc.Restated(o, gc.replay_target(D), sd, mu, half)
    if D <= 50:
        tol, x_tol = (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    else:   # (the flow's error at this width, measured on the kernel that shares its evaluator, on its own likelihood)
        tol, x_tol, _ = measured_tolerances(nvp, GaussRestated(o, sd, mu, half), z0, sd, mu, half, seed, offset)
    check_gdata_replay(nvp, rs, z0, 1.0 / np.sqrt(D), seed, offset, tol, x_tol, 'nvp x_dim %d' % D)


@pytest.mark.parametrize('D', [5, 40])
def test_spline_kernel_replays_on_its_draws(D):
    C = 70
    half, scale, seed = REPLAY[('spline', D, 0)]
    sp, o, z0 = spline_and_start(D, C, D, scale)
    sd, mu = affine(D, D)
    rs = gc.Restated(o, gc.replay_target(D), sd, mu, half)
    t = lambda v: SPL_TOL * (1.0 + np.abs(v))
    check_gdata_replay(sp, rs, z0, 1.0 / np.sqrt(D), seed, 0, t, t, 'spline x_dim %d' % D)


# ---- 3. cuts and shards ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,D', [('nvp', 5), ('spline', 5), ('nvp', 70)])
def test_cuts_and_shards_are_bit_exact(name, D):
    C, k, A, half = 70, 3, 5, 3.0
    net, z0 = _flow_and_start(name, D, C, 8, 1.0)
    sd, mu = affine(D, 8)
    data = _like(D, 8).hip_like_data
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=42, like_data=data, global_every=k, adapt_steps=A)
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
    assert 0 < int(one['n_accept'].sum()) < 7 * C and bool((one['logl'] <= LOGL0).all())
    # a shard
    part = net.mcmc_steps(None, z0[24:].contiguous(), 7, step, walker_offset=24, **kw)
    for key in hist + ends + BOTH:
        assert torch.equal(part[key], one[key][24:]), key
    # the ends alone (no history) are the same run
    bare = net.mcmc_steps(None, z0, 7, step, history=False, **kw)
    assert bare['hist_z'] is None and bare['hist_step'] is None
    for key in ends + BOTH:
        assert torch.equal(bare[key], one[key]), key
    # the keys follow the arguments, as without like_data; steps = 0 evaluates the start
    base = dict(t_std=sd, t_mean=mu, lo=-np.full(D, half), hi=np.full(D, half), seed=42, like_data=data)
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
SD3 = np.array([1.0, 0.6, 0.4])
CORR3 = np.array([[1.0, 0.6, -0.4], [0.6, 1.0, 0.2], [-0.4, 0.2, 1.0]])   # unequal variances, correlations of both signs
MEAN3 = np.array([0.2, -0.1, 0.3])


def exact_draws(rng, n, cov, mean, half):
    """exact draws of N(mean, cov) in the box mean +- half, by Cholesky and rejection"""
    L = np.linalg.cholesky(cov)
    out, have = [], 0
    while have < n:
        x = mean + rng.normal(size=(2 * n, len(mean))) @ L.T
        x = x[np.all(np.abs(x - mean) <= half, axis=1)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


@pytest.mark.parametrize('name,beta', [('nvp', 1.0), ('nvp', 0.5), ('spline', 1.0), ('spline', 0.5)])
def test_exact_start_stays_exact(name, beta):
    from nnest_amd import flow
    from nnest_amd.likelihoods import GaussianData
    from nnest_amd.spline import HipSpline
    D, N, S = 3, 4096, 30
    cov = CORR3 * np.outer(SD3, SD3)
    assert np.all(np.linalg.eigvalsh(cov) > 0)
    like = GaussianData(MEAN3, cov=cov, logl_max=LOGL0)
    half = 4.0 * np.sqrt(np.diag(cov) / beta)                  # +-4 sigma of the tempered Gaussian N(mean, cov / beta)
    net = flow.HipNVP(D, 16, 3, 1, seed=21) if name == 'nvp' else HipSpline(D, 16, 3, seed=21)
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(61)
    tx0 = exact_draws(rng, N, cov / beta, MEAN3, half)
    z0, _ = net.forward(((tx0 - mu) / sd).astype(np.float32))   # (the spline's first forward sets the ActNorm layers from these points)
    res = net.mcmc_steps(None, z0.contiguous(), S, 0.5, t_std=sd, t_mean=mu, lo=MEAN3 - half, hi=MEAN3 + half, seed=5, beta=beta,
                         global_every=3, like_data=like.hip_like_data, history=False)
    moved = int(res['n_accept'].sum())
    assert 0.05 * N * S < moved < 0.95 * N * S and int(res['n_accept_global'].sum()) > 0
    tx = res['x'].cpu().numpy().astype(np.float64) * sd + mu
    unit = lambda x: (x - MEAN3) / half                        # the box as slice_invariance's unit box
    assert np.all(np.abs(unit(tx)) <= 1.0 + 1e-6)
    p = stationarity_pvalues(np.clip(unit(tx), -1.0, 1.0), unit(exact_draws(rng, N, cov / beta, MEAN3, half)))
    print('%s beta=%g: moved %.3f of the steps; smallest p-value %.3g of %d' % (name, beta, moved / float(N * S), min(p.values()), len(p)))
    assert_invariant(p, what='gdata walk, fused, %s beta=%g' % (name, beta))


# ---- 5. the front ends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_mcmc_front_end(tmp_path, flow_name):
    import nnest_amd
    from nnest_amd.likelihoods import GaussianData
    cov = CORR3 * np.outer(SD3, SD3)
    like = GaussianData(MEAN3, cov=cov, logl_max=LOGL0)
    rng = np.random.RandomState(3)
    N, S, A = 64, 600, 100
    train = MEAN3 + rng.normal(size=(2000, 3)) @ np.linalg.cholesky(cov).T
    init = (train[:N] - train.mean(0)) / train.std(0)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(3, like, log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.run(S, N, train, init_samples=init, route='fused', seed=1, adapt_steps=A, global_every=5)
    assert s.mcmc_route == 'fused'
    assert s.samples.shape == (N, S + 1, 3) and s.step_sizes.shape == (N,) and s.global_proposed == N * (S // 5)
    np.testing.assert_allclose(s.loglikes.reshape(-1), like(s.samples.reshape(-1, 3)), rtol=1e-5, atol=1e-4)
    # every component of the mean and of the covariance within five standard errors of the truth; the standard error is the spread
    # of the per-chain estimates over the independent chains / sqrt(chains), the adapting steps discarded.  (The per-chain second
    # moments are taken about the TRUE mean: about the chain's own they would be biased low by its autocorrelation.)
    x = s.samples[:, A + 1:, :].astype(np.float64)
    m = x.mean(1)
    d = x - MEAN3
    c = np.einsum('nti,ntj->nij', d, d) / x.shape[1]
    for est, truth, what in ((m, MEAN3, 'mean'), (c, cov, 'covariance')):
        se = est.std(0, ddof=1) / np.sqrt(N)
        off = np.abs(est.mean(0) - truth) / se
        print('%s: %s off by at most %.2f standard errors (largest standard error %.3g)' % (flow_name, what, off.max(), se.max()))
        assert np.all(off <= 5.0), (what, off)
    # the routes this likelihood has no kernel for answer as they did
    with pytest.raises(ValueError, match='importance_evidence: the fused route does not take a likelihood the kernels do not know'):
        s.importance_evidence(64, route='fused')


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_smc_front_end(tmp_path, flow_name):
    """log Z of a 2-D Gaussian likelihood under a uniform prior that holds +-8 sigma: logl0 + log 2 pi - 1/2 log det P - log(volume)
    (the mass outside +-8 sigma is below 1e-14).  Over 8 seeds the mean of log Z^ is within five standard errors of that, plus half
    the sample variance: the Jensen bias of the logarithm of an unbiased Z^.  The sampler runs as it comes (adapt_fraction = 0,
    global_every = 0: the tempered walk at a fixed step, which keeps every stage's target and so Z^ unbiased); with the step adapted
    over half of a stage's ten moves log Z^ comes out low by 0.1 to 0.25 -- with these kernels and, on the same Gaussian as
    NNEST_LIKE_GAUSSIAN, with the adaptive kernels alike, seed for seed --, so that setting is held to the route and to 1 only."""
    import nnest_amd
    from nnest_amd.likelihoods import GaussianData
    from nnest_amd.priors import UniformPrior
    mean = np.array([0.3, -0.2])
    P = np.array([[2.0, 1.2], [1.2, 1.0]])
    like = GaussianData(mean, precision=P, logl_max=LOGL0)
    sig = np.sqrt(np.diag(np.linalg.inv(P)))
    lo, hi = float((mean - 8 * sig).min()), float((mean + 8 * sig).max())
    exact = LOGL0 + np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(P)[1] - 2 * np.log(hi - lo)
    s = nnest_amd.SMCSampler(2, like, prior=UniformPrior(2, lo, hi), log_dir=str(tmp_path), log_level=30, flow=flow_name)
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
    print('%s: log Z %.4f +- %.4f over 8 seeds (exact %.4f, sample variance %.4f); %d stages' % (flow_name, mean_z, se, exact, var, len(s.betas)))
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
    from nnest_amd.likelihoods import GaussianData
    cov = CORR3 * np.outer(SD3, SD3)
    like = GaussianData(MEAN3, cov=cov, logl_max=LOGL0)
    train = MEAN3 + np.random.RandomState(3).normal(size=(500, 3)) @ np.linalg.cholesky(cov).T
    e = nnest_amd.EnsembleSampler(3, like, log_dir=str(tmp_path), log_level=30, flow='nvp')
    e.trainer.train = lambda samples, **kw: None
    with pytest.raises(ValueError, match='ensemble: the fused route does not take this flow, likelihood, population or move'):
        e.run(4, 16, train, route='fused')
    # a descriptor that does not describe the host callable is refused with a warning, not run
    bad = GaussianData(MEAN3, cov=cov, logl_max=LOGL0)
    bad.hip_like_data['mu'] = bad.hip_like_data['mu'] + np.float32(0.5)
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
    assert any(level == logging.WARNING and 'hip_like_data disagrees with the host callable' in line for level, line in seen), seen
    # a descriptor of another dimension than the flow's: the library's words
    net = s.trainer.netG
    assert net.mcmc_gdata_refusal() is None and net.mcmc_gdata_refusal(3) is None
    assert "the likelihood's D=4 is not the flow's x_dim=3" in net.mcmc_gdata_refusal(4)


# ---- 6. the argument errors -----------------------------------------------------------------------------------------------------------
def _raw_entry(net, spec, z0, outs, C, S, beta=1.0, k=0, rate=1.0, target=0.234, step=0.1, null_x=False):
    from nnest_amd import _lib
    dev = z0.device
    with torch.cuda.device(dev):
        return net._sym['mcmc_gdata'](
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
    data = _like(D, 3).hip_like_data
    good, keep = flow.gdata_spec(data, dev)
    other, keep4 = flow.gdata_spec(_like(4, 3).hip_like_data, dev)
    E_ARG = 1

    def spec(**kw):
        s = _lib.GdataSpec(good.mu_dev, good.r_dev, good.logl0, good.D)
        for key, val in kw.items():
            setattr(s, key, val)
        return s

    def outs():
        f64 = dict(dtype=torch.float64, device=dev)
        return dict(z=torch.full((C, D), 123.0, device=dev), x=torch.full((C, D), 123.0, device=dev), lp=torch.full((C,), 123.0, **f64),
                    logl=torch.full((C,), 123.0, **f64), n_accept=torch.full((C,), -7, dtype=torch.int32, device=dev),
                    step=torch.full((C,), 123.0, **f64))

    cases = [('gdata NULL', dict(spec=None)), ('mu_dev NULL', dict(spec=spec(mu_dev=None))), ('r_dev NULL', dict(spec=spec(r_dev=None))),
             ('D of another flow', dict(spec=other)), ('D = 0', dict(spec=spec(D=0))), ('D = 129', dict(spec=spec(D=129))),
             ('logl0 inf', dict(spec=spec(logl0=float('inf')))), ('logl0 nan', dict(spec=spec(logl0=float('nan')))),
             ('beta < 0', dict(beta=-1.0)), ('beta nan', dict(beta=float('nan'))), ('global_every < 0', dict(k=-1)),
             ('adapt_rate > 1', dict(rate=1.5)), ('target_accept = 1', dict(target=1.0)), ('steps < 0', dict(S=-1)), ('C = 0', dict(C=0)),
             ('step_size nan', dict(step=float('nan'))), ('x_out NULL', dict(null_x=True))]
    for what, kw in cases:
        o = outs()
        args = dict(spec=good, C=C, S=3)
        args.update(kw)
        rc = _raw_entry(net, args.pop('spec'), z0, o, args.pop('C'), args.pop('S'), **args)
        torch.cuda.synchronize()
        assert rc == E_ARG, (what, rc, net._lib.nnest_hip_last_error())
        for key, t in o.items():
            assert bool((t == (-7 if key == 'n_accept' else 123.0)).all()), (what, key)
    # the call with nothing wrong runs
    o = outs()
    assert _raw_entry(net, good, z0, o, C, 3) == 0
    torch.cuda.synchronize()
    assert bool((o['logl'] <= LOGL0).all()) and bool((o['n_accept'] >= 0).all())
    # nnest_loglike_gdata
    t = torch.zeros(4, D, device=dev)
    out = torch.full((4,), 123.0, dtype=torch.float64, device=dev)
    lib = _lib.load()
    st = _lib.current_stream(dev)
    for what, s, n, d in (('gdata NULL', None, 4, D), ('mu_dev NULL', spec(mu_dev=None), 4, D), ('r_dev NULL', spec(r_dev=None), 4, D),
                          ('D differs', good, 4, D - 1), ('logl0 nan', spec(logl0=float('nan')), 4, D), ('N < 0', good, -1, D)):
        rc = lib.nnest_loglike_gdata(None if s is None else ctypes.byref(s), _lib.ptr(t), _lib.ptr(out), n, d, st)
        torch.cuda.synchronize()
        assert rc == E_ARG and bool((out == 123.0).all()), what
    assert lib.nnest_loglike_gdata(ctypes.byref(good), None, None, 0, D, st) == 0
    with pytest.raises(ValueError, match='like_data'):
        flow.loglike_gdata(dict(mu=data['mu'], R=data['R'][:4], logl0=0.0), np.zeros((2, D), np.float32))
