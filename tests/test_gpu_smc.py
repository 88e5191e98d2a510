"""GPU checks of the sequential Monte Carlo sampler (include/nnest_hip.h nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps,
nnest_smc_reweight, nnest_smc_resample; HipNVP / HipSpline.mcmc_steps(beta=...), flow.smc_reweight, flow.smc_resample,
nnest_amd.SMCSampler): the tempered kernels against the numpy restatement on their own draws (tests/test_gpu_mcmc_walk.check_replay
with the restated target carrying beta); beta = 1.0 is the untempered entry bit for bit; the invariances of the untempered run at
beta = 0.3; the refusals of beta; the reweighting and the resampling against tests/smc_check.py; the sampler end to end on targets
with a known evidence, on both routes.

Tolerances of the replay: tests/test_gpu_mcmc_walk.py's own.  lp_beta's error is at most beta * err(logL) + err(log|det|), which for
beta <= 1 is within the untempered bound; above x_dim 50 the bound is twice the ensemble kernel's measured error, obtained as that file
obtains it.  The same cap holds: at most 1 % of the decisions excluded as borderline."""
import ctypes

import numpy as np
import pytest
import torch

from tests import smc_check as sc
from tests.test_gpu_mcmc_walk import (BOX, CORR, ENDS, GAUSS, HIST, SPL_TOL, SPLINE_SEEDS, Restated, _flow_and_start, affine, check_replay, err,
                                      in_box, spline_and_start)

pytestmark = pytest.mark.gpu


class TemperedRestated(Restated):
    """tests/test_gpu_mcmc_walk.Restated with the likelihood to the power beta in lp"""

    def __init__(self, o, sd, mu, half, beta):
        super(TemperedRestated, self).__init__(o, sd, mu, half)
        self.lp = sc.tempered_target(self.x_of_z, self.logl, lambda x: in_box(self.T(x), half), beta)


class Tempered(object):
    """a flow whose mcmc_steps runs the tempered entry at beta: what check_replay drives"""

    def __init__(self, net, beta):
        self.net, self.beta = net, beta

    def mcmc_steps(self, *a, **kw):
        return self.net.mcmc_steps(*a, beta=self.beta, **kw)


@pytest.mark.parametrize('beta', [0.0, 0.3])
@pytest.mark.parametrize('D,offset', [(5, 0), (50, 1000), (70, 0), (100, 0)])
def test_nvp_tempered_kernel_replays_on_its_draws(D, offset, beta):
    from nnest_amd import flow
    from oracle import oracle as orc
    C, S, seed = 70, 6, 4000 + D
    nvp = flow.HipNVP(D, 16, 3, 1, seed=D)
    sd, mu = affine(D, D)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    rs = TemperedRestated(o, sd, mu, BOX, beta)
    z0 = torch.from_numpy(np.random.RandomState(D).normal(size=(C, D)).astype(np.float32) * 0.5).cuda()
    if D <= 50:
        tol, x_tol = (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    else:
        # the evaluator's error in the existing ensemble kernel at this width, against the untempered restatement: twice that is allowed
        plain = Restated(o, sd, mu, BOX)
        ens = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=seed, like_params=(CORR,))
        ez, ex = (ens[k].cpu().numpy().reshape(C * S, D) for k in ('hist_z', 'hist_x'))
        elp = ens['hist_lp'].cpu().numpy().reshape(C * S)
        e_lp = err(elp, plain.lp(ez), lambda v: 0.0 * v)
        e_x = float(np.max(np.abs(ex - plain.x_of_z(ez)[0])))
        print('x_dim %d: nnest_ensemble_steps against the restatement: lp %.3g, x %.3g' % (D, e_lp, e_x))
        assert e_lp > 0.0 and e_x > 0.0
        tol, x_tol = (lambda v: 2.0 * e_lp + 0.0 * v), (lambda v: 2.0 * e_x + 0.0 * v)
    check_replay(Tempered(nvp, beta), rs, z0, S, 1.0 / np.sqrt(D), seed, offset, tol, x_tol, 'nvp x_dim %d beta %g' % (D, beta))


# (the seeds, chosen as tests/test_gpu_mcmc_walk.py chose SPLINE_SEEDS, for each target: on the CPU, the first of 5000 + x_dim, ...
# for which the restatement alone -- mcmc_walk_check.mcmc_draws and rw_step through the oracle's spline on the same initialisation, with
# smc_check.tempered_target -- has no decision within 3 m.  The untempered target's seed does not serve at x_dim 40: at beta = 0.3
# the restatement alone has decisions within 0.14 m (seed 5040) .. 0.5 m there, and the kernel run with 5050 excluded 4 of 160)
TEMPERED_SPLINE_SEEDS = {(5, 0.0): SPLINE_SEEDS[5], (5, 0.3): SPLINE_SEEDS[5], (40, 0.0): 5041, (40, 0.3): 5052}


@pytest.mark.parametrize('beta', [0.0, 0.3])
@pytest.mark.parametrize('D', [5, 40])
def test_spline_tempered_kernel_replays_on_its_draws(D, beta):
    C, S, seed = 40, 4, TEMPERED_SPLINE_SEEDS[(D, beta)]
    sp, o, z0 = spline_and_start(D, C, D)
    sd, mu = affine(D, D)
    rs = TemperedRestated(o, sd, mu, BOX, beta)
    check_replay(Tempered(sp, beta), rs, z0, S, 1.0 / np.sqrt(D), seed, 0, lambda v: SPL_TOL * (1.0 + np.abs(v)),
                 lambda v: SPL_TOL * (1.0 + np.abs(v)), 'spline x_dim %d beta %g' % (D, beta))


def _kw(D, seed, params=(CORR,)):
    sd, mu = affine(D, seed)
    return dict(t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=40 + seed, like_params=params)


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_beta_zero_moves_as_the_prior_and_the_jacobian_say(name):
    """two likelihood parameter sets: logL differs in every row, and at beta = 0 nothing else does -- bit for bit"""
    D, C, S = 20, 70, 6
    net, z0 = _flow_and_start(name, D, C, 11)
    a = net.mcmc_steps(GAUSS, z0, S, 0.2, beta=0.0, **_kw(D, 11, (CORR,)))
    b = net.mcmc_steps(GAUSS, z0, S, 0.2, beta=0.0, **_kw(D, 11, (0.2,)))
    for key in ('hist_z', 'hist_x', 'z', 'x', 'lp', 'n_accept'):
        assert torch.equal(a[key], b[key]), key
    assert bool((a['hist_logl'] != b['hist_logl']).all()) and bool((a['logl'] != b['logl']).all())
    assert 0 < int(a['n_accept'].sum()) < C * S
    # lp at beta = 0 is the Jacobian in the box and -inf outside: no likelihood in it
    fin = torch.isfinite(a['lp'])
    c = net.mcmc_steps(GAUSS, z0, S, 0.2, beta=0.3, **_kw(D, 11, (CORR,)))
    assert not torch.equal(a['hist_z'], c['hist_z'])
    assert bool(fin.any()) and bool((a['lp'][fin].abs() < 1e3).all())


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_beta_one_is_the_untempered_entry_bit_for_bit(name):
    for D, C, S in ((20, 70, 7), (70 if name == 'nvp' else 40, 21, 4)):   # (the NVP's weights in registers and in LDS)
        net, z0 = _flow_and_start(name, D, C, 12)
        kw = _kw(D, 12)
        old = net.mcmc_steps(GAUSS, z0, S, 0.2, **kw)
        new = net.mcmc_steps(GAUSS, z0, S, 0.2, beta=1.0, **kw)
        for key in HIST + ENDS + ('n_accept',):
            assert torch.equal(old[key], new[key]), (D, key)
        assert 0 < int(old['n_accept'].sum()) < C * S
        old0, new0 = net.mcmc_steps(GAUSS, z0, 0, 0.2, **kw), net.mcmc_steps(GAUSS, z0, 0, 0.2, beta=1.0, **kw)
        for key in ('x', 'lp', 'logl'):
            assert torch.equal(old0[key], new0[key]), (D, key)


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_invariances_at_beta_0_3(name):
    from nnest_amd import _lib
    D, C, beta = 20, 70, 0.3
    net, z0 = _flow_and_start(name, D, C, 8)
    kw = dict(beta=beta, **_kw(D, 8))
    # a run cut into launches
    one = net.mcmc_steps(GAUSS, z0, 7, 0.2, **kw)
    a = net.mcmc_steps(GAUSS, z0, 3, 0.2, **kw)
    b = net.mcmc_steps(GAUSS, a['z'], 4, 0.2, lp=a['lp'], logl=a['logl'], step0=3, **kw)
    for key in HIST:
        assert torch.equal(torch.cat([a[key], b[key]], 1), one[key]), key
    for key in ENDS:
        assert torch.equal(b[key], one[key]), key
    assert torch.equal(a['n_accept'] + b['n_accept'], one['n_accept']) and 0 < int(one['n_accept'].sum()) < 7 * C
    # a shard
    part = net.mcmc_steps(GAUSS, z0[24:].contiguous(), 7, 0.2, walker_offset=24, **kw)
    for key in HIST + ENDS + ('n_accept',):
        assert torch.equal(part[key], one[key][24:]), key
    # steps = 0 writes x, lp and logL only, and they are the start of the run: lp is lp_beta, logL is untempered
    dev = z0.device
    z_out = torch.full((C, D), 123.0, device=dev)
    n_acc = torch.full((C,), -7, dtype=torch.int32, device=dev)
    x_out = torch.empty(C, D, device=dev)
    lp_out, ll_out = torch.empty(C, dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)
    lk = _lib.like_spec(GAUSS, 1.0, (CORR,))
    vec = lambda v: torch.as_tensor(np.asarray(v, np.float32)).to(dev)
    t_std, t_mean, lo, hi = vec(kw['t_std']), vec(kw['t_mean']), vec(kw['lo']), vec(kw['hi'])
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc_tempered'](net._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(z0),
                                             None, None, _lib.ptr(z_out), _lib.ptr(x_out), _lib.ptr(lp_out), _lib.ptr(ll_out), None, None, None,
                                             _lib.ptr(n_acc), C, 0, ctypes.c_float(0.2), 0, kw['seed'], 0, ctypes.c_double(beta),
                                             _lib.current_stream(dev)))
    torch.cuda.synchronize()
    assert bool((z_out == 123.0).all()) and bool((n_acc == -7).all())
    zero = net.mcmc_steps(GAUSS, z0, 0, 0.2, **kw)
    plain = net.mcmc_steps(GAUSS, z0, 0, 0.2, **_kw(D, 8))
    assert torch.equal(zero['x'], x_out) and torch.equal(zero['lp'], lp_out) and torch.equal(zero['logl'], ll_out)
    assert torch.equal(zero['logl'], plain['logl']) and torch.equal(zero['x'], plain['x'])
    fin = torch.isfinite(plain['lp'])
    assert bool(fin.any()) and torch.equal(torch.isfinite(zero['lp']), fin)
    # lp_beta = lp - (1 - beta) logL, to the rounding of three float64 operations on |lp| < 1e3
    want = plain['lp'][fin] - (1.0 - beta) * plain['logl'][fin]
    assert float((zero['lp'][fin] - want).abs().max()) < 1e-11


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_c_entry_refuses_beta_and_leaves_the_outputs(name):
    from nnest_amd import _lib
    D, C, S = 6, 21, 3
    net, z0 = _flow_and_start(name, D, C, 10)
    dev = z0.device
    f32 = lambda *shape: torch.full(shape, 123.0, device=dev)
    f64 = lambda *shape: torch.full(shape, 321.0, dtype=torch.float64, device=dev)
    outs = dict(z=f32(C, D), x=f32(C, D), lp=f64(C), logl=f64(C), hz=f32(C, S, D), hx=f32(C, S, D), hl=f64(C, S))
    n_acc = torch.full((C,), -7, dtype=torch.int32, device=dev)
    lk = _lib.like_spec(GAUSS, 1.0, (CORR,))

    def call(beta):
        with torch.cuda.device(dev):
            return net._sym['mcmc_tempered'](net._h, ctypes.byref(lk), None, None, None, None, _lib.ptr(z0), None, None, _lib.ptr(outs['z']),
                                             _lib.ptr(outs['x']), _lib.ptr(outs['lp']), _lib.ptr(outs['logl']), _lib.ptr(outs['hz']),
                                             _lib.ptr(outs['hx']), _lib.ptr(outs['hl']), _lib.ptr(n_acc), C, S, ctypes.c_float(0.3), 0, 0, 0,
                                             ctypes.c_double(beta), _lib.current_stream(dev))

    for beta in (float('nan'), -1.0, float('inf'), -float('inf')):
        assert call(beta) == 1 and b'beta' in net._lib.nnest_hip_last_error(), beta
        with pytest.raises(_lib.NnestHipError, match='beta'):
            net.mcmc_steps(GAUSS, z0, S, 0.3, beta=beta, like_params=(CORR,))
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == (123.0 if t.dtype == torch.float32 else 321.0)).all()), k
    assert bool((n_acc == -7).all())
    assert call(0.0) == 0   # (beta = 0 is valid)
    torch.cuda.synchronize()
    assert not bool((outs['x'] == 123.0).any()) and not bool((n_acc == -7).any())


# ---- reweight and resample ----------------------------------------------------------------------------------------------------
def heavy_logl(rng, N, dead):
    """a Rosenbrock-like heavy-tailed log-likelihood sample with `dead` entries at the safe value -1e100"""
    x = rng.uniform(-5, 5, size=(N, 2))
    logl = -(100.0 * (x[:, 1] - x[:, 0] ** 2) ** 2 + (1.0 - x[:, 0]) ** 2)
    if dead:
        logl[rng.choice(N, size=dead, replace=False)] = -1e100
    return logl


REWEIGHT_N = (1, 3, 64, 1000, 4099)


@pytest.mark.parametrize('frac', [0.5, 0.9])
def test_reweight(frac):
    """(the dead entries stay below (1 - ess_fraction) N: above that the ESS cannot reach its target at any beta' > beta and the
    rule's answer, one bracket above beta, is right but not on the target)"""
    from nnest_amd import flow
    rng = np.random.RandomState(17)
    for N in REWEIGHT_N:
        for beta in (0.0, 0.003):
            logl = heavy_logl(rng, N, N // 50)
            dev_logl = torch.from_numpy(logl).cuda()
            out, m = flow.smc_reweight(dev_logl, beta, frac)
            out2, m2 = flow.smc_reweight(dev_logl, beta, frac)
            assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(m, m2)   # the same bits twice
            b, inc, ess, mx = (float(v) for v in out.cpu().numpy())
            m = m.cpu().numpy()
            (rb, rinc, ress, rmx), _ = sc.reweight(logl, beta, frac)
            target = frac * N
            ess_np = sc.ess_of(sc.weights(logl, beta, b))
            print('N %d beta %g frac %g: beta\' %.17g (restated %.17g), ESS %.9g of target %.9g, increment %.17g (restated %.17g)'
                  % (N, beta, frac, b, rb, ess_np, target, inc, rinc))
            assert mx == rmx == logl.max()
            assert beta < b <= 1.0 and abs(b - rb) <= 1e-9
            assert abs(ess_np - target) <= 1e-6 * N or (b == 1.0 and ess_np >= target)
            assert ess == pytest.approx(ess_np, rel=1e-12)
            assert inc == pytest.approx(sc.increment(logl, beta, b), rel=1e-12)   # (the restated increment at the kernel's beta')
            want = sc.integer_weights(logl, beta, b)
            assert m.dtype == np.int64 and np.all(np.abs(m - want) <= 1) and m.max() == 2 ** 31 and np.all(m[logl == -1e100] == 0)
    # an easy population goes to 1 at once
    out, m = flow.smc_reweight(torch.from_numpy(rng.normal(size=500) * 0.01).cuda(), 0.4, frac)
    assert float(out[0]) == 1.0 and float(out[2]) >= frac * 500
    with pytest.raises(Exception, match='beta'):
        flow.smc_reweight(dev_logl, 1.0, frac)


@pytest.mark.parametrize('D', [1, 5, 50])
def test_resample(D):
    from nnest_amd import _lib, flow
    lib = _lib.load()
    rng = np.random.RandomState(23 + D)
    for N in (1, 3, 1000, 4099):
        logl = heavy_logl(rng, N, N // 50)
        theta = rng.normal(size=(N, D)).astype(np.float32)
        dev_logl = torch.from_numpy(logl).cuda()
        _, m = flow.smc_reweight(dev_logl, 0.0, 0.5)
        seed, stage = (7 << 33) + N, 3 + D
        anc, th, ll = flow.smc_resample(m, torch.from_numpy(theta).cuda(), dev_logl, seed, stage)
        want = sc.systematic(m.cpu().numpy(), sc.smc_uniform(seed, stage))
        np.testing.assert_array_equal(anc.cpu().numpy(), want)
        assert anc.dtype == torch.int32
        assert np.array_equal(th.cpu().numpy().view(np.uint32), theta[want].view(np.uint32))
        assert np.array_equal(ll.cpu().numpy().view(np.uint64), logl[want].view(np.uint64))
        if N > 3:
            assert len(np.unique(want)) < N   # (something was resampled)
        # through the C entry with longer buffers: the rows past N keep their guard pattern
        dev = m.device
        anc_g = torch.full((N + 3,), -9, dtype=torch.int32, device=dev)
        th_g = torch.full((N + 3, D), 123.0, device=dev)
        ll_g = torch.full((N + 3,), 321.0, dtype=torch.float64, device=dev)
        th_in = torch.from_numpy(theta).cuda()
        with torch.cuda.device(dev):
            _lib.check(lib.nnest_smc_resample(_lib.ptr(m), N, D, seed, stage, _lib.ptr(th_in), _lib.ptr(dev_logl), _lib.ptr(anc_g), _lib.ptr(th_g),
                                              _lib.ptr(ll_g), _lib.current_stream(dev)))
        assert torch.equal(anc_g[:N], anc) and torch.equal(th_g[:N], th) and torch.equal(ll_g[:N], ll)
        assert bool((anc_g[N:] == -9).all()) and bool((th_g[N:] == 123.0).all()) and bool((ll_g[N:] == 321.0).all())
    # weights that sum to 0 are refused, the outputs unwritten
    th_g.fill_(123.0)
    ll_g.fill_(321.0)
    none = torch.zeros_like(m)
    with torch.cuda.device(dev):
        rc = lib.nnest_smc_resample(_lib.ptr(none), N, D, seed, stage, _lib.ptr(th_in), _lib.ptr(dev_logl), _lib.ptr(anc_g),
                                    _lib.ptr(th_g), _lib.ptr(ll_g), _lib.current_stream(dev))
    assert rc == 1 and b'sum to 0' in lib.nnest_hip_last_error()
    assert bool((th_g == 123.0).all()) and bool((ll_g == 321.0).all())


def test_resample_the_largest_population():
    """N = 2^20 weights near 2^31: the prefix sums reach 2^51, every chunk of the scan is full"""
    from nnest_amd import flow
    N = 1 << 20
    logl = np.random.RandomState(5).normal(size=N) * 0.5
    dev_logl = torch.from_numpy(logl).cuda()
    out, m = flow.smc_reweight(dev_logl, 0.0, 0.5)
    assert float(out[0]) == 1.0
    assert float(out[1]) == pytest.approx(sc.increment(logl, 0.0, 1.0), rel=1e-12)
    theta = torch.arange(N, dtype=torch.float32, device='cuda').reshape(N, 1)
    anc, th, ll = flow.smc_resample(m, theta, dev_logl, 9, 0)
    want = sc.systematic(m.cpu().numpy(), sc.smc_uniform(9, 0))
    np.testing.assert_array_equal(anc.cpu().numpy(), want)
    assert torch.equal(th[:, 0], anc.float()) and np.array_equal(ll.cpu().numpy(), logl[want])


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
TRAIN_EPOCHS = 30   # the cap on every retraining in these tests (Trainer.train's own `max_iters`)


def _sampler(tmp_path, D, like, prior, flow_name):
    import nnest_amd
    s = nnest_amd.SMCSampler(D, like, prior=prior, log_dir=str(tmp_path), log_level=30, flow=flow_name)
    train = s.trainer.train
    s.trainer.train = lambda samples, **kw: train(samples, max_iters=TRAIN_EPOCHS, **kw)
    return s


def _runs(s, seeds, **kw):
    out = []
    for seed in seeds:
        np.random.seed(seed)
        torch.manual_seed(seed)
        s.run(seed=seed, **kw)
        assert s.betas[-1] == 1.0 and np.all(np.diff([0.0] + s.betas) > 0)
        assert all(0.0 < a < 1.0 for a in s.acceptance), s.acceptance
        assert sum(s.logz_steps) == pytest.approx(s.logz, rel=1e-12)
        out.append((s.logz, s.samples.copy(), len(s.betas)))
    return out


def _mean_se(v):
    v = np.asarray(v, np.float64)
    return float(v.mean()), float(v.std(ddof=1) / np.sqrt(len(v)))


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_end_to_end_fused_gaussian(tmp_path, flow_name):
    """Gaussian(4, 0.5) in a +-6 box, N = 512, 10 steps a stage, 8 seeds: the mean log Z within 4 standard errors of -4 log 12 = -9.9396.
    (With the flow trained on the resampled population, copies included, the spline flow's mean was -10.31 +- 0.04 here: the sampler
    trains on the distinct particles -- SMCSampler._smc_train has the reason.)"""
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    like = Gaussian(4, 0.5)
    s = _sampler(tmp_path, 4, like, UniformPrior(4, -6.0, 6.0), flow_name)
    runs = _runs(s, range(8), num_particles=512, mcmc_steps=10)
    assert s.smc_route == 'fused'
    mean, se = _mean_se([r[0] for r in runs])
    print('%s: log Z %.4f +- %.4f over 8 seeds (exact %.4f); stages %s' % (flow_name, mean, se, -4 * np.log(12.0), [r[2] for r in runs]))
    assert abs(mean + 4.0 * np.log(12.0)) <= 4.0 * se
    K = runs[-1][2]
    assert s.samples.shape == (512, 4) and s.loglikes.shape == (512,) and s.latent_samples.shape == (512, 4)
    assert len(s.ess) == len(s.acceptance) == len(s.logz_steps) == K
    np.testing.assert_allclose(s.loglikes, like(s.samples), rtol=1e-5, atol=1e-4)
    assert np.all(np.abs(s.samples) <= 6.0)
    # the posterior at beta = 1: N(0, Sigma), pooled over the seeds
    pooled = np.concatenate([r[1] for r in runs])
    c = np.cov(pooled.T)
    assert np.all(np.abs(pooled.mean(0)) < 0.2) and np.all(np.abs(np.diag(c) - 1.0) < 0.25) and np.all(np.abs(c[np.triu_indices(4, 1)] - 0.5) < 0.25)


def test_modes(tmp_path):
    from nnest_amd.likelihoods import GaussianMix
    from nnest_amd.priors import UniformPrior
    s = _sampler(tmp_path, 2, GaussianMix(2), UniformPrior(2, -10.0, 10.0), 'spline')
    runs = _runs(s, range(6), num_particles=2048, mcmc_steps=10)
    assert s.smc_route == 'fused'
    mean, se = _mean_se([r[0] for r in runs])
    pooled = np.concatenate([r[1] for r in runs])
    centres = np.array([[0.0, 4.0], [0.0, -4.0], [4.0, 0.0], [-4.0, 0.0]])
    nearest = np.argmin(((pooled[:, None, :] - centres[None]) ** 2).sum(-1), axis=1)
    shares = np.bincount(nearest, minlength=4) / float(len(pooled))
    want = np.array([0.4, 0.3, 0.2, 0.1])
    bse = np.sqrt(want * (1.0 - want) / len(pooled))
    print('modes: log Z %.4f +- %.4f over 6 seeds (exact %.4f); shares %s (in binomial standard errors: %s); stages %s'
          % (mean, se, -2 * np.log(20.0), shares, (shares - want) / bse, [r[2] for r in runs]))
    assert abs(mean + 2.0 * np.log(20.0)) <= 4.0 * se
    assert np.all(np.abs(shares - want) <= 4.0 * bse)


def test_host_route_agrees_with_the_fused_route(tmp_path):
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    like = Gaussian(3, 0.5)
    python_like = lambda x: like(x)   # (no hip_like_id: a likelihood the kernels do not know)
    host = _sampler(tmp_path, 3, python_like, UniformPrior(3, -6.0, 6.0), 'nvp')
    with pytest.raises(ValueError, match='Python callable'):
        host.run(num_particles=512, mcmc_steps=10, route='fused')
    hruns = _runs(host, range(4), num_particles=512, mcmc_steps=10)
    assert host.smc_route == 'host'
    assert host.total_calls == sum(512 + r[2] * 512 * 11 for r in hruns)
    fused = _sampler(tmp_path, 3, like, UniformPrior(3, -6.0, 6.0), 'nvp')
    fruns = _runs(fused, range(4), num_particles=512, mcmc_steps=10)
    assert fused.smc_route == 'fused'
    assert fused.total_calls == sum(512 + r[2] * 512 * 11 for r in fruns)
    (hm, hse), (fm, fse) = _mean_se([r[0] for r in hruns]), _mean_se([r[0] for r in fruns])
    print('host log Z %.4f +- %.4f, fused %.4f +- %.4f (exact %.4f)' % (hm, hse, fm, fse, -3 * np.log(12.0)))
    assert abs(hm - fm) <= 4.0 * np.hypot(hse, fse)
    np.testing.assert_allclose(host.loglikes, like(host.samples), rtol=1e-5, atol=1e-4)
