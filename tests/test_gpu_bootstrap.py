"""GPU checks of EnsembleSampler.bootstrap's pieces: the fused x-space stretch-move kernel (nnest_ensemble_x_steps) against the numpy
restatement on its exported draws and against the round driver on an identity flow (the only x-space route before the kernel),
chunking, invariance of an exactly sampled target, the residency refusal, emcee's integrated autocorrelation time
(nnest_chain_autocorr) against the float64 restatement, and the front end on both routes."""
import numpy as np
import pytest
import torch

from tests import bootstrap_check as bc
from tests.ensemble_check import borderline_prefix, latent_target, stretch_step
from tests.slice_invariance import assert_invariant, stationarity_pvalues

pytestmark = pytest.mark.gpu

GAUSS = 3   # NNEST_LIKE_GAUSSIAN: N(0, Sigma), Sigma = I + corr (11^T - I)
CORR = 0.5


def affine(D, seed):
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)


def in_unit_box(x):
    return np.all(np.abs(np.asarray(x, np.float64)) <= 1.0, axis=1)


def start(D, N, seed):
    return torch.from_numpy(np.random.RandomState(seed).normal(size=(N, D)).astype(np.float32) * 0.5).cuda()


def x_target(sd, mu):
    """lp(x) of the x-space run in the kernel's arithmetic: T in float32 (two roundings), the float64-moment Gaussian of the oracle,
    the unit box on T(x); the identity for the flow"""
    from oracle import oracle as orc
    T = lambda x: (np.asarray(x, np.float32) * sd) + mu
    return latent_target(lambda q: (np.asarray(q, np.float32), np.zeros(len(q))),
                         lambda x: orc.loglike('gaussian', T(x), 1.0, params=[CORR]), lambda x: in_unit_box(T(x)))


def replay(res, x0, inds, u, lp_fn):
    """the restatement step by step from the kernel's own state: the half-step records and the first that may not be compared"""
    hx, hl = res['hist_x'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    records = []
    for i in range(hx.shape[1]):
        rec = []
        stretch_step(x0 if i == 0 else hx[:, i - 1], lp_fn(x0) if i == 0 else hl[:, i - 1], inds[i], u[i], lp_fn, record=rec)
        for r in rec:
            r['step'] = i
        records += rec
    return records, borderline_prefix(records)


@pytest.mark.parametrize('D', [5, 20, 50])
def test_fused_x_kernel_replays_on_its_draws(D):
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import fill_noise
    N, S, seed = max(64, 2 * D), 6, 4321 + D
    sd, mu = affine(D, D)
    x0 = start(D, N, D)
    res = flow.ensemble_x_steps(GAUSS, x0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=seed, like_params=(CORR,))
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed))
    n0 = (N + 1) // 2
    assert np.all((inds == 0).sum(1) == n0) and np.all((inds == 1).sum(1) == N - n0)
    records, ok = replay(res, x0.cpu().numpy(), inds, u, x_target(sd, mu))
    print('D=%d: comparable prefix %d of %d half-steps' % (D, ok, len(records)))
    assert ok >= 4, 'borderline decisions too early to compare anything'
    hx, hl = res['hist_x'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    for r in records[:ok]:
        i, k, acc = r['step'], r['walkers'], r['accept']
        x_prev = x0.cpu().numpy() if i == 0 else hx[:, i - 1]
        moved = np.any(hx[k, i] != x_prev[k], axis=1)
        assert np.array_equal(moved, acc), 'step %d half %d: decisions differ' % (i, r['half'])
        assert np.array_equal(hx[k[acc], i].view(np.uint32), r['q'][acc].view(np.uint32)), 'proposals not bit-equal'
        np.testing.assert_allclose(hl[k[acc], i], r['lp_q'][acc], rtol=1e-6, atol=2e-5)
    assert int(res['n_accept'].sum()) > 0
    np.testing.assert_array_equal(res['x'].cpu().numpy(), hx[:, -1])
    np.testing.assert_array_equal(res['lp'].cpu().numpy(), hl[:, -1])
    np.testing.assert_array_equal(res['tx'].cpu().numpy(), hx[:, -1] * sd + mu)


@pytest.mark.parametrize('with_T', [True, False])
def test_routes_agree(with_T):
    """the fused kernel against ensemble_rounds on an IdentityFlow: the x-space run as it could be computed before the kernel"""
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import IdentityFlow, ensemble_rounds, fill_noise
    D, N, S, seed = 20, 96, 6, 77
    sd, mu = affine(D, 5) if with_T else (None, None)
    x0 = start(D, N, 6) * (1.0 if with_T else 0.6)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=seed, like_params=(CORR,))
    fused = flow.ensemble_x_steps(GAUSS, x0, S, **kw)
    _, rounds = ensemble_rounds(IdentityFlow(x0.device), x0, S, like_id=GAUSS, **kw)
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed))
    one, zero = np.ones(D, np.float32), np.zeros(D, np.float32)
    records, ok = replay(fused, x0.cpu().numpy(), inds, u, x_target(sd if with_T else one, mu if with_T else zero))
    last = records[ok]['step'] if ok < len(records) else S   # steps before the first borderline decision compare bit for bit
    print('first borderline step %d of %d' % (last, S))
    assert last >= 2
    fx, rx = fused['hist_x'].cpu().numpy()[:, :last], rounds['hist_z'].cpu().numpy()[:, :last]
    assert np.array_equal(fx.view(np.uint32), rx.view(np.uint32))
    np.testing.assert_allclose(rounds['hist_lp'].cpu().numpy()[:, :last], fused['hist_lp'].cpu().numpy()[:, :last], rtol=1e-6, atol=2e-5)


def test_chunking_is_bit_exact():
    from nnest_amd import flow
    D, N, S, seed = 20, 80, 8, 42
    sd, mu = affine(D, 8)
    x0 = start(D, N, 8)
    kw = dict(t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,))
    one = flow.ensemble_x_steps(GAUSS, x0, S, **kw)
    x, lp, parts = x0, None, []
    for c in range(4):
        r = flow.ensemble_x_steps(GAUSS, x, S // 4, lp=lp, step0=c * (S // 4), **kw)
        x, lp = r['x'], r['lp']
        parts.append(r)
    for key in ('hist_x', 'hist_lp'):
        assert torch.equal(torch.cat([p[key] for p in parts], 1), one[key]), key
    assert torch.equal(sum(p['n_accept'] for p in parts), one['n_accept'])
    assert torch.equal(parts[-1]['x'], one['x']) and torch.equal(parts[-1]['tx'], one['tx'])


def exact_gauss_box(rng, n, D):
    cov = (1 - CORR) * np.eye(D) + CORR * np.ones((D, D))
    out, have = [], 0
    while have < n:
        x = rng.multivariate_normal(np.zeros(D), cov, size=8 * n)
        x = x[in_unit_box(x)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


def test_invariance_fused():
    """walkers started from exact draws of N(0, Sigma) in the unit box stay exact (T = identity)"""
    from nnest_amd import flow
    D, N, S = 5, 2000, 20
    assert flow.ensemble_x_max_walkers(D, GAUSS) >= N   # (so the fused kernel takes the population)
    rng = np.random.RandomState(21)
    x0 = exact_gauss_box(rng, N, D).astype(np.float32)
    res = flow.ensemble_x_steps(GAUSS, x0, S, lo=-np.ones(D), hi=np.ones(D), seed=5, like_params=(CORR,))
    acc = int(res['n_accept'].sum()) / (N * S)
    p = stationarity_pvalues(res['x'].cpu().numpy(), exact_gauss_box(rng, N, D))
    print('acceptance %.3f, corrected minimum p %.3g' % (acc, min(p.values()) * len(p)))
    assert 0.2 < acc < 0.95
    assert_invariant(p, what='ensemble, x space, fused')


def test_residency_refusal_routes_to_rounds(tmp_path):
    import nnest_amd
    from nnest_amd import _lib, flow
    from nnest_amd.likelihoods import Gaussian
    D = 4
    cap = flow.ensemble_x_max_walkers(D, GAUSS)
    assert cap >= 1024 and cap % 4 == 0
    with pytest.raises(_lib.NnestHipError) as e:
        flow.ensemble_x_steps(GAUSS, start(D, cap + 4, 1), 2, like_params=(CORR,))
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), log_dir=str(tmp_path), log_level=30, flow='nvp')
    out = s._ensemble_sample_x(2, start(D, cap + 4, 1).cpu().numpy(), seed=3)
    assert s.ensemble_route == 'rounds' and out[0].shape == (cap + 4, 2, D) and out[1].shape == (cap + 4, 2)
    x0 = start(D, 64, 2).cpu().numpy()
    fused = s._ensemble_sample_x(4, x0, seed=3)
    assert s.ensemble_route == 'fused' and fused[3] == 64 * 5
    with pytest.raises(ValueError):
        s._ensemble_sample_x(2, start(D, cap + 4, 1).cpu().numpy(), seed=3, route='fused')
    # the pinned round route and another cut into launches compute the same run
    rounds = s._ensemble_sample_x(4, x0, seed=3, route='rounds', chunk_steps=3)
    assert s.ensemble_route == 'rounds'
    np.testing.assert_array_equal(fused[0][:, :1], rounds[0][:, :1])


def _f32(x):
    return np.asarray(x, np.float32)


@pytest.mark.parametrize('case', ['ar1', '3d'])
def test_integrated_autocorr_time(case):
    from nnest_amd.evaluation import integrated_autocorr_time
    if case == 'ar1':
        x = _f32(bc.ar1(np.random.RandomState(0), 32, 4000, 1, 0.9))
    else:   # three dimensions with different times and offsets, a chain length that is no multiple of any tile
        rng = np.random.RandomState(3)
        x = _f32(np.concatenate([bc.ar1(rng, 20, 1531, 1, phi) * sc + off
                                 for phi, sc, off in ((0.5, 1.0, 0.0), (0.8, 30.0, 1000.0), (0.2, 1e-3, -5.0))], axis=2))
    want, win = bc.integrated_time(x.astype(np.float64))
    tau, window = integrated_autocorr_time(x, return_window=True)
    print('%s: tau %r (float64 restatement %r), windows %r' % (case, tau, want, window))
    assert np.array_equal(window, win)
    np.testing.assert_allclose(tau, want, rtol=1e-6, atol=0)
    # read in place through the strides: a view of a longer, wider CUDA tensor
    wide = torch.zeros(x.shape[0], x.shape[1] + 7, x.shape[2] + 2, device='cuda')
    wide[:, 3:3 + x.shape[1], 1:1 + x.shape[2]] = torch.from_numpy(x).cuda()
    np.testing.assert_array_equal(integrated_autocorr_time(wide[:, 3:3 + x.shape[1], 1:1 + x.shape[2]]), tau)


def test_integrated_autocorr_time_short_chain():
    from nnest_amd.evaluation import AutocorrError, integrated_autocorr_time
    x = _f32(bc.ar1(np.random.RandomState(2), 16, 200, 2, 0.9))
    want, _ = bc.integrated_time(x.astype(np.float64), quiet=True)
    with pytest.raises(AutocorrError) as e:
        integrated_autocorr_time(x)
    assert e.value.thresh == 200 / 50
    np.testing.assert_allclose(e.value.tau, want, rtol=1e-6)
    np.testing.assert_allclose(integrated_autocorr_time(x, quiet=True), want, rtol=1e-6)


# The front end's target: the stretch move on Gaussian(4, 0.5) in the box [-5, 5]^4 with 64 walkers started from the prior.
# Its integrated autocorrelation time, from the numpy restatement of the same move (tests/ensemble_check.stretch_run, numpy draws,
# 3000 and 4000 steps, six seeds): max over the dimensions 42 - 46, so tol = 50 needs about 2300 steps; BOOT_STEPS = 4000 leaves
# room for an estimate of 80.  (No MI355X run had measured it when this was written: the test prints the GPU run's tau.)
BOOT_STEPS = 4000


def test_bootstrap_front_end(tmp_path):
    """bootstrap end to end on the fused x-space route.  The 15 % margin on the standard deviation is the issue's; the scatter of that
    quantity over seeds and against equally thinned exact draws has not been measured (it is printed here)."""
    import nnest_amd
    from nnest_amd.evaluation import integrated_autocorr_time
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, N, thin = 4, 64, 10
    np.random.seed(11)
    torch.manual_seed(11)
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30, flow='nvp')
    routes = []
    run_x = s._ensemble_sample_x

    def spy(*a, **kw):
        out = run_x(*a, **kw)
        routes.append(s.ensemble_route)
        print('x-space run: tau %r' % (integrated_autocorr_time(out[0], quiet=True),))
        return out

    s._ensemble_sample_x = spy
    out = s.bootstrap(BOOT_STEPS, N, iters=2, thin=thin, seed=11)
    assert routes == ['fused']
    n = len(out)
    assert out.shape == (n, D) and n > 100
    assert np.all(np.abs(out) <= 5.0)
    assert s.samples.shape == (N, BOOT_STEPS, D) and s.latent_samples.shape == (N, BOOT_STEPS, D) and s.loglikes.shape == (N, BOOT_STEPS)
    assert abs(n - N * BOOT_STEPS / thin) < 6 * np.sqrt(N * BOOT_STEPS / thin)   # each row kept with probability 1 / thin
    # the mean: its variance is that of the chain's mean, sd^2 tau / (N S) by the chain's own autocorrelation time, plus that of
    # keeping a random 1 / thin of its rows, sd^2 (1 - 1 / thin) / n
    tau = integrated_autocorr_time(s.samples[:, :, :D], quiet=True)
    sd = out.std(axis=0)
    se = sd * np.sqrt(tau / (N * BOOT_STEPS) + (1.0 - 1.0 / thin) / n)
    print('n %d mean %r se %r std %r latent tau %r' % (n, out.mean(axis=0), se, sd, tau))
    assert np.all(np.abs(out.mean(axis=0)) < 5 * se)
    assert np.all(np.abs(sd - 1.0) < 0.15)


def test_bootstrap_python_likelihood_on_the_round_route(tmp_path):
    import nnest_amd
    from nnest_amd.priors import UniformPrior
    D, N, S = 3, 32, 3000   # (the restated move on this target: tau 37 - 39 over four seeds, tol = 50 needs about 1950 steps)

    def like(x):
        x = np.asarray(x, np.float64)
        return -0.5 * (x * x).sum(1), x[:, :1] * 2.0

    np.random.seed(5)
    torch.manual_seed(5)
    s = nnest_amd.EnsembleSampler(D, like, prior=UniformPrior(D, -5, 5), num_derived=1, log_dir=str(tmp_path), log_level=30,
                                  flow='nvp')
    routes = []
    run_x = s._ensemble_sample_x
    s._ensemble_sample_x = lambda *a, **kw: (run_x(*a, **kw), routes.append(s.ensemble_route))[0]
    out = s.bootstrap(S, N, iters=1, thin=5, seed=5, init_samples=np.random.RandomState(5).normal(size=(N, D)))
    assert routes == ['rounds'] and s.ensemble_route == 'rounds'
    assert out.ndim == 2 and out.shape[1] == D and len(out) > 0 and np.all(np.abs(out) <= 5.0)
    assert s.samples.shape == (N, S, D + 1) and s.total_calls == 2 * N * (S + 1)
