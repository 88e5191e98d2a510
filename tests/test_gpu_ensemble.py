"""GPU checks of the ensemble sampler (include/nnest_hip.h nnest_ensemble_*): the fused kernel against the numpy restatement on its
exported draws, the round route against the fused one, invariance of exactly sampled targets (unconstrained and under a likelihood
constraint, through an NVP and a spline flow), chunking, the residency refusal and the EnsembleSampler front end."""
import numpy as np
import pytest
import torch

from tests.ensemble_check import borderline_prefix, latent_target, stretch_step
from tests.slice_invariance import assert_invariant, stationarity_pvalues, uniform_on

pytestmark = pytest.mark.gpu

GAUSS = 3   # NNEST_LIKE_GAUSSIAN: N(0, Sigma), Sigma = I + corr (11^T - I)
CORR = 0.5


def gauss_logl(x):
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    s1, s2 = x.sum(1), (x * x).sum(1)
    quad = (s2 - CORR * s1 * s1 / (1.0 + (D - 1.0) * CORR)) / (1.0 - CORR)
    logdet = (D - 1.0) * np.log(1.0 - CORR) + np.log(1.0 + (D - 1.0) * CORR)
    return -0.5 * quad - 0.5 * logdet - 0.5 * D * np.log(2 * np.pi)


def affine(D, seed):
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)


def in_unit_box(x):
    return np.all(np.abs(np.asarray(x, np.float64)) <= 1.0, axis=1)


def start(D, N, seed):
    return torch.from_numpy(np.random.RandomState(seed).normal(size=(N, D)).astype(np.float32) * 0.5).cuda()


def oracle_lp(o, sd, mu, loglstar=None):
    """the latent target of the fused route's arithmetic: oracle inverse (float32), T in float32, the float64-moment Gaussian"""
    from oracle import oracle as orc

    def x_of_z(q):
        x, ld = o.inverse(np.asarray(q, np.float32))
        return x, ld

    def logl(x):
        tx = (np.asarray(x, np.float32) * sd) + mu
        return orc.loglike('gaussian', tx, 1.0, params=[CORR])

    return latent_target(x_of_z, logl, lambda x: in_unit_box((np.asarray(x, np.float32) * sd) + mu), loglstar=loglstar)


def replay(res, z0, inds, u, lp_fn):
    """the restatement step by step from the kernel's own state; returns the half-step records and the index of the first half-step
    that may not be compared (a borderline decision)"""
    hz, hl = res['hist_z'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    S = hz.shape[1]
    records = []
    for i in range(S):
        z_prev = z0 if i == 0 else hz[:, i - 1]
        lp_prev = lp_fn(z0) if i == 0 else hl[:, i - 1]
        rec = []
        stretch_step(z_prev, lp_prev, inds[i], u[i], lp_fn, record=rec)
        for r in rec:
            r['step'] = i
        records += rec
    return records, borderline_prefix(records)


@pytest.mark.parametrize('D', [5, 20, 50])
def test_fused_kernel_replays_on_its_draws(D):
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import fill_noise
    from oracle import oracle as orc
    N, S, seed = max(64, 2 * D), 6, 1234 + D
    nvp = flow.HipNVP(D, 16, 3, 1, seed=D)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    sd, mu = affine(D, D)
    z0 = start(D, N, D)
    res = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=seed, like_params=(CORR,))
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed))
    n0 = (N + 1) // 2
    assert np.all((inds == 0).sum(1) == n0) and np.all((inds == 1).sum(1) == N - n0)
    lp_fn = oracle_lp(o, sd, mu)
    records, ok = replay(res, z0.cpu().numpy(), inds, u, lp_fn)
    assert ok >= 4, 'borderline decisions too early to compare anything'
    hz, hl = res['hist_z'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    for r in records[:ok]:
        i, k, acc = r['step'], r['walkers'], r['accept']
        z_prev = z0.cpu().numpy() if i == 0 else hz[:, i - 1]
        moved = np.any(hz[k, i] != z_prev[k], axis=1)
        assert np.array_equal(moved, acc), 'step %d half %d: decisions differ' % (i, r['half'])
        assert np.array_equal(hz[k[acc], i].view(np.uint32), r['q'][acc].view(np.uint32)), 'proposals not bit-equal'
        lq = r['lp_q'][acc]
        np.testing.assert_allclose(hl[k[acc], i], lq, rtol=1e-6, atol=2e-5)
    assert int(res['n_accept'].sum()) > 0
    np.testing.assert_array_equal(res['z'].cpu().numpy(), hz[:, -1])
    np.testing.assert_array_equal(res['lp'].cpu().numpy(), hl[:, -1])


def test_routes_agree():
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import ensemble_rounds, fill_noise
    from oracle import oracle as orc
    D, N, S, seed = 20, 96, 6, 77
    nvp = flow.HipNVP(D, 16, 3, 1, seed=3)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    sd, mu = affine(D, 5)
    z0 = start(D, N, 6)
    box = dict(lo=-np.ones(D), hi=np.ones(D))
    fused = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,), **box)
    _, rounds = ensemble_rounds(nvp, z0, S, like_id=GAUSS, like_params=(CORR,), t_std=sd, t_mean=mu, seed=seed, **box)
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed))
    records, ok = replay(fused, z0.cpu().numpy(), inds, u, oracle_lp(o, sd, mu))
    last = records[ok]['step'] if ok < len(records) else S   # steps before the first borderline decision compare bit for bit
    assert last >= 2
    fz, rz = fused['hist_z'].cpu().numpy()[:, :last], rounds['hist_z'].cpu().numpy()[:, :last]
    assert np.array_equal(fz.view(np.uint32), rz.view(np.uint32))
    np.testing.assert_allclose(rounds['hist_lp'].cpu().numpy()[:, :last], fused['hist_lp'].cpu().numpy()[:, :last], rtol=1e-6, atol=2e-5)
    np.testing.assert_allclose(rounds['hist_x'].cpu().numpy()[:, :last], fused['hist_x'].cpu().numpy()[:, :last], atol=2e-5)


def exact_gauss_box(rng, n, D):
    cov = (1 - CORR) * np.eye(D) + CORR * np.ones((D, D))
    out, have = [], 0
    while have < n:
        x = rng.multivariate_normal(np.zeros(D), cov, size=8 * n)
        x = x[in_unit_box(x)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


def test_invariance_unconstrained_fused():
    """walkers started from exact draws of N(0, Sigma) in the box, seen through T and a random NVP, stay exact"""
    from nnest_amd import flow
    D, N, S = 5, 2000, 20
    nvp = flow.HipNVP(D, 16, 3, 1, seed=21)
    assert nvp.ensemble_max_walkers(GAUSS) >= N
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(21)
    tx0 = exact_gauss_box(rng, N, D)
    z0, _ = nvp.forward(((tx0 - mu) / sd).astype(np.float32))
    res = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=5, like_params=(CORR,))
    tx = res['x'].cpu().numpy() * sd + mu
    assert 0.2 < int(res['n_accept'].sum()) / (N * S) < 0.95
    assert_invariant(stationarity_pvalues(tx, exact_gauss_box(rng, N, D)), what='ensemble, fused, unconstrained')


@pytest.mark.parametrize('route', ['fused', 'rounds_spline'])
def test_invariance_constrained(route):
    """with loglstar the target is uniform on {logL > L*} in the box"""
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import ensemble_rounds
    from nnest_amd.spline import HipSpline
    D, N, S = 5, 2000, 15
    star = float(np.quantile(gauss_logl(np.random.RandomState(0).uniform(-1, 1, (20000, D))), 0.5))
    inside = lambda x: gauss_logl(x) > star
    rng = np.random.RandomState(31)
    sd, mu = affine(D, 31)
    tx0 = uniform_on(rng, N, D, inside)
    x0 = ((tx0 - mu) / sd).astype(np.float32)
    box = dict(lo=-np.ones(D), hi=np.ones(D))
    if route == 'fused':
        nvp = flow.HipNVP(D, 16, 3, 1, seed=31)
        z0, _ = nvp.forward(x0)
        res = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, loglstar=star, seed=9, like_params=(CORR,), **box)
        x, nacc = res['x'], res['n_accept']
    else:
        sp = HipSpline(D, 16, 3, seed=31)
        z0, _ = sp.forward(x0)   # (the first forward sets the ActNorm layers from these points)
        st, _ = ensemble_rounds(sp, z0, S, like_id=GAUSS, like_params=(CORR,), t_std=sd, t_mean=mu, loglstar=star, seed=9, **box)
        x, nacc = st.x, st.n_accept
    tx = x.cpu().numpy() * sd + mu
    assert np.all(inside(tx)) and np.all(in_unit_box(tx))
    assert 0.2 < int(nacc.sum()) / (N * S) < 0.95
    assert_invariant(stationarity_pvalues(tx, uniform_on(rng, N, D, inside)), what='ensemble, %s, constrained' % route)


def test_chunking_is_bit_exact():
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import ensemble_rounds
    D, N, S, seed = 20, 80, 8, 42
    nvp = flow.HipNVP(D, 16, 3, 1, seed=8)
    sd, mu = affine(D, 8)
    z0 = start(D, N, 8)
    kw = dict(t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,))
    one = nvp.ensemble_steps(GAUSS, z0, S, **kw)
    z, lp, parts = z0, None, []
    for c in range(4):
        r = nvp.ensemble_steps(GAUSS, z, S // 4, lp=lp, step0=c * (S // 4), **kw)
        z, lp = r['z'], r['lp']
        parts.append(r)
    for key in ('hist_z', 'hist_x', 'hist_lp'):
        assert torch.equal(torch.cat([p[key] for p in parts], 1), one[key]), key
    assert torch.equal(sum(p['n_accept'] for p in parts), one['n_accept'])
    # the round route likewise
    _, rone = ensemble_rounds(nvp, z0, S, like_id=GAUSS, **kw)
    st, rparts = None, []
    for c in range(4):
        st, h = ensemble_rounds(nvp, z0, S // 4, state=st, like_id=GAUSS, step0=c * (S // 4), **kw)
        rparts.append(h)
    for key in ('hist_z', 'hist_x', 'hist_lp'):
        assert torch.equal(torch.cat([p[key] for p in rparts], 1), rone[key]), key


def test_residency_refusal_routes_to_rounds(tmp_path):
    import nnest_amd
    from nnest_amd import _lib
    from nnest_amd.likelihoods import Gaussian
    D = 4
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), log_dir=str(tmp_path), log_level=30, flow='nvp')
    nvp = s.trainer.netG
    cap = nvp.ensemble_max_walkers(GAUSS)
    assert cap >= 1024 and cap % 4 == 0
    with pytest.raises(_lib.NnestHipError) as e:
        nvp.ensemble_steps(GAUSS, start(D, cap + 4, 1), 2, like_params=(CORR,))
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    out = s._ensemble_sample(2, cap + 4, seed=3)
    assert s.ensemble_route == 'rounds' and out[0].shape == (cap + 4, 2, D)
    s._ensemble_sample(2, 64, seed=3)
    assert s.ensemble_route == 'fused'


def _train(rng, D, n=1000):
    return rng.multivariate_normal(np.zeros(D), (1 - CORR) * np.eye(D) + CORR * np.ones((D, D)), size=n)


@pytest.mark.parametrize('flow_name,known', [('nvp', True), ('nvp', False), ('spline', True), ('spline', False)])
def test_front_end(tmp_path, flow_name, known):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, N, S = 3, 32, 12
    rng = np.random.RandomState(2)
    np.random.seed(2)
    torch.manual_seed(2)
    if known:
        like, nd = Gaussian(D, CORR), 0
    else:
        def like(x):
            return gauss_logl(x), np.stack([x.sum(1), (x * x).sum(1)], 1)
        nd = 2
    s = nnest_amd.EnsembleSampler(D, like, prior=UniformPrior(D, -5, 5), num_derived=nd, log_dir=str(tmp_path), log_level=30,
                                  flow=flow_name)
    s.trainer.train = lambda samples, jitter=0.0, **kw: None   # (keep the test short: the flow stays at its initialisation)
    s.run(S, N, _train(rng, D))
    assert s.samples.shape == (N, S, D + nd) and s.latent_samples.shape == (N, S, D) and s.loglikes.shape == (N, S)
    assert s.total_calls == N * (S + 1)
    assert s.ensemble_route == ('fused' if known and flow_name == 'nvp' else 'rounds')
    acc = s.total_accepted / float(N * S)
    assert 0.0 < acc < 1.0
    if nd:
        assert np.all(s.samples[:, :, D:] == 0)   # derived values are zeros without loglstar (sampler.py:687)
    assert np.all(np.isfinite(s.loglikes))


def test_front_end_derived_with_loglstar(tmp_path):
    """the round route with a Python likelihood carries the derived parameters of the accepted proposals under a constraint"""
    import nnest_amd
    D, N, S = 3, 24, 6

    def like(x):
        return gauss_logl(x), x[:, :1] * 2.0

    s = nnest_amd.EnsembleSampler(D, like, num_derived=1, log_dir=str(tmp_path), log_level=30, flow='spline')
    x0 = _train(np.random.RandomState(4), D, 400)[:N] * 0.3
    star = float(gauss_logl(x0).min()) - 1.0
    samples, latent, derived, loglikes, ncall = s._ensemble_sample(S, N, init_samples=x0, loglstar=star, seed=4)
    assert ncall == N * (S + 1) and s.total_calls == N * (S + 1)
    np.testing.assert_allclose(derived[:, :, 0], samples[:, :, 0] * 2.0, rtol=1e-5, atol=1e-6)
