"""GPU checks of the spline flow's fused stretch-move kernel (include/nnest_hip.h nnest_spline_ensemble_steps; HipSpline.ensemble_steps):
the kernel against the numpy restatement on its exported draws with the oracle's spline inverse, the fused route against the round
route on the same flow, invariance of exactly sampled targets (unconstrained and under a likelihood constraint), chunking, the
residency refusal and the EnsembleSampler front end (route='fused').

Tolerances.  LP_TOL: hist_lp and hist_x against the oracle and against the round route, relative to 1 + |value|: the bound
tests/test_gpu_spline.py line 93 puts on the inverse's x and log-det against the oracle (`rel(cpu(x), xo) < 3e-5 and rel(cpu(ld),
ldo) < 3e-5`); the Gaussian likelihood is a float64 function of that x.  Decisions: the log-det is a float32 sum taken in another
order than the oracle's (and than the round route's one-wave-per-tile inverse), so a decision whose margin |lnpdiff - log u3| is below
tests/mh_checks.MARGIN_TOL -- the level that module derives for such sums -- may fall the other way: half-steps are compared
decision for decision up to the first such one, and a decision that differs anywhere is held to assert_borderline on the oracle's
margin.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests.ensemble_check import borderline_prefix, latent_target, stretch_step
from tests.mh_checks import MARGIN_TOL, assert_borderline
from tests.slice_invariance import assert_invariant, stationarity_pvalues, uniform_on

pytestmark = pytest.mark.gpu

GAUSS = 3   # NNEST_LIKE_GAUSSIAN: N(0, Sigma), Sigma = I + corr (11^T - I)
CORR = 0.5
LP_TOL = 3e-5
TILE = 16   # walkers per workgroup of the team form


def rel(a, b):
    """max |a - b| / (1 + |b|) over the finite entries; the others (lp = -inf outside the box or below L*) must be equal"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin]), 'non-finite entries differ'
    return float(np.max(np.abs(a[fin] - b[fin]) / (1.0 + np.abs(b[fin])))) if fin.any() else 0.0


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


def spline_and_start(D, H, N, seed):
    """a HipSpline at its random initialisation with the ActNorm layers set from the start points (its first forward), the oracle on
    the same weights, and the walkers' start z0 = f(x0)"""
    from nnest_amd.spline import HipSpline
    from oracle import oracle as orc
    sp = HipSpline(D, H, 3, seed=seed)
    x0 = np.random.RandomState(seed).normal(size=(N, D)).astype(np.float32) * 0.5
    z0, _ = sp.forward(x0)
    o = orc.Spline(D, H, 3, 8, 3.0, sp.store_packed(), sp.P)
    return sp, o, z0.contiguous()


def oracle_lp(o, sd, mu, loglstar=None):
    """the latent target in the fused route's arithmetic: the oracle's inverse (float32), T in float32, the float64-moment Gaussian"""
    from oracle import oracle as orc
    T = lambda x: (np.asarray(x, np.float32) * sd) + mu
    return latent_target(lambda q: o.inverse(np.asarray(q, np.float32)), lambda x: orc.loglike('gaussian', T(x), 1.0, params=[CORR]),
                         lambda x: in_unit_box(T(x)), loglstar=loglstar)


def replay(res, z0, inds, u, lp_fn):
    """the restatement step by step from the kernel's own previous state (as tests/test_gpu_ensemble.replay); returns the half-step
    records and the number of leading half-steps without a borderline decision"""
    hz, hl = res['hist_z'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    records = []
    for i in range(hz.shape[1]):
        z_prev = z0 if i == 0 else hz[:, i - 1]
        lp_prev = lp_fn(z0) if i == 0 else hl[:, i - 1]
        rec = []
        stretch_step(z_prev, lp_prev, inds[i], u[i], lp_fn, record=rec)
        for r in rec:
            r['step'] = i
        records += rec
    return records, borderline_prefix(records, margin=MARGIN_TOL)


def check_against_replay(res, z0, records, ok):
    """every half-step of the replay against the kernel's history.  Proposals bit-equal and lp within LP_TOL wherever both accepted;
    decisions equal on the first `ok` half-steps; a decision that differs later must be borderline by the oracle's margin, and the
    second half of that step (whose partners then differ) is not compared."""
    hz, hl = res['hist_z'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    worst_lp, parted_step = 0.0, -1
    for n, r in enumerate(records):
        i, k, acc = r['step'], r['walkers'], r['accept']
        if i == parted_step:
            continue
        z_prev = z0 if i == 0 else hz[:, i - 1]
        moved = np.any(hz[k, i] != z_prev[k], axis=1)
        differ = np.flatnonzero(moved != acc)
        if n < ok:
            assert len(differ) == 0, 'step %d half %d: decisions differ before any borderline one' % (i, r['half'])
        if len(differ):
            margins = np.abs(r['lnpdiff'] - r['logu3'])
            print('step %d half %d: %d decisions differ, margins %r' % (i, r['half'], len(differ), margins[differ]))
            h_gpu = np.stack([z_prev[k], hz[k, i]], 1)
            h_orc = np.stack([z_prev[k], np.where(acc[:, None], r['q'], z_prev[k])], 1)
            assert_borderline(h_gpu, h_orc, margins[None, :], differ)
            parted_step = i
        both = moved & acc
        assert np.array_equal(hz[k[both], i].view(np.uint32), r['q'][both].view(np.uint32)), 'proposals not bit-equal'
        worst_lp = max(worst_lp, rel(hl[k[both], i], r['lp_q'][both]))
    return worst_lp


@pytest.mark.parametrize('D,H', [(5, 16), (20, 16), (50, 16), (5, 10)])
def test_fused_kernel_replays_on_its_draws(D, H):
    from nnest_amd.ensemble_rounds import fill_noise
    N, S, seed = max(64, 2 * D), 6, 4321 + D + H
    sp, o, z0 = spline_and_start(D, H, N, D + H)
    sd, mu = affine(D, D)
    res = sp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=seed, like_params=(CORR,))
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed))
    lp_fn = oracle_lp(o, sd, mu)
    z0n = z0.cpu().numpy()
    records, ok = replay(res, z0n, inds, u, lp_fn)
    worst = check_against_replay(res, z0n, records, ok)
    print('D %d H %d: %d of %d half-steps before the first borderline decision; hist_lp against the oracle: %.3g (tolerance %.3g)'
          % (D, H, ok, len(records), worst, LP_TOL))
    assert ok >= 4, 'borderline decisions too early to compare anything'
    assert worst < LP_TOL
    hz, hl = res['hist_z'].cpu().numpy(), res['hist_lp'].cpu().numpy()
    xo, _ = o.inverse(hz[:, -1])
    print('hist_x against the oracle: %.3g' % rel(res['hist_x'].cpu().numpy()[:, -1], xo))
    assert rel(res['hist_x'].cpu().numpy()[:, -1], xo) < LP_TOL
    assert int(res['n_accept'].sum()) > 0
    np.testing.assert_array_equal(res['z'].cpu().numpy(), hz[:, -1])
    np.testing.assert_array_equal(res['lp'].cpu().numpy(), hl[:, -1])
    np.testing.assert_array_equal(res['x'].cpu().numpy(), res['hist_x'].cpu().numpy()[:, -1])
    moved = np.any(np.diff(np.concatenate([z0n[:, None], hz], 1), axis=1) != 0, axis=2).sum(1)
    np.testing.assert_array_equal(res['n_accept'].cpu().numpy(), moved)


def test_routes_agree():
    from nnest_amd.ensemble_rounds import ensemble_rounds, fill_noise
    D, N, S, seed = 20, 96, 6, 77
    sp, o, z0 = spline_and_start(D, 16, N, 3)
    sd, mu = affine(D, 5)
    box = dict(lo=-np.ones(D), hi=np.ones(D))
    fused = sp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,), **box)
    _, rounds = ensemble_rounds(sp, z0, S, like_id=GAUSS, like_params=(CORR,), t_std=sd, t_mean=mu, seed=seed, **box)
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed))
    records, ok = replay(fused, z0.cpu().numpy(), inds, u, oracle_lp(o, sd, mu))
    last = records[ok]['step'] if ok < len(records) else S   # steps before the first borderline decision compare bit for bit
    print('steps before the first borderline decision: %d of %d' % (last, S))
    assert last >= 2
    fz, rz = fused['hist_z'].cpu().numpy()[:, :last], rounds['hist_z'].cpu().numpy()[:, :last]
    assert np.array_equal(fz.view(np.uint32), rz.view(np.uint32))
    dlp = rel(rounds['hist_lp'].cpu().numpy()[:, :last], fused['hist_lp'].cpu().numpy()[:, :last])
    dx = rel(rounds['hist_x'].cpu().numpy()[:, :last], fused['hist_x'].cpu().numpy()[:, :last])
    print('round route against fused: hist_lp %.3g hist_x %.3g (tolerance %.3g)' % (dlp, dx, LP_TOL))
    assert dlp < LP_TOL and dx < LP_TOL


def exact_gauss_box(rng, n, D):
    cov = (1 - CORR) * np.eye(D) + CORR * np.ones((D, D))
    out, have = [], 0
    while have < n:
        x = rng.multivariate_normal(np.zeros(D), cov, size=8 * n)
        x = x[in_unit_box(x)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


def test_invariance_unconstrained():
    """walkers started from exact draws of N(0, Sigma) in the box, seen through T and a spline flow, stay exact"""
    from nnest_amd.spline import HipSpline
    D, N, S = 5, 2000, 20
    sp = HipSpline(D, 16, 3, seed=21)
    assert sp.ensemble_max_walkers(GAUSS) >= N
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(21)
    tx0 = exact_gauss_box(rng, N, D)
    z0, _ = sp.forward(((tx0 - mu) / sd).astype(np.float32))   # (the first forward sets the ActNorm layers from these points)
    res = sp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=5, like_params=(CORR,))
    tx = res['x'].cpu().numpy() * sd + mu
    rate = int(res['n_accept'].sum()) / (N * S)
    print('acceptance %.3f' % rate)
    assert 0.2 < rate < 0.95
    assert_invariant(stationarity_pvalues(tx, exact_gauss_box(rng, N, D)), what='spline ensemble, fused, unconstrained')


def test_invariance_constrained():
    """with loglstar the target is uniform on {logL > L*} in the box"""
    from nnest_amd.spline import HipSpline
    D, N, S = 5, 2000, 15
    star = float(np.quantile(gauss_logl(np.random.RandomState(0).uniform(-1, 1, (20000, D))), 0.5))
    inside = lambda x: gauss_logl(x) > star
    rng = np.random.RandomState(31)
    sd, mu = affine(D, 31)
    tx0 = uniform_on(rng, N, D, inside)
    sp = HipSpline(D, 16, 3, seed=31)
    z0, _ = sp.forward(((tx0 - mu) / sd).astype(np.float32))
    res = sp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), loglstar=star, seed=9, like_params=(CORR,))
    tx = res['x'].cpu().numpy() * sd + mu
    assert np.all(inside(tx)) and np.all(in_unit_box(tx))
    rate = int(res['n_accept'].sum()) / (N * S)
    print('acceptance %.3f' % rate)
    assert 0.2 < rate < 0.95
    assert_invariant(stationarity_pvalues(tx, uniform_on(rng, N, D, inside)), what='spline ensemble, fused, constrained')


def test_chunking_is_bit_exact():
    D, N, S, seed = 20, 80, 8, 42
    sp, _, z0 = spline_and_start(D, 16, N, 8)
    sd, mu = affine(D, 8)
    kw = dict(t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,))
    one = sp.ensemble_steps(GAUSS, z0, S, **kw)
    z, lp, parts = z0, None, []
    for c in range(4):
        r = sp.ensemble_steps(GAUSS, z, S // 4, lp=lp, step0=c * (S // 4), **kw)
        z, lp = r['z'], r['lp']
        parts.append(r)
    for key in ('hist_z', 'hist_x', 'hist_lp'):
        assert torch.equal(torch.cat([p[key] for p in parts], 1), one[key]), key
    assert torch.equal(sum(p['n_accept'] for p in parts), one['n_accept'])
    assert int(one['n_accept'].sum()) > 0


def test_residency_refusal(tmp_path):
    import nnest_amd
    from nnest_amd import _lib
    from nnest_amd.likelihoods import Gaussian
    D = 4
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), log_dir=str(tmp_path), log_level=30, flow='spline')
    sp = s.trainer.netG
    cap = sp.ensemble_max_walkers(GAUSS)
    print('resident population: %d walkers' % cap)
    assert cap > 0 and cap % TILE == 0
    z = torch.from_numpy(np.random.RandomState(1).normal(size=(cap + TILE, D)).astype(np.float32) * 0.5).cuda()
    with pytest.raises(_lib.NnestHipError) as e:
        sp.ensemble_steps(GAUSS, z, 2, like_params=(CORR,))
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    with pytest.raises(ValueError, match='fused route'):
        s._ensemble_sample(2, cap + TILE, seed=3, route='fused')
    out = s._ensemble_sample(2, 64, seed=3, route='fused')
    assert s.ensemble_route == 'fused' and out[0].shape == (64, 2, D)
    s._ensemble_sample(2, 64, seed=3)
    assert s.ensemble_route == 'rounds'   # (the default stays the round route for the spline)


def _train(rng, D, n=1000):
    return rng.multivariate_normal(np.zeros(D), (1 - CORR) * np.eye(D) + CORR * np.ones((D, D)), size=n)


def test_front_end(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, N, S = 3, 32, 12
    rng = np.random.RandomState(2)
    np.random.seed(2)
    torch.manual_seed(2)

    def sampler(like, nd=0):
        s = nnest_amd.EnsembleSampler(D, like, prior=UniformPrior(D, -5, 5), num_derived=nd, log_dir=str(tmp_path), log_level=30)
        assert type(s.trainer.netG).__name__ == 'HipSpline'   # flow='spline' is the default
        s.trainer.train = lambda samples, jitter=0.0, **kw: None   # (keep the test short: the flow stays at its initialisation)
        return s

    s = sampler(Gaussian(D, CORR))
    s.run(S, N, _train(rng, D), route='fused')
    assert s.ensemble_route == 'fused'
    assert s.samples.shape == (N, S, D) and s.latent_samples.shape == (N, S, D) and s.loglikes.shape == (N, S)
    assert s.total_calls == N * (S + 1)
    assert 0.0 < s.total_accepted / float(N * S) < 1.0
    assert np.all(np.isfinite(s.loglikes))
    s = sampler(Gaussian(D, CORR))
    s.run(S, N, _train(rng, D))
    assert s.ensemble_route == 'rounds'
    s = sampler(lambda x: (gauss_logl(x), np.stack([x.sum(1), (x * x).sum(1)], 1)), nd=2)
    with pytest.raises(ValueError, match='fused route'):
        s.run(S, N, _train(rng, D), route='fused')


def test_bootstrap_takes_the_fused_route_in_its_latent_rounds(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, N, S = 4, 64, 4000   # (tests/test_gpu_bootstrap.py BOOT_STEPS: the x-space run must be 50 autocorrelation times long)
    np.random.seed(11)
    torch.manual_seed(11)
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30)
    s.trainer.train = lambda samples, jitter=0.0, **kw: None
    routes = []
    run_x, run_z = s._ensemble_sample_x, s._ensemble_sample
    s._ensemble_sample_x = lambda *a, **kw: (run_x(*a, **kw), routes.append(('x', s.ensemble_route)))[0]
    s._ensemble_sample = lambda *a, **kw: (run_z(*a, **kw), routes.append(('z', s.ensemble_route)))[0]
    out = s.bootstrap(S, N, iters=2, thin=10, seed=11, route='fused')
    assert routes == [('x', 'fused'), ('z', 'fused'), ('z', 'fused')]
    assert out.ndim == 2 and out.shape[1] == D and len(out) > 0
    assert s.samples.shape == (N, S, D) and s.latent_samples.shape == (N, S, D) and s.loglikes.shape == (N, S)
    assert s.total_calls == 3 * N * (S + 1)
