"""GPU checks of the ensemble sampler's move mixtures (include/nnest_hip.h nnest_ensemble_moves_*): emcee's differential-evolution
move beside the stretch move.  The fused kernels and the round route against the numpy restatement on their exported draws
(fill_noise, fill_moves), the routes against each other, chunking, the stretch move unchanged through the new entries, invariance of
exactly sampled targets, the residency refusal and the EnsembleSampler front end."""
import numpy as np
import pytest
import torch

from tests.ensemble_check import borderline_prefix, latent_target
from tests.ensemble_moves_check import DE, STRETCH, de_gamma0, moves_run, moves_step, numpy_moves_draws
from tests.slice_invariance import assert_invariant, stationarity_pvalues, uniform_on
from tests.test_gpu_ensemble import CORR, GAUSS, _train, affine, exact_gauss_box, gauss_logl, in_unit_box, oracle_lp, start

pytestmark = pytest.mark.gpu

DE_ONLY = {'de': 1.0}
MIX = {'stretch': 0.5, 'de': 0.5}
MOVED = 0.9   # a frozen chain is trivially invariant: each invariance run must have moved this fraction of its walkers


def draws(N, D, S, seed, moves, step0=0):
    from nnest_amd.ensemble_rounds import fill_moves, fill_noise
    inds, u = (t.cpu().numpy() for t in fill_noise(N, S, seed=seed, step0=step0))
    move, jb, gamma = (t.cpu().numpy() for t in fill_moves(N, D, S, moves=moves, seed=seed, step0=step0))
    return inds, u, move, jb, gamma


def move_ids_by_the_rule(seed, S, moves):
    """m_t < thr recomputed from the definition: word 0 of Philox(seed; 0, t, 1, 4 << 28), thr = floor(p_stretch 2^24)"""
    from oracle import oracle as orc
    ws, wd = float(moves.get('stretch', 0.0)), float(moves.get('de', 0.0))
    thr = int(np.floor(ws / (ws + wd) * (1 << 24)))
    m = [orc.philox4x32_10([0, t, 1, 4 << 28], [seed & 0xffffffff, seed >> 32])[0] >> 8 for t in range(S)]
    return np.array([STRETCH if v < thr else DE for v in m], np.int32)


def check_draws(N, D, inds, u, move, jb, gamma, seed, moves):
    S = len(move)
    np.testing.assert_array_equal(move, move_ids_by_the_rule(seed, S, moves))
    n0 = (N + 1) // 2
    assert np.all((inds == 0).sum(1) == n0) and np.all((inds == 1).sum(1) == N - n0)
    nc = np.where(inds == 0, N - n0, n0)
    m2 = np.round(u[:, :, 1].astype(np.float64) * (1 << 24)).astype(np.int64)
    ja = (m2 * nc) >> 24
    assert np.all(jb != ja) and np.all(jb >= 0) and np.all(jb < nc)
    # gamma = g0 (1 + 1e-5 n): within 1e-4 of g0 for |n| < 10, and not constant
    g0 = de_gamma0(D)
    assert np.all(np.abs(gamma / g0 - 1.0) < 1e-4) and gamma.std() > 0


def replay(hist, hist_lp, z0, d, lp_fn):
    """the restatement step by step from the kernel's own previous state; the half-step records and the number of leading
    half-steps without a borderline decision (margin 1e-5, tests/ensemble_check.py)"""
    inds, u, move, jb, gamma = d
    records = []
    for i in range(hist.shape[1]):
        z_prev = z0 if i == 0 else hist[:, i - 1]
        lp_prev = lp_fn(z0) if i == 0 else hist_lp[:, i - 1]
        rec = []
        moves_step(z_prev, lp_prev, inds[i], u[i], move[i], jb[i], gamma[i], lp_fn, record=rec)
        for r in rec:
            r['step'] = i
        records += rec
    return records, borderline_prefix(records)


def check_replay(hist, hist_lp, z0, records, ok, lp_close):
    assert ok >= 4, 'borderline decisions too early to compare anything'
    for r in records[:ok]:
        i, k, acc = r['step'], r['walkers'], r['accept']
        z_prev = z0 if i == 0 else hist[:, i - 1]
        moved = np.any(hist[k, i] != z_prev[k], axis=1)
        assert np.array_equal(moved, acc), 'step %d half %d (move %d): decisions differ' % (i, r['half'], r['move'])
        assert np.array_equal(hist[k[acc], i].view(np.uint32), r['q'][acc].view(np.uint32)), 'proposals not bit-equal (move %d)' % r['move']
        lp_close(hist_lp[k[acc], i], r['lp_q'][acc])
    return set(r['move'] for r in records[:ok])


def nvp_lp_close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=2e-5)


@pytest.mark.parametrize('moves', [DE_ONLY, MIX], ids=['de', 'mix'])
@pytest.mark.parametrize('D', [5, 20, 50])
def test_fused_kernel_replays_on_its_draws(D, moves):
    from nnest_amd import flow
    from oracle import oracle as orc
    N, S, seed = 2 * D + 1, 8, 1234 + D   # (an odd population: the sets differ in size; D = 5: Nc = 5 and 6)
    nvp = flow.HipNVP(D, 16, 3, 1, seed=D)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    sd, mu = affine(D, D)
    z0 = start(D, N, D)
    res = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=seed, like_params=(CORR,), moves=moves)
    d = draws(N, D, S, seed, moves)
    check_draws(N, D, *d, seed=seed, moves=moves)
    kinds = set(d[2].tolist())
    assert kinds == ({DE} if moves is DE_ONLY else {STRETCH, DE}), 'the seed must give a step of each kind'
    hz, hl, z0n = res['hist_z'].cpu().numpy(), res['hist_lp'].cpu().numpy(), z0.cpu().numpy()
    records, ok = replay(hz, hl, z0n, d, oracle_lp(o, sd, mu))
    seen = check_replay(hz, hl, z0n, records, ok, nvp_lp_close)
    print('D %d %s: %d of %d half-steps compared, moves seen %s, acceptance %.3f' % (
        D, moves, ok, len(records), sorted(seen), float(res['n_accept'].sum()) / (N * S)))
    assert DE in seen
    assert int(res['n_accept'].sum()) > 0
    np.testing.assert_array_equal(res['z'].cpu().numpy(), hz[:, -1])
    np.testing.assert_array_equal(res['lp'].cpu().numpy(), hl[:, -1])


@pytest.mark.parametrize('D', [5, 70])
def test_x_space_kernel_replays_on_its_draws(D):
    """T = identity, no box: lp(x) = logL(x); D = 70 is the third register shape (U = 3)"""
    from nnest_amd import flow
    from oracle import oracle as orc
    N, S, seed = 2 * D + 1, 8, 4321 + D
    x0 = start(D, N, D + 1)
    res = flow.ensemble_x_steps(GAUSS, x0, S, seed=seed, like_params=(CORR,), moves=DE_ONLY)
    d = draws(N, D, S, seed, DE_ONLY)
    check_draws(N, D, *d, seed=seed, moves=DE_ONLY)
    lp_fn = latent_target(lambda q: (np.asarray(q, np.float32), np.zeros(len(q))),
                          lambda x: orc.loglike('gaussian', np.asarray(x, np.float32), 1.0, params=[CORR]), lambda x: np.ones(len(x), bool))
    hx, hl, x0n = res['hist_x'].cpu().numpy(), res['hist_lp'].cpu().numpy(), x0.cpu().numpy()
    records, ok = replay(hx, hl, x0n, d, lp_fn)
    check_replay(hx, hl, x0n, records, ok, nvp_lp_close)
    print('D %d: %d of %d half-steps compared, acceptance %.3f' % (D, ok, len(records), float(res['n_accept'].sum()) / (N * S)))
    assert int(res['n_accept'].sum()) > 0
    np.testing.assert_array_equal(res['x'].cpu().numpy(), hx[:, -1])


def test_routes_agree():
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import ensemble_rounds
    from oracle import oracle as orc
    D, N, S, seed = 20, 96, 6, 1239   # (a seed whose first step is a DE step, its second a stretch step)
    nvp = flow.HipNVP(D, 16, 3, 1, seed=3)
    o = orc.NVP(D, 16, 3, 1, nvp.store_packed())
    sd, mu = affine(D, 5)
    z0 = start(D, N, 6)
    box = dict(lo=-np.ones(D), hi=np.ones(D))
    fused = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,), moves=MIX, **box)
    _, rounds = ensemble_rounds(nvp, z0, S, like_id=GAUSS, like_params=(CORR,), t_std=sd, t_mean=mu, seed=seed, moves=MIX, **box)
    d = draws(N, D, S, seed, MIX)
    assert set(d[2].tolist()) == {STRETCH, DE}, 'the seed must give a step of each kind'
    records, ok = replay(fused['hist_z'].cpu().numpy(), fused['hist_lp'].cpu().numpy(), z0.cpu().numpy(), d, oracle_lp(o, sd, mu))
    last = records[ok]['step'] if ok < len(records) else S   # steps before the first borderline decision compare bit for bit
    print('steps before the first borderline decision: %d of %d; moves %s' % (last, S, d[2].tolist()))
    assert last >= 2 and DE in d[2][:last]
    fz, rz = fused['hist_z'].cpu().numpy()[:, :last], rounds['hist_z'].cpu().numpy()[:, :last]
    assert np.array_equal(fz.view(np.uint32), rz.view(np.uint32))
    np.testing.assert_allclose(rounds['hist_lp'].cpu().numpy()[:, :last], fused['hist_lp'].cpu().numpy()[:, :last], rtol=1e-6, atol=2e-5)
    np.testing.assert_allclose(rounds['hist_x'].cpu().numpy()[:, :last], fused['hist_x'].cpu().numpy()[:, :last], atol=2e-5)


def test_rounds_through_the_spline_replay_on_their_draws():
    """the round route through a flow without a fused DE kernel.  lp against the oracle within the tolerance
    tests/test_gpu_spline_ensemble.py holds that flow's inverse to (LP_TOL, relative to 1 + |lp|)"""
    from nnest_amd.ensemble_rounds import ensemble_rounds
    from tests.test_gpu_spline_ensemble import LP_TOL, oracle_lp as spline_lp, rel, spline_and_start
    D, N, S, seed = 5, 11, 8, 99
    sp, o, z0 = spline_and_start(D, 16, N, 7)
    sd, mu = affine(D, 7)
    _, h = ensemble_rounds(sp, z0, S, like_id=GAUSS, like_params=(CORR,), t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=seed,
                           moves=MIX)
    d = draws(N, D, S, seed, MIX)
    assert set(d[2].tolist()) == {STRETCH, DE}, 'the seed must give a step of each kind'
    hz, hl, z0n = h['hist_z'].cpu().numpy(), h['hist_lp'].cpu().numpy(), z0.cpu().numpy()
    records, ok = replay(hz, hl, z0n, d, spline_lp(o, sd, mu))

    def lp_close(a, b):
        assert rel(a, b) < LP_TOL, rel(a, b)

    seen = check_replay(hz, hl, z0n, records, ok, lp_close)
    print('%d of %d half-steps compared, moves seen %s' % (ok, len(records), sorted(seen)))
    assert DE in seen


def test_chunking_is_bit_exact():
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import ensemble_rounds
    D, N, S, seed = 20, 80, 8, 42
    nvp = flow.HipNVP(D, 16, 3, 1, seed=8)
    sd, mu = affine(D, 8)
    z0 = start(D, N, 8)
    kw = dict(t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,), moves=MIX)
    assert set(move_ids_by_the_rule(seed, S, MIX).tolist()) == {STRETCH, DE}
    one = nvp.ensemble_steps(GAUSS, z0, S, **kw)
    z, lp, parts = z0, None, []
    for s0, k in ((0, 3), (3, 5)):
        r = nvp.ensemble_steps(GAUSS, z, k, lp=lp, step0=s0, **kw)
        z, lp = r['z'], r['lp']
        parts.append(r)
    for key in ('hist_z', 'hist_x', 'hist_lp'):
        assert torch.equal(torch.cat([p[key] for p in parts], 1), one[key]), key
    assert torch.equal(sum(p['n_accept'] for p in parts), one['n_accept'])
    # the round route likewise
    st1, rone = ensemble_rounds(nvp, z0, S, like_id=GAUSS, **kw)
    st, rparts, acc = None, [], []
    for s0, k in ((0, 3), (3, 5)):
        st, h = ensemble_rounds(nvp, z0, k, state=st, like_id=GAUSS, step0=s0, **kw)
        rparts.append(h)
    for key in ('hist_z', 'hist_x', 'hist_lp'):
        assert torch.equal(torch.cat([p[key] for p in rparts], 1), rone[key]), key
    assert torch.equal(st.n_accept, st1.n_accept)


def test_the_stretch_move_is_unchanged():
    """the new entries with weight on the stretch move alone, and with NULL, are the old entries bit for bit"""
    from nnest_amd import _lib, flow
    from nnest_amd.ensemble_rounds import ensemble_rounds
    D, N, S, seed = 20, 80, 6, 5
    lib = _lib.load()
    nvp = flow.HipNVP(D, 16, 3, 1, seed=9)
    sd, mu = affine(D, 9)
    z0 = start(D, N, 9)
    kw = dict(t_std=sd, t_mean=mu, seed=seed, like_params=(CORR,), lo=-np.ones(D), hi=np.ones(D))
    old = nvp.ensemble_steps(GAUSS, z0, S, **kw)
    new = nvp.ensemble_steps(GAUSS, z0, S, moves={'stretch': 1}, **kw)
    nvp._sym['ensemble'] = lambda *a: lib.nnest_ensemble_moves_steps(*a, None)   # the new entry with NULL
    null = nvp.ensemble_steps(GAUSS, z0, S, **kw)
    for key in ('z', 'x', 'lp', 'hist_z', 'hist_x', 'hist_lp', 'n_accept'):
        assert torch.equal(new[key], old[key]) and torch.equal(null[key], old[key]), key
    assert nvp.ensemble_max_walkers(GAUSS, moves={'stretch': 1}) == lib.nnest_ensemble_max_walkers(nvp._h, GAUSS)
    # x space
    xkw = dict(seed=seed, like_params=(CORR,))
    xold = flow.ensemble_x_steps(GAUSS, z0, S, **xkw)
    xnew = flow.ensemble_x_steps(GAUSS, z0, S, moves={'Stretch': 2.0}, **xkw)
    for key in ('x', 'tx', 'lp', 'hist_x', 'hist_lp', 'n_accept'):
        assert torch.equal(xnew[key], xold[key]), key
    # rounds
    _, rold = ensemble_rounds(nvp, z0, S, like_id=GAUSS, **kw)
    _, rnew = ensemble_rounds(nvp, z0, S, like_id=GAUSS, moves={'stretch': 1}, **kw)
    for key in ('hist_z', 'hist_x', 'hist_lp'):
        assert torch.equal(rnew[key], rold[key]), key


def restatement_moves_enough(D, N, S, moves, lp_fn, z0, seed):
    """the condition on S, met on the CPU first: the numpy restatement at the same D, N, weights, start and flow (the checker's
    inverse on the flow's weights; numpy draws) moves MOVED of its walkers"""
    rng = np.random.RandomState(seed)
    p = moves.get('stretch', 0.0) / (moves.get('stretch', 0.0) + moves.get('de', 0.0))
    _, _, moved = moves_run(z0, lp_fn(z0), numpy_moves_draws(rng, N, S, D, p), lp_fn)
    return moved.mean()


def moved_fraction(start_rows, hist):
    return float(np.mean(np.any(hist != start_rows[:, None, :], axis=(1, 2))))


@pytest.mark.parametrize('moves', [DE_ONLY, MIX], ids=['de', 'mix'])
def test_invariance_unconstrained_fused(moves):
    """walkers started from exact draws of N(0, Sigma) in the box, seen through T and a random NVP, stay exact"""
    from nnest_amd import flow
    from oracle import oracle as orc
    D, N, S = 5, 2000, 20
    nvp = flow.HipNVP(D, 16, 3, 1, seed=21)
    assert nvp.ensemble_max_walkers(GAUSS, moves=moves) >= N
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(21)
    tx0 = exact_gauss_box(rng, N, D)
    z0, _ = nvp.forward(((tx0 - mu) / sd).astype(np.float32))
    frac_cpu = restatement_moves_enough(D, N, S, moves, oracle_lp(orc.NVP(D, 16, 3, 1, nvp.store_packed()), sd, mu), z0.cpu().numpy(), 1)
    assert frac_cpu >= MOVED, frac_cpu
    res = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=5, like_params=(CORR,), moves=moves)
    tx = res['x'].cpu().numpy() * sd + mu
    frac = moved_fraction(z0.cpu().numpy(), res['hist_z'].cpu().numpy())
    print('%s: acceptance %.3f, moved %.3f (restatement %.3f)' % (moves, int(res['n_accept'].sum()) / (N * S), frac, frac_cpu))
    assert frac >= MOVED
    assert_invariant(stationarity_pvalues(tx, exact_gauss_box(rng, N, D)), what='ensemble moves %s, fused, unconstrained' % moves)


@pytest.mark.parametrize('moves', [DE_ONLY, MIX], ids=['de', 'mix'])
@pytest.mark.parametrize('route', ['fused', 'rounds_spline'])
def test_invariance_constrained(route, moves):
    """with loglstar the target is uniform on {logL > L*} in the box.  S: 15 as tests/test_gpu_ensemble.py through the NVP; through
    the spline flow (ActNorm set from the start points: another latent geometry, where the DE move alone is accepted less often) 15
    steps leave more than a tenth of the walkers where they started, so that run takes 40"""
    from nnest_amd import flow
    from nnest_amd.ensemble_rounds import ensemble_rounds
    from nnest_amd.spline import HipSpline
    from oracle import oracle as orc
    from tests.test_gpu_spline_ensemble import oracle_lp as spline_lp
    D, N, S = 5, 2000, 15 if route == 'fused' else 40
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
        lp_cpu = oracle_lp(orc.NVP(D, 16, 3, 1, nvp.store_packed()), sd, mu, loglstar=star)
        frac_cpu = restatement_moves_enough(D, N, S, moves, lp_cpu, z0.cpu().numpy(), 2)
        assert frac_cpu >= MOVED, frac_cpu
        res = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, loglstar=star, seed=9, like_params=(CORR,), moves=moves, **box)
        x, nacc, hz = res['x'], res['n_accept'], res['hist_z']
    else:
        sp = HipSpline(D, 16, 3, seed=31)
        z0, _ = sp.forward(x0)   # (the first forward sets the ActNorm layers from these points)
        lp_cpu = spline_lp(orc.Spline(D, 16, 3, 8, 3.0, sp.store_packed(), sp.P), sd, mu, loglstar=star)
        frac_cpu = restatement_moves_enough(D, N, S, moves, lp_cpu, z0.cpu().numpy(), 2)
        assert frac_cpu >= MOVED, frac_cpu
        st, h = ensemble_rounds(sp, z0, S, like_id=GAUSS, like_params=(CORR,), t_std=sd, t_mean=mu, loglstar=star, seed=9, moves=moves, **box)
        x, nacc, hz = st.x, st.n_accept, h['hist_z']
    tx = x.cpu().numpy() * sd + mu
    assert np.all(inside(tx)) and np.all(in_unit_box(tx))
    frac = moved_fraction(z0.cpu().numpy(), hz.cpu().numpy())
    print('%s %s: acceptance %.3f, moved %.3f (restatement %.3f)' % (route, moves, int(nacc.sum()) / (N * S), frac, frac_cpu))
    assert frac >= MOVED
    assert_invariant(stationarity_pvalues(tx, uniform_on(rng, N, D, inside)), what='ensemble moves %s, %s, constrained' % (moves, route))


def test_residency_refusal_routes_to_rounds(tmp_path):
    import nnest_amd
    from nnest_amd import _lib
    from nnest_amd.likelihoods import Gaussian
    D = 4
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), log_dir=str(tmp_path), log_level=30, flow='nvp')
    nvp = s.trainer.netG
    cap = nvp.ensemble_max_walkers(GAUSS, moves=MIX)
    assert cap >= 512 and cap % 4 == 0 and cap <= nvp.ensemble_max_walkers(GAUSS)
    with pytest.raises(_lib.NnestHipError) as e:
        nvp.ensemble_steps(GAUSS, start(D, cap + 4, 1), 2, like_params=(CORR,), moves=MIX)
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    out = s._ensemble_sample(2, cap + 4, seed=3, moves=MIX)
    assert s.ensemble_route == 'rounds' and out[0].shape == (cap + 4, 2, D)
    s._ensemble_sample(2, 64, seed=3, moves=MIX)
    assert s.ensemble_route == 'fused'


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_front_end(tmp_path, flow_name):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, N, S = 3, 32, 12
    rng = np.random.RandomState(2)
    np.random.seed(2)
    torch.manual_seed(2)
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.trainer.train = lambda samples, jitter=0.0, **kw: None   # (keep the test short: the flow stays at its initialisation)
    s.run(S, N, _train(rng, D), moves={'stretch': .5, 'de': .5})
    assert s.samples.shape == (N, S, D) and s.latent_samples.shape == (N, S, D) and s.loglikes.shape == (N, S)
    assert s.ensemble_route == ('fused' if flow_name == 'nvp' else 'rounds')
    assert np.all(np.isfinite(s.samples)) and np.all(np.isfinite(s.loglikes))
    assert 0 < s.total_accepted < N * S
    if flow_name == 'spline':
        with pytest.raises(ValueError, match='fused route'):
            s.run(S, N, _train(rng, D), moves={'stretch': .5, 'de': .5}, route='fused')
    with pytest.raises(NotImplementedError, match='snooker'):
        s.run(S, N, _train(rng, D), moves={'snooker': 1.0})


def test_bootstrap_takes_latent_moves(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, N, S = 4, 64, 4000   # (tests/test_gpu_bootstrap.py BOOT_STEPS: the x-space run must be 50 autocorrelation times long)
    np.random.seed(11)
    torch.manual_seed(11)
    s = nnest_amd.EnsembleSampler(D, Gaussian(D, CORR), prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30, flow='nvp')
    s.trainer.train = lambda samples, jitter=0.0, **kw: None
    seen = []
    run_z = s._ensemble_sample
    s._ensemble_sample = lambda *a, **kw: (run_z(*a, **kw), seen.append((s.ensemble_route, kw.get('moves'))))[0]
    out = s.bootstrap(S, N, iters=1, thin=10, seed=11, latent_moves={'de': 1.0})
    assert len(seen) == 1 and seen[0][0] == 'fused' and seen[0][1].w_de == 1.0 and seen[0][1].w_stretch == 0.0
    assert out.ndim == 2 and out.shape[1] == D and len(out) > 0 and np.all(np.isfinite(out))
    assert s.samples.shape == (N, S, D) and np.all(np.isfinite(s.samples)) and np.all(np.isfinite(s.loglikes))
