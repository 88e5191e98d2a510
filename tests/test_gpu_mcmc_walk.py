"""GPU checks of the fused random-walk Metropolis run (include/nnest_hip.h nnest_mcmc_steps, nnest_spline_mcmc_steps,
nnest_mcmc_fill_noise; HipNVP.mcmc_steps, HipSpline.mcmc_steps, Sampler._mcmc_sample_device, MCMCSampler.run(route='fused')): both
kernels against the numpy restatement (tests/mcmc_walk_check.py) on their exported draws, step by step from the kernel's own
previous row; a run cut into launches or into shards is the same run, bit for bit; steps = 0 evaluates the start; exactly sampled
targets stay exact; the front end.

Tolerances.  lp, logL and x of the kernels against the float32 oracle inverse + float64 likelihood:
  NVP, x_dim <= 50: rtol 1e-6, atol 2e-5 on lp and logL (tests/test_gpu_ensemble.py's figure for this evaluator), 5e-5 on x (the figure
    of the kernels' inverse against the oracle's: __graft_entry__.smoke, tests/test_gpu_nested.py);
  NVP, x_dim 70 and 100 (weights in LDS): no recorded figure, so the test measures the error of the existing nnest_ensemble_steps --
    the same evaluator in another kernel -- against the same restatement at that width and allows twice that (DESIGN.md 3.10 has
    the measured values);
  spline: 3e-5 in |a - b| / (1 + |b|) (tests/test_gpu_spline_ensemble.py's figure for that evaluator).
A decision is compared unless |lp(q) - lp(z) - log u| < m, m = ten times the lp tolerance in force: log u has density <= 1, so the
expected share of such decisions is at most 2 m; at most 1 % may be excluded (NVP: 2 m < 0.3 % whatever the seed; spline: see
SPLINE_SEEDS)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.mcmc_walk_check import latent_target, rw_step
from tests.slice_invariance import assert_invariant, stationarity_pvalues

pytestmark = pytest.mark.gpu

GAUSS = 3   # NNEST_LIKE_GAUSSIAN: N(0, Sigma), Sigma = I + corr (11^T - I)
CORR = 0.5
BOX = 2.5   # the replay tests' prior box on T(x): some starts and some proposals fall outside (chosen on the CPU with the restatement)
SPL_TOL = 3e-5


def affine(D, seed):
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)


def in_box(tx, half):
    return np.all(np.abs(np.asarray(tx, np.float64)) <= half, axis=1)


class Restated(object):
    """the target in the kernels' arithmetic: the oracle's inverse (float32), T in float32, the float64-moment Gaussian"""

    def __init__(self, o, sd, mu, half):
        self.o, self.sd, self.mu, self.half = o, sd, mu, half
        self.lp = latent_target(self.x_of_z, self.logl, lambda x: in_box(self.T(x), half))

    def T(self, x):
        return (np.asarray(x, np.float32) * self.sd) + self.mu

    def x_of_z(self, q):
        return self.o.inverse(np.asarray(q, np.float32))

    def logl(self, x):
        from oracle import oracle as orc
        return orc.loglike('gaussian', self.T(x), 1.0, params=[CORR])


def err(a, b, tol):
    """max over the entries of (|a - b| - tol(b)); the non-finite entries (lp = -inf outside the box) must be equal"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin]), 'non-finite entries differ'
    return float(np.max(np.abs(a[fin] - b[fin]) - tol(b[fin]))) if fin.any() else -1.0


def check_replay(net, rs, z0, S, step, seed, offset, tol, x_tol, what):
    """every step replayed from the kernel's own previous row.  tol(v), x_tol(v): the tolerance on lp / logL and on x at value v"""
    from nnest_amd import flow
    C, D = z0.shape
    kw = dict(t_std=rs.sd, t_mean=rs.mu, lo=-np.full(D, rs.half), hi=np.full(D, rs.half), seed=seed, walker_offset=offset,
              like_params=(CORR,))
    begin = net.mcmc_steps(GAUSS, z0, 0, step, **kw)
    res = net.mcmc_steps(GAUSS, z0, S, step, **kw)
    eps, u = (t.cpu().numpy() for t in flow.mcmc_fill_noise(S, C, D, seed=seed, walker_offset=offset))
    z0n = z0.cpu().numpy()
    hz, hx, hl = (res[k].cpu().numpy() for k in ('hist_z', 'hist_x', 'hist_logl'))
    # the start: lp, logL and x of z0
    x0o, _ = rs.x_of_z(z0n)
    worst_lp = err(begin['lp'].cpu().numpy(), rs.lp(z0n), tol)
    worst_ll = err(begin['logl'].cpu().numpy(), rs.logl(x0o), tol)
    worst_x = err(begin['x'].cpu().numpy(), x0o, x_tol)
    excluded, n_moved = 0, np.zeros(C, np.int64)
    for i in range(S):
        z_prev = z0n if i == 0 else hz[:, i - 1]
        x_prev = begin['x'].cpu().numpy() if i == 0 else hx[:, i - 1]
        l_prev = begin['logl'].cpu().numpy() if i == 0 else hl[:, i - 1]
        lp_prev = rs.lp(z_prev)
        rec = {}
        rw_step(z_prev, lp_prev, eps[i], u[i], step, rs.lp, record=rec)
        moved = np.any(hz[:, i] != z_prev, axis=1)
        with np.errstate(invalid='ignore'):
            m = 10.0 * tol(np.maximum(np.abs(np.where(np.isfinite(rec['lp_q']), rec['lp_q'], 0.0)),
                                      np.abs(np.where(np.isfinite(lp_prev), lp_prev, 0.0))))
            border = np.abs(rec['margin']) < m   # (a NaN margin -- from -inf to -inf -- is no borderline case: both refuse)
        excluded += int(border.sum())
        assert np.array_equal(moved[~border], rec['accept'][~border]), '%s step %d: decisions differ' % (what, i)
        # moved rows: the proposal, bit for bit; x and logL against the restatement
        assert np.array_equal(hz[moved, i].view(np.uint32), rec['q'][moved].view(np.uint32)), '%s step %d: proposals not bit-equal' % (what, i)
        xq, _ = rs.x_of_z(rec['q'][moved])
        if moved.any():
            worst_x = max(worst_x, err(hx[moved, i], xq, x_tol))
            worst_ll = max(worst_ll, err(hl[moved, i], rs.logl(xq), tol))
        # unmoved rows: the previous row, bit for bit
        for name, now, prev in (('z', hz[:, i], z_prev), ('x', hx[:, i], x_prev)):
            assert np.array_equal(now[~moved].view(np.uint32), prev[~moved].view(np.uint32)), '%s step %d: unmoved %s changed' % (what, i, name)
        assert np.array_equal(hl[~moved, i].view(np.uint64), l_prev[~moved].view(np.uint64)), '%s step %d: unmoved logL changed' % (what, i)
        n_moved += moved
    # the ends are the last history row; lp of the ends against the restatement
    for key, h in (('z', hz), ('x', hx), ('logl', hl)):
        np.testing.assert_array_equal(res[key].cpu().numpy(), h[:, -1])
    np.testing.assert_array_equal(res['n_accept'].cpu().numpy(), n_moved)
    worst_lp = max(worst_lp, err(res['lp'].cpu().numpy(), rs.lp(hz[:, -1]), tol))
    print('%s: %d of %d decisions excluded; lp %+.3g, logL %+.3g, x %+.3g over the tolerance (negative: inside); moved %d of %d'
          % (what, excluded, C * S, worst_lp, worst_ll, worst_x, int(n_moved.sum()), C * S))
    assert excluded <= 0.01 * C * S
    assert worst_lp <= 0.0 and worst_ll <= 0.0 and worst_x <= 0.0
    assert 0 < n_moved.sum() < C * S


@pytest.mark.parametrize('D,offset', [(5, 0), (50, 1000), (70, 0), (100, 0)])
def test_nvp_kernel_replays_on_its_draws(D, offset):
    from nnest_amd import flow
    from oracle import oracle as orc
    C, S, seed = 70, 6, 4000 + D
    nvp = flow.HipNVP(D, 16, 3, 1, seed=D)
    sd, mu = affine(D, D)
    rs = Restated(orc.NVP(D, 16, 3, 1, nvp.store_packed()), sd, mu, BOX)
    z0 = torch.from_numpy(np.random.RandomState(D).normal(size=(C, D)).astype(np.float32) * 0.5).cuda()
    if D <= 50:
        tol, x_tol = (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    else:
        # the evaluator's error in the existing ensemble kernel at this width, against the same restatement: twice that is allowed
        ens = nvp.ensemble_steps(GAUSS, z0, S, t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=seed, like_params=(CORR,))
        ez, ex = (ens[k].cpu().numpy().reshape(C * S, D) for k in ('hist_z', 'hist_x'))
        elp = ens['hist_lp'].cpu().numpy().reshape(C * S)
        e_lp = err(elp, rs.lp(ez), lambda v: 0.0 * v)
        e_x = float(np.max(np.abs(ex - rs.x_of_z(ez)[0])))
        print('x_dim %d: nnest_ensemble_steps against the restatement: lp %.3g, x %.3g' % (D, e_lp, e_x))
        assert e_lp > 0.0 and e_x > 0.0
        tol, x_tol = (lambda v: 2.0 * e_lp + 0.0 * v), (lambda v: 2.0 * e_x + 0.0 * v)
    check_replay(nvp, rs, z0, S, 1.0 / np.sqrt(D), seed, offset, tol, x_tol, 'nvp x_dim %d' % D)


def test_exported_draws_are_the_defined_streams():
    """nnest_mcmc_fill_noise against the definition restated in numpy (mcmc_walk_check.mcmc_draws): the uniforms bit for bit; the
    normals to 1e-3 -- a check of the counter layout (a wrong block, word or stream is off by O(1)), not of the hardware's log, sin
    and cos, which are build-defined.  A walker index beyond 2^32, a step offset, a width that is no multiple of 4; either output
    alone"""
    from nnest_amd import _lib, flow
    from tests.mcmc_walk_check import mcmc_draws
    for D, C, S, seed, step0, off in ((7, 33, 3, 99, 7, (3 << 32) + 5), (50, 70, 2, (5 << 40) + 1, 0, 1000), (1, 5, 2, 3, 0, 0)):
        eps, u = flow.mcmc_fill_noise(S, C, D, seed=seed, step0=step0, walker_offset=off)
        eps_r, u_r = mcmc_draws(seed, off, C, step0, S, D)
        assert np.array_equal(u.cpu().numpy().view(np.uint32), u_r.view(np.uint32))
        np.testing.assert_allclose(eps.cpu().numpy(), eps_r, rtol=0, atol=1e-3)
        assert abs(float(eps.mean())) < 5.0 / np.sqrt(eps.numel()) + 0.05 and np.all(u_r < 1.0)
    lib, dev = _lib.load(), eps.device
    only_u, only_e = torch.empty_like(u), torch.empty_like(eps)
    with torch.cuda.device(dev):
        _lib.check(lib.nnest_mcmc_fill_noise(None, _lib.ptr(only_u), S, C, D, step0, seed, off, _lib.current_stream(dev)))
        _lib.check(lib.nnest_mcmc_fill_noise(_lib.ptr(only_e), None, S, C, D, step0, seed, off, _lib.current_stream(dev)))
    assert torch.equal(only_u, u) and torch.equal(only_e, eps)


def spline_and_start(D, N, seed):
    """a HipSpline at its random initialisation with the ActNorm layers set from the start points (its first forward), the oracle on
    the same weights, and the walkers' start z0 = f(x0)"""
    from nnest_amd.spline import HipSpline
    from oracle import oracle as orc
    sp = HipSpline(D, 16, 3, seed=seed)
    x0 = np.random.RandomState(seed).normal(size=(N, D)).astype(np.float32) * 0.5
    z0, _ = sp.forward(x0)
    return sp, orc.Spline(D, 16, 3, 8, 3.0, sp.store_packed(), sp.P), z0.contiguous()


# (the spline's relative tolerance makes m about 0.02 at x_dim 40, where |lp| is about 70: up to 4 % of the decisions would fall within
# it.  The seeds were picked on the CPU, as the first of 5000 + x_dim, ... for which the restatement alone -- mcmc_walk_check.mcmc_draws
# and rw_step through the oracle's spline on the same initialisation -- has no decision within m, nor close to it)
SPLINE_SEEDS = {5: 5005, 40: 5050}


@pytest.mark.parametrize('D', [5, 40])
def test_spline_kernel_replays_on_its_draws(D):
    C, S, seed = 40, 4, SPLINE_SEEDS[D]
    sp, o, z0 = spline_and_start(D, C, D)
    sd, mu = affine(D, D)
    rs = Restated(o, sd, mu, BOX)
    check_replay(sp, rs, z0, S, 1.0 / np.sqrt(D), seed, 0, lambda v: SPL_TOL * (1.0 + np.abs(v)), lambda v: SPL_TOL * (1.0 + np.abs(v)),
                 'spline x_dim %d' % D)


def _flow_and_start(name, D, C, seed):
    from nnest_amd import flow
    if name == 'nvp':
        return flow.HipNVP(D, 16, 3, 1, seed=seed), torch.from_numpy(np.random.RandomState(seed).normal(size=(C, D)).astype(np.float32) * 0.5).cuda()
    sp, _, z0 = spline_and_start(D, C, seed)
    return sp, z0


HIST = ('hist_z', 'hist_x', 'hist_logl')
ENDS = ('z', 'x', 'lp', 'logl')


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_chunking_is_bit_exact(name):
    D, C = 20, 70
    net, z0 = _flow_and_start(name, D, C, 8)
    sd, mu = affine(D, 8)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=42, like_params=(CORR,))
    one = net.mcmc_steps(GAUSS, z0, 7, 0.2, **kw)
    a = net.mcmc_steps(GAUSS, z0, 3, 0.2, **kw)
    b = net.mcmc_steps(GAUSS, a['z'], 4, 0.2, lp=a['lp'], logl=a['logl'], step0=3, **kw)
    for key in HIST:
        assert torch.equal(torch.cat([a[key], b[key]], 1), one[key]), key
    for key in ENDS:
        assert torch.equal(b[key], one[key]), key
    assert torch.equal(a['n_accept'] + b['n_accept'], one['n_accept'])
    assert 0 < int(one['n_accept'].sum()) < 7 * C
    # the ends alone (no history) are the same run
    bare = net.mcmc_steps(GAUSS, z0, 7, 0.2, history=False, **kw)
    assert bare['hist_z'] is None
    for key in ENDS + ('n_accept',):
        assert torch.equal(bare[key], one[key]), key


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_a_shard_is_the_same_run(name):
    D, C, S = 20, 70, 5
    net, z0 = _flow_and_start(name, D, C, 9)
    sd, mu = affine(D, 9)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=43, like_params=(CORR,))
    full = net.mcmc_steps(GAUSS, z0, S, 0.2, **kw)
    part = net.mcmc_steps(GAUSS, z0[24:].contiguous(), S, 0.2, walker_offset=24, **kw)
    for key in HIST + ENDS + ('n_accept',):
        assert torch.equal(part[key], full[key][24:]), key
    other = net.mcmc_steps(GAUSS, z0[24:].contiguous(), S, 0.2, **kw)   # (without the offset the shard draws walker 0's stream)
    assert not torch.equal(other['hist_z'], part['hist_z'])


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_zero_steps_evaluates_the_start_and_writes_nothing_else(name):
    from nnest_amd import _lib
    from oracle import oracle as orc
    D, C = 6, 21
    net, z0 = _flow_and_start(name, D, C, 10)
    sd, mu = affine(D, 10)
    out = net.mcmc_steps(GAUSS, z0, 0, 0.3, t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), like_params=(CORR,))
    assert out['hist_z'] is None and torch.equal(out['z'], z0) and int(out['n_accept'].sum()) == 0
    o = orc.NVP(D, 16, 3, 1, net.store_packed()) if name == 'nvp' else orc.Spline(D, 16, 3, 8, 3.0, net.store_packed(), net.P)
    rs = Restated(o, sd, mu, BOX)
    tol = (lambda v: 2e-5 + 1e-6 * np.abs(v)) if name == 'nvp' else (lambda v: SPL_TOL * (1.0 + np.abs(v)))
    xo, _ = rs.x_of_z(z0.cpu().numpy())
    assert err(out['lp'].cpu().numpy(), rs.lp(z0.cpu().numpy()), tol) <= 0.0
    assert err(out['logl'].cpu().numpy(), rs.logl(xo), tol) <= 0.0
    assert np.max(np.abs(out['x'].cpu().numpy() - xo)) <= 5e-5
    # through the C entry with every optional buffer given: z_out and n_accept keep their contents; T = identity and no prior as NULLs
    dev = z0.device
    z_out = torch.full((C, D), 123.0, device=dev)
    n_acc = torch.full((C,), -7, dtype=torch.int32, device=dev)
    x_out = torch.empty(C, D, device=dev)
    lp_out, ll_out = torch.empty(C, dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)
    lk = _lib.like_spec(GAUSS, 1.0, (CORR,))
    with torch.cuda.device(dev):
        _lib.check(net._sym['mcmc'](net._h, ctypes.byref(lk), None, None, None, None, _lib.ptr(z0), None, None, _lib.ptr(z_out),
                                    _lib.ptr(x_out), _lib.ptr(lp_out), _lib.ptr(ll_out), None, None, None, _lib.ptr(n_acc), C, 0,
                                    ctypes.c_float(0.3), 0, 0, 0, _lib.current_stream(dev)))
    torch.cuda.synchronize()
    assert bool((z_out == 123.0).all()) and bool((n_acc == -7).all())
    ident = Restated(o, np.ones(D, np.float32), np.zeros(D, np.float32), np.inf)
    assert err(lp_out.cpu().numpy(), ident.lp(z0.cpu().numpy()), tol) <= 0.0
    assert np.max(np.abs(x_out.cpu().numpy() - xo)) <= 5e-5
    assert torch.equal(x_out, out['x'])


def exact_gauss_box(rng, n, D):
    cov = (1 - CORR) * np.eye(D) + CORR * np.ones((D, D))
    out, have = [], 0
    while have < n:
        x = rng.multivariate_normal(np.zeros(D), cov, size=8 * n)
        x = x[in_box(x, 1.0)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_invariance(name):
    """walkers started from exact draws of N(0, Sigma) in the box, seen through T and a random flow, stay exact (the set-up of
    tests/test_gpu_ensemble.py test_invariance_unconstrained_fused).  The step, 0.45, was chosen on the CPU with the restatement
    through the oracle's NVP: acceptance 0.47, every walker moved"""
    from nnest_amd import flow
    from nnest_amd.spline import HipSpline
    D, N, S = 5, 2000, 20
    net = flow.HipNVP(D, 16, 3, 1, seed=21) if name == 'nvp' else HipSpline(D, 16, 3, seed=21)
    sd, mu = affine(D, 21)
    rng = np.random.RandomState(21)
    tx0 = exact_gauss_box(rng, N, D)
    z0, _ = net.forward(((tx0 - mu) / sd).astype(np.float32))   # (the spline's first forward sets the ActNorm layers from these points)
    res = net.mcmc_steps(GAUSS, z0, S, 0.45, t_std=sd, t_mean=mu, lo=-np.ones(D), hi=np.ones(D), seed=5, like_params=(CORR,), history=False)
    tx = res['x'].cpu().numpy() * sd + mu
    assert np.all(in_box(tx, 1.0))
    assert float((res['n_accept'] > 0).float().mean()) >= 0.9
    assert_invariant(stationarity_pvalues(tx, exact_gauss_box(rng, N, D)), what='random-walk Metropolis, fused, %s' % name)


# ---- the front end ----------------------------------------------------------------------------------------------------------
COV = np.array([[1.0, 0.8], [0.8, 1.0]])


def _train(seed=0, n=2000):
    return np.random.RandomState(seed).multivariate_normal([0.0, 0.0], COV, size=n)


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_front_end(tmp_path, flow_name):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    train = _train()
    like = Gaussian(2, 0.8)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(2, like, log_dir=str(tmp_path), log_level=30, flow=flow_name)
    init = (train[:50] - train.mean(0)) / train.std(0)
    s.run(400, 50, train, init_samples=init, route='fused', seed=1)
    assert s.mcmc_route == 'fused'
    assert s.samples.shape == (50, 401, 2) and s.loglikes.shape == (50, 401) and s.latent_samples.shape == (50, 401, 2)
    assert s.total_calls == 50 * 401
    assert s.total_accepted + s.total_rejected == 50 * 400 and 0 < s.total_accepted < 50 * 400
    np.testing.assert_allclose(s.loglikes.reshape(-1), like(s.samples.reshape(-1, 2)), rtol=1e-5, atol=1e-4)
    flat = s.samples[:, 100:, :].reshape(-1, 2)
    assert np.all(np.abs(flat.mean(0)) < 0.25)
    c = np.cov(flat.T)
    assert abs(c[0, 0] - 1) < 0.3 and abs(c[1, 1] - 1) < 0.3 and abs(c[0, 1] - 0.8) < 0.3
    # the same seed gives the same chains (the flow as trained: the second run does not train again)
    first = s.samples.copy()
    s.trainer.train = lambda samples, jitter=0.0, **kw: None
    s.run(400, 50, train, init_samples=init, route='fused', seed=1)
    np.testing.assert_array_equal(s.samples, first)
    s.run(40, 50, train, init_samples=init, route='fused', seed=2)
    assert not np.array_equal(s.samples, first[:, :41])
    # without init_samples the run starts from the flow's base
    s.total_calls = 0
    s.run(20, 30, train, route='fused', seed=3)
    assert s.samples.shape == (30, 21, 2) and np.all(np.isfinite(s.loglikes)) and np.all(np.isfinite(s.latent_samples))
    assert s.total_calls % 30 == 0 and s.total_calls >= 30 * 21
    # route=None keeps the host step loop
    s.run(3, 8, train, init_samples=init[:8])
    assert s.mcmc_route == 'host' and s.samples.shape == (8, 4, 2)


def test_front_end_start_search_gives_up(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    s = nnest_amd.MCMCSampler(2, Gaussian(2, 0.8), prior=UniformPrior(2, 50.0, 51.0), log_dir=str(tmp_path), log_level=30, flow='nvp')
    s._install_transform(np.zeros(2), np.ones(2))
    calls = s.total_calls
    with pytest.raises(Exception, match='Could not find starting value'):
        s._mcmc_sample_device(5, num_chains=16, max_start_tries=3, seed=1)
    assert s.total_calls == calls
    # (a box the base does reach is taken)
    s2 = nnest_amd.MCMCSampler(2, Gaussian(2, 0.8), prior=UniformPrior(2, -50.0, 50.0), log_dir=str(tmp_path), log_level=30, flow='nvp')
    s2._install_transform(np.zeros(2), np.ones(2))
    out = s2._mcmc_sample_device(5, num_chains=16, max_start_tries=3, seed=1)
    assert out[0].shape == (16, 6, 2) and np.all(np.abs(out[0]) <= 50.0)


def test_front_end_refusals(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    train = _train()
    python_like = lambda x: -0.5 * (x * x).sum(1)
    derived_like = lambda x: (-0.5 * (x * x).sum(1), x[:, :1])
    for kw, like, word in ((dict(flow='nvp'), python_like, 'Python callable'),
                           (dict(flow='nvp', num_derived=1), derived_like, 'derived'),
                           (dict(flow='maf'), Gaussian(2, 0.8), 'HipMAF')):
        s = nnest_amd.MCMCSampler(2, like, log_dir=str(tmp_path), log_level=30, **kw)
        s.trainer.train = lambda samples, jitter=0.0, **k: pytest.fail('refused before training')
        with pytest.raises(ValueError, match=word):
            s.run(5, 8, train, route='fused')
    with pytest.raises(ValueError, match='route'):
        s.run(5, 8, train, route='rounds')
