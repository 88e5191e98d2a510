"""GPU checks of the importance-sampled evidence (include/nnest_hip.h nnest_importance_evidence, nnest_spline_importance_evidence,
nnest_importance_fill_noise, nnest_importance_groups; HipNVP / HipSpline.importance_evidence, Sampler.importance_evidence): the
exported draws against the restated stream; both kernels against the numpy restatement (tests/importance_check.py) on their own
draws, over more than two passes of the persistent loop and a ragged tail; the reduction against float64 sums of the kernel's own
log weights; small launches and a guard row; a run cut into launches is the same run; a target with a known evidence; the front end.

Tolerances.  x, logL and logw of the kernels against the float32 oracle inverse + float64 likelihood, the figures in force for this
evaluator (tests/test_gpu_mcmc_walk.py):
  NVP, x_dim <= 50: 2e-5 + 1e-6 |v| on logL and logw, 5e-5 on x;
  NVP, x_dim 70 and 100 (weights in LDS): the test measures nnest_mcmc_steps(steps = 0) -- the same evaluator in another kernel --
    against the same restatement on the same points and allows twice that, each quantity by its own measured error: lp's for logw,
    logL's for logL, x's for x (DESIGN.md 3.11 has the measured values);
  spline: 3e-5 (1 + |v|).
Live / dead is compared unless the verdict hangs on a coordinate of T(x) within ten times the x tolerance of a face of the box (no
coordinate is outside by more than that, and one is within it of a face); at most 1 % of M may be excluded."""
import ctypes

import numpy as np
import pytest
import torch

from tests import importance_check as ic

pytestmark = pytest.mark.gpu

GAUSS = 3   # NNEST_LIKE_GAUSSIAN
CORR = 0.5
BOX = 2.5
SPL_TOL = 3e-5


def affine(D, seed):
    r = np.random.RandomState(seed)
    return r.uniform(0.5, 1.5, D).astype(np.float32), r.uniform(-0.3, 0.3, D).astype(np.float32)


class Restated(object):
    """the target in the kernels' arithmetic: the oracle's inverse (float32), T in float32, the float64-moment Gaussian"""

    def __init__(self, o, sd, mu, half):
        self.o, self.sd, self.mu, self.half = o, sd, mu, half
        self.lp = ic.latent_target(self.x_of_z, self.logl, self.in_box)

    def T(self, x):
        return (np.asarray(x, np.float32) * self.sd) + self.mu

    def in_box(self, x):
        return np.all(np.abs(self.T(x).astype(np.float64)) <= self.half, axis=1)

    def x_of_z(self, q):
        return self.o.inverse(np.asarray(q, np.float32))

    def logl(self, x):
        from oracle import oracle as orc
        return orc.loglike('gaussian', self.T(x), 1.0, params=[CORR])


def groups_of(M, tile):
    from nnest_amd import _lib
    return int(_lib.load().nnest_importance_groups(int(M), tile))


def sums_of(res):
    return tuple(float(v) for v in res['sums'].cpu().numpy())


def nvp_and_oracle(D, seed):
    from nnest_amd import flow
    from oracle import oracle as orc
    nvp = flow.HipNVP(D, 16, 3, 1, seed=seed)
    return nvp, orc.NVP(D, 16, 3, 1, nvp.store_packed())


def spline_and_oracle(D, seed, N=40):
    """a HipSpline as tests/test_gpu_mcmc_walk.spline_and_start builds it: the random initialisation with the ActNorm layers set from
    start points (its first forward), and the oracle on the same weights"""
    from nnest_amd.spline import HipSpline
    from oracle import oracle as orc
    sp = HipSpline(D, 16, 3, seed=seed)
    sp.forward(np.random.RandomState(seed).normal(size=(N, D)).astype(np.float32) * 0.5)
    return sp, orc.Spline(D, 16, 3, 8, 3.0, sp.store_packed(), sp.P)


def check_sums_from_own_logw(res, what):
    """the reduction alone: the sums against float64 numpy sums of the kernel's OWN logw"""
    a, s1, s2, n = sums_of(res)
    ra, rs1, rs2, rn = ic.sums(res['logw'].cpu().numpy())
    assert a == ra and n == rn, (what, a, ra, n, rn)
    assert s1 == pytest.approx(rs1, rel=1e-12) and s2 == pytest.approx(rs2, rel=1e-12), what


@pytest.mark.parametrize('D,seed,off', [(1, 3, 0), (7, 99, (3 << 32) + 5), (50, (5 << 40) + 1, 1000)])
def test_exported_draws_are_the_defined_stream(D, seed, off):
    """nnest_importance_fill_noise against the definition restated in numpy: to 1e-3 -- a check of the counter layout (a wrong block,
    word or stream is off by O(1)), not of the hardware's log, sin and cos (tests/test_gpu_mcmc_walk.py's figure)"""
    from nnest_amd import flow
    M = 333
    z = flow.importance_fill_noise(M, D, seed=seed, sample_offset=off).cpu().numpy()
    np.testing.assert_allclose(z, ic.importance_draws(seed, off, M, D), rtol=0, atol=1e-3)
    assert z.shape == (M, D) and np.all(np.isfinite(z))


def check_kernel(net, o, D, M, seed, off, tile, tol, x_tol, what, measure=False):
    tol_ll = tol_lw = tol
    from nnest_amd import flow
    groups = groups_of(M, tile)
    assert M > 2 * tile * groups and M % tile != 0, (M, groups)   # at least two passes of the persistent loop, a ragged tail
    sd, mu = affine(D, D)
    rs = Restated(o, sd, mu, BOX)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=seed, sample_offset=off, like_params=(CORR,))
    res = net.importance_evidence(GAUSS, M, want_samples=True, **kw)
    assert res['groups'] == groups
    z, x, logl, logw = (res[k].cpu().numpy() for k in ('z', 'x', 'logl', 'logw'))
    draws = flow.importance_fill_noise(M, D, seed=seed, sample_offset=off)
    assert torch.equal(res['z'], draws), '%s: z_out is not the exported draws' % what
    xo, _ = rs.x_of_z(z)
    if measure:
        # the evaluator's error in nnest_mcmc_steps(steps = 0) on the same points against the same restatement: twice that is allowed
        ev = net.mcmc_steps(GAUSS, res['z'], 0, 0.1, t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), like_params=(CORR,))
        lp_m, lp_r = ev['lp'].cpu().numpy(), rs.lp(z)
        fin = np.isfinite(lp_m) & np.isfinite(lp_r)
        e_lp = float(np.max(np.abs(lp_m[fin] - lp_r[fin])))
        e_ll = float(np.max(np.abs(ev['logl'].cpu().numpy() - rs.logl(xo))))
        e_x = float(np.max(np.abs(ev['x'].cpu().numpy() - xo)))
        print('%s: nnest_mcmc_steps(steps=0) against the restatement: lp %.3g, logL %.3g, x %.3g' % (what, e_lp, e_ll, e_x))
        assert e_lp > 0.0 and e_ll > 0.0 and e_x > 0.0
        # (logw = lp - logb with logb in float64 on both sides: lp's error is logw's)
        tol_lw, tol_ll, x_tol = (lambda v: 2.0 * e_lp + 0.0 * v), (lambda v: 2.0 * e_ll + 0.0 * v), (lambda v: 2.0 * e_x + 0.0 * v)
    lw_r, ll_r = ic.logw_of(z, rs.lp), rs.logl(xo)
    live_k, live_r = ic.is_live(logw), ic.is_live(lw_r)
    # a verdict that hangs on a coordinate near a face
    t = np.abs(rs.T(xo).astype(np.float64)) - BOX
    m = 10.0 * float(np.max(x_tol(np.abs(xo))))
    border = np.all(t <= m, axis=1) & np.any(np.abs(t) <= m, axis=1)
    both = live_k & live_r
    worst_x = float(np.max(np.abs(x - xo) - x_tol(np.abs(xo))))
    worst_ll = float(np.max(np.abs(logl - ll_r) - tol_ll(np.abs(ll_r))))
    worst_lw = float(np.max(np.abs(logw[both] - lw_r[both]) - tol_lw(np.abs(lw_r[both]))))
    print('%s: M %d, groups %d; %d of %d live/dead verdicts excluded, %d live; x %+.3g, logL %+.3g, logw %+.3g over the tolerance '
          '(negative: inside)' % (what, M, groups, int(border.sum()), M, int(live_k.sum()), worst_x, worst_ll, worst_lw))
    assert border.sum() <= 0.01 * M
    assert np.array_equal(live_k[~border], live_r[~border]), '%s: live / dead differ' % what
    assert np.all(logw[~live_k] == -np.inf)   # (a dead sample of this target is outside the box: nothing here is NaN)
    assert worst_x <= 0.0 and worst_ll <= 0.0 and worst_lw <= 0.0
    assert 0 < live_k.sum() < M
    check_sums_from_own_logw(res, what)


@pytest.mark.parametrize('D,off', [(5, 0), (50, 1000), (70, 0), (100, 0)])
def test_nvp_kernel_against_the_restatement(D, off):
    cap = groups_of(1 << 30, 4)
    M = 2 * 4 * cap + 5
    nvp, o = nvp_and_oracle(D, D)
    check_kernel(nvp, o, D, M, 7000 + D, off, 4, lambda v: 2e-5 + 1e-6 * v, lambda v: 5e-5 + 0.0 * v, 'nvp x_dim %d' % D, measure=D > 50)


@pytest.mark.parametrize('D', [5, 40])
def test_spline_kernel_against_the_restatement(D):
    cap = groups_of(1 << 30, 16)
    M = 2 * 16 * cap + 7
    sp, o = spline_and_oracle(D, D)
    check_kernel(sp, o, D, M, 7100 + D, 0, 16, lambda v: SPL_TOL * (1.0 + v), lambda v: SPL_TOL * (1.0 + v), 'spline x_dim %d' % D)


def _flow(name, D, seed):
    return nvp_and_oracle(D, seed)[0] if name == 'nvp' else spline_and_oracle(D, seed)[0]


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_small_launches_and_the_guard_row(name):
    from nnest_amd import _lib
    D = 6
    net = _flow(name, D, 10)
    sd, mu = affine(D, 10)
    dev = net.device
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    vec = lambda v: torch.as_tensor(v, **f32)
    t_std, t_mean, lo, hi = vec(sd), vec(mu), vec(-np.full(D, BOX)), vec(np.full(D, BOX))
    lk = _lib.like_spec(GAUSS, 1.0, (CORR,))
    for M in (0, 1, 3, 17):
        # the per-sample outputs with a guard row behind row M - 1
        z, x = torch.full((M + 1, D), 123.0, **f32), torch.full((M + 1, D), 124.0, **f32)
        logl, logw = torch.full((M + 1,), 125.0, **f64), torch.full((M + 1,), 126.0, **f64)
        groups = groups_of(M, net._IMPORTANCE_TILE)
        assert groups == (M + net._IMPORTANCE_TILE - 1) // net._IMPORTANCE_TILE
        partials, sums = torch.full((3 * groups + 3,), 127.0, **f64), torch.full((4,), 128.0, **f64)
        with torch.cuda.device(dev):
            _lib.check(net._sym['importance'](net._h, ctypes.byref(lk), _lib.ptr(t_std), _lib.ptr(t_mean), _lib.ptr(lo), _lib.ptr(hi),
                                              _lib.ptr(z), _lib.ptr(x), _lib.ptr(logl), _lib.ptr(logw), _lib.ptr(partials), _lib.ptr(sums),
                                              M, 77, 5, _lib.current_stream(dev)))
        torch.cuda.synchronize()
        assert bool((z[M] == 123.0).all()) and bool((x[M] == 124.0).all()) and float(logl[M]) == 125.0 and float(logw[M]) == 126.0
        assert bool((partials[3 * groups:] == 127.0).all())
        a, s1, s2, n = (float(v) for v in sums.cpu().numpy())
        assert 0 <= n <= M and n == int(ic.is_live(logw[:M].cpu().numpy()).sum())
        ra, rs1, rs2, rn = ic.sums(logw[:M].cpu().numpy())
        assert (a, n) == (ra, rn) and s1 == pytest.approx(rs1, rel=1e-12) and s2 == pytest.approx(rs2, rel=1e-12)
        if M == 0:
            assert (a, s1, s2, n) == (-np.inf, 0.0, 0.0, 0.0)
        else:
            assert bool(torch.isfinite(z[:M]).all()) and bool(torch.isfinite(x[:M]).all()) and bool((z[:M] != 123.0).all())
        # the method, without the per-sample outputs: the same sums, bit for bit
        bare = net.importance_evidence(GAUSS, M, t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=77, sample_offset=5,
                                       like_params=(CORR,))
        assert sums_of(bare) == (a, s1, s2, n)
    # T = identity and no prior as NULLs: everything is live
    res = net.importance_evidence(GAUSS, 17, like_params=(CORR,), seed=77, want_samples=True)
    assert sums_of(res)[3] == 17.0 and bool(torch.isfinite(res['logw']).all())
    check_sums_from_own_logw(res, name)


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_a_run_cut_into_launches_is_the_same_run(name):
    from nnest_amd import _lib
    D, M = 20, 1003
    net = _flow(name, D, 8)
    sd, mu = affine(D, 8)
    kw = dict(t_std=sd, t_mean=mu, lo=-np.full(D, BOX), hi=np.full(D, BOX), seed=42, like_params=(CORR,))
    off = (1 << 33) + 11
    one = net.importance_evidence(GAUSS, M, sample_offset=off, want_samples=True, **kw)
    again = net.importance_evidence(GAUSS, M, sample_offset=off, want_samples=True, **kw)
    assert torch.equal(one['sums'].view(torch.int64), again['sums'].view(torch.int64))   # the same call twice: the same bits
    bare = net.importance_evidence(GAUSS, M, sample_offset=off, **kw)
    assert torch.equal(one['sums'].view(torch.int64), bare['sums'].view(torch.int64))   # with and without the per-sample outputs
    cuts = [(0, 400), (400, 13), (413, M - 413)]
    parts = [net.importance_evidence(GAUSS, k, sample_offset=off + first, want_samples=True, **kw) for first, k in cuts]
    for key in ('z', 'x', 'logl', 'logw'):
        assert torch.equal(torch.cat([p[key] for p in parts], 0), one[key]), key
    whole = sums_of(one)
    for merged in (_lib.merge_importance([sums_of(p) for p in parts]),
                   _lib.merge_importance([sums_of(net.importance_evidence(GAUSS, k, sample_offset=off + first, **kw)) for first, k in cuts])):
        assert merged[0] == whole[0] and merged[3] == whole[3]
        assert merged[1] == pytest.approx(whole[1], rel=1e-12) and merged[2] == pytest.approx(whole[2], rel=1e-12)
    assert 0 < whole[3] < M
    other = net.importance_evidence(GAUSS, M, want_samples=True, **kw)   # (another offset: other samples)
    assert not torch.equal(other['z'], one['z'])


def neutral_actnorm(sp):
    """the spline flow's ActNorm layers set to the identity (s = t = 0).  The construction draws them from N(0, 1) as placeholders
    that the reference replaces on the first batch it sees; a flow that has seen no batch is made definite this way"""
    w, off = sp.store_packed(), 0
    for name, shape in sp.layer_shapes():
        n = int(np.prod(shape))
        if name.split('.')[-1] in ('s', 't'):
            w[off:off + n] = 0.0
        off += n
    sp.load_packed(w, sp.P)


# flow seed, t_std, draw seed: picked on the CPU (see test_known_evidence)
KNOWN = {'nvp': (2, 1.6, 1), 'spline': (1, 1.6, 2)}


@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_known_evidence(name):
    """Gaussian(4, 0.5) with the box +-6 on theta: Z = P(box), log Z = 0 to within 1e-8 (the normal cdf bound below).  Both flows
    at their initialisation (the spline with its ActNorm placeholders at the identity: neutral_actnorm; with the N(0, 1) placeholders
    the restatement's ESS / M is about 1e-4), M = 2^16, T(x) = t_std x.  t_std and the seeds were picked on the CPU so that the
    restatement (importance_check.importance_draws through the oracle's flow on the same initialisation) meets ESS / M >= 0.1,
    logzerr <= 0.02 and |logz - exact| <= 2.5 logzerr.  The restatement's numbers:
      nvp    (flow seed 2, t_std 1.6, seed 1):  logz -0.00199, logzerr 0.00656, ESS / M 0.2621
      spline (flow seed 1, t_std 1.6, seed 2):  logz -0.00127, logzerr 0.00880, ESS / M 0.1645"""
    from nnest_amd import _lib, flow
    from nnest_amd.spline import HipSpline
    from scipy.stats import norm
    D, M = 4, 1 << 16
    # the marginals are N(0, 1): 1 - P(box) <= 2 D (1 - Phi(6)), so |log Z| <= -log(1 - 2 D Phi(-6))
    bound = -np.log1p(-2.0 * D * norm.cdf(-6.0))
    assert 0.0 <= bound < 1e-8
    exact = 0.0
    fseed, t_std, seed = KNOWN[name]
    if name == 'nvp':
        net = flow.HipNVP(D, 16, 3, 1, seed=fseed)
    else:
        net = HipSpline(D, 16, 3, seed=fseed)
        neutral_actnorm(net)
    res = net.importance_evidence(GAUSS, M, t_std=np.full(D, t_std), t_mean=np.zeros(D), lo=-np.full(D, 6.0), hi=np.full(D, 6.0), seed=seed,
                                  like_params=(CORR,))
    r = _lib.importance_result(*sums_of(res), M)
    logz = r['logz_x'] + D * np.log(t_std)
    print('%s: logz %.5f, logzerr %.5f, ESS / M %.4f' % (name, logz, r['logzerr'], r['ess'] / M))
    assert abs(logz - exact) <= 4.0 * r['logzerr'] + bound and r['ess'] / M >= 0.05


# ---- the front end ----------------------------------------------------------------------------------------------------------
def _agree(a, b):
    assert abs(a['logz'] - b['logz']) <= 4.0 * np.hypot(a['logzerr'], b['logzerr']), (a, b)


@pytest.mark.parametrize('cls_name,flow_name', [('MCMCSampler', 'nvp'), ('EnsembleSampler', 'spline')])
def test_front_end(tmp_path, cls_name, flow_name):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    from scipy.special import logsumexp
    D, M = 3, 1 << 14
    np.random.seed(1)
    torch.manual_seed(1)
    s = getattr(nnest_amd, cls_name)(D, Gaussian(D, CORR), prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.trainer.train = lambda samples, jitter=0.0, **kw: None   # the flow stays at its initialisation
    train = np.random.RandomState(0).normal(size=(500, D)) * 1.5
    if cls_name == 'MCMCSampler':
        s.run(3, 8, train, route='fused', seed=1)   # installs T(x) = x * std + mean
    else:
        s._install_transform(train.mean(0), train.std(0))
        s.trainer.netG.forward(((train - train.mean(0)) / train.std(0)).astype(np.float32))   # (the spline's ActNorm layers see a batch)
    calls = s.total_calls
    fused = s.importance_evidence(M, seed=3)
    assert fused['route'] == 'fused' and s.importance_route == 'fused' and s.total_calls == calls + M
    assert fused['n_samples'] == M and 0 < fused['n_live'] <= M and 1.0 < fused['ess'] <= M and 0.0 < fused['max_weight_share'] < 1.0
    host = s.importance_evidence(M, route='host')
    assert host['route'] == 'host' and s.importance_route == 'host'
    _agree(fused, host)
    # (the UniformPrior is the indicator of +-5: log Z = log P(box), 0 to 1e-5)
    assert abs(fused['logz']) <= 5.0 * fused['logzerr'] + 1e-5
    assert s.importance_evidence(M, seed=3)['logz'] == fused['logz']   # the same seed: the same number
    cut = s.importance_evidence(M, seed=3, chunk=5000)
    assert cut['logz'] == pytest.approx(fused['logz'], rel=1e-11, abs=1e-11) and cut['n_live'] == fused['n_live']
    got = s.importance_evidence(M, seed=3, return_samples=True)
    assert got['samples'].shape == (M, D) and got['logw'].shape == (M,) and got['logz'] == pytest.approx(fused['logz'], rel=1e-11, abs=1e-11)
    const = float(np.sum(np.log(np.abs(s._ensemble_transform[0]))))
    assert logsumexp(got['logw'][ic.is_live(got['logw'])]) - np.log(M) + const == pytest.approx(got['logz'], rel=1e-11, abs=1e-11)
    live = ic.is_live(got['logw'])
    assert np.all(np.abs(got['samples'][live]) <= 5.0 + 1e-4) and np.any(~live) == (fused['n_live'] < M)


def test_front_end_nested(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from scipy.special import logsumexp
    D, M = 3, 1 << 14
    np.random.seed(2)
    torch.manual_seed(2)
    s = nnest_amd.NestedSampler(D, Gaussian(D, CORR), transform=lambda x: 5 * x, log_dir=str(tmp_path), log_level=30, flow='nvp',
                                num_live_points=50)
    fused = s.importance_evidence(M, seed=4)
    assert fused['route'] == 'fused'
    host = s.importance_evidence(M, route='host')
    assert host['route'] == 'host'
    _agree(fused, host)
    # NestedSampler's convention: the prior is 2^-D on the unit box of x, so Z = P(|theta| <= 5) / 10^D
    assert abs(fused['logz'] + D * np.log(10.0)) <= 5.0 * fused['logzerr'] + 1e-5
    got = s.importance_evidence(M, seed=4, return_samples=True)
    assert got['samples'].shape == (M, D)
    live = ic.is_live(got['logw'])
    assert logsumexp(got['logw'][live]) - np.log(M) - D * np.log(2.0) == pytest.approx(got['logz'], rel=1e-11, abs=1e-11)
    assert np.all(np.abs(got['samples'][live]) <= 5.0 + 1e-4)


def test_front_end_falls_back_to_the_host_and_names_why(tmp_path):
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    D, M = 3, 512
    python_like = lambda x: -0.5 * (x * x).sum(1)
    for kw, like, word in ((dict(flow='nvp'), python_like, 'Python callable'), (dict(flow='maf'), Gaussian(D, CORR), 'HipMAF')):
        s = nnest_amd.MCMCSampler(D, like, log_dir=str(tmp_path), log_level=30, **kw)
        s._install_transform(np.zeros(D), np.full(D, 1.5))
        out = s.importance_evidence(M)
        assert out['route'] == 'host' and np.isfinite(out['logz']) and out['n_live'] == M
        with pytest.raises(ValueError, match='the fused route does not take .*%s' % word):
            s.importance_evidence(M, route='fused')


def test_the_library_refuses_what_the_kernels_do_not_take():
    """NNEST_E_UNSUPPORTED with the reason, before any launch (the outputs keep their contents): another RealNVP shape, a
    GeneralisedNormal base, an unknown likelihood id; `importance_refusal` answers the same without a launch"""
    from nnest_amd import _lib, flow
    from nnest_amd.spline import HipSpline
    D = 3
    lib = _lib.load()

    def refused(net, like_id, word):
        why = net.importance_refusal(like_id)
        assert why is not None and word in why, why
        dev = net.device
        sums = torch.full((4,), 128.0, dtype=torch.float64, device=dev)
        partials = torch.full((6,), 127.0, dtype=torch.float64, device=dev)
        lk = _lib.like_spec(like_id, 1.0, (CORR,))
        with torch.cuda.device(dev):
            rc = net._sym['importance'](net._h, ctypes.byref(lk), None, None, None, None, None, None, None, None, _lib.ptr(partials),
                                        _lib.ptr(sums), 8, 1, 0, _lib.current_stream(dev))
        torch.cuda.synchronize()
        assert rc == _lib.NNEST_E_UNSUPPORTED and word.encode() in lib.nnest_hip_last_error()
        assert bool((sums == 128.0).all()) and bool((partials == 127.0).all())
        with pytest.raises(_lib.NnestHipError, match=word) as e:
            net.importance_evidence(like_id, 8, like_params=(CORR,))
        assert e.value.code == _lib.NNEST_E_UNSUPPORTED

    for kw, word in ((dict(num_hidden=32), 'hidden=32'), (dict(num_blocks=2), 'blocks=2'), (dict(num_layers=2), 'layers=2'),
                     (dict(scale='translate'), 'scale mode 1')):
        refused(flow.HipNVP(D, **kw), GAUSS, word)
    for net in (flow.HipNVP(D, 16, 3, 1, seed=1), HipSpline(D, 16, 3, seed=1)):
        assert net.importance_refusal(GAUSS) is None
        refused(net, 99, 'unknown likelihood id 99')
        with torch.cuda.device(net.device):
            _lib.check(net._sym['set_base'](net._h, ctypes.c_float(8.0)))   # GeneralisedNormal(0, 1, beta = 8)
        refused(net, GAUSS, 'GeneralisedNormal')
        with torch.cuda.device(net.device):
            _lib.check(net._sym['set_base'](net._h, ctypes.c_float(0.0)))
        assert net.importance_refusal(GAUSS) is None and sums_of(net.importance_evidence(GAUSS, 8, like_params=(CORR,)))[3] == 8.0


@pytest.mark.parametrize('kw,word', [(dict(hidden_dim=32), 'hidden=32'), (dict(num_blocks=2), 'blocks=2'), (dict(scale='translate'), 'scale mode 1')])
def test_front_end_takes_the_host_route_for_another_nvp_shape(tmp_path, kw, word):
    """a RealNVP the project supports and the kernel does not take: route=None observes it (the library is asked before any launch)
    and runs on the host; route='fused' names the shape"""
    import nnest_amd
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.priors import UniformPrior
    D, M = 3, 1 << 12
    s = nnest_amd.MCMCSampler(D, Gaussian(D, CORR), prior=UniformPrior(D, -5, 5), log_dir=str(tmp_path), log_level=30, flow='nvp', **kw)
    s._install_transform(np.zeros(D), np.full(D, 1.5))
    out = s.importance_evidence(M)
    assert out['route'] == 'host' and s.importance_route == 'host' and np.isfinite(out['logz']) and 0 < out['n_live'] <= M
    with pytest.raises(ValueError, match='the fused route does not take the flow HipNVP: .*%s' % word):
        s.importance_evidence(M, route='fused')
    # the nested front end, as `python -m nnest_amd.run --flow nvp --hidden_dim 32 --importance_samples N` reaches it
    if 'hidden_dim' in kw:
        ns = nnest_amd.NestedSampler(D, Gaussian(D, CORR), transform=lambda x: 5 * x, log_dir=str(tmp_path), log_level=30, flow='nvp',
                                     num_live_points=50, **kw)
        got = ns.importance_evidence(M)
        assert got['route'] == 'host' and np.isfinite(got['logz'])
