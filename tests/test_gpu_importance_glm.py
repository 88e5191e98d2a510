"""GPU checks of the importance-sampled evidence of a regression (include/nnest_hip.h nnest_importance_glm_evidence,
nnest_spline_importance_glm_evidence and their _check entries; HipNVP / HipSpline.importance_evidence with like_glm and prior_gauss;
Sampler.importance_evidence on a likelihoods.GLMData), after tests/test_gpu_importance.py:
  1. both kernels against the numpy restatement (tests/importance_glm_check.py) on their own draws, over more than two passes of
     the persistent loop and a ragged tail, under a box, under a GaussianPrior and with neither;
  2. the reduction against float64 sums of the kernel's own log weights;
  3. determinism: the same call twice, with and without the per-sample outputs, a run cut into launches, dirtied padded rows;
  4. small launches and a guard row;
  5. a non-finite sample is dead, not NaN in the sums;
  6. the argument errors;
  7. the front end against the float64 grid quadrature of L pi.

Tolerances, those in force for these evaluators (tests/test_gpu_mcmc_glm.py).  logL at the kernel's own x (with T applied as
affine_on_device applies it) is held to float64 within the a-priori bound B of tests/glm_check.py alone.  The flow's part --
logw + logb - logL - log pi against the restated log-determinant, x against the restated inverse -- takes the flow's tolerances:
NVP x_dim <= 50 rtol 1e-6, atol 2e-5 on lp and 5e-5 on x; NVP x_dim 70 and 100 twice the error measured of nnest_ensemble_steps, the
same evaluator, at that width (tests/test_gpu_mcmc_adapt.py measured_tolerances); spline 3e-5 (1 + |v|).  log pi is not an output
of its own: the exact log pi (tests/gauss_prior_check.exact) at the kernel's own T(x) is subtracted, and its bound B_pi there is
added to the flow's tolerance.  Live / dead is compared unless the verdict hangs on a coordinate of T(x) within ten times the x
tolerance of a face of the box; at most 1 % of M may be excluded.  Box and seed of each case were chosen on the CPU
(tools/importance_glm_cases.py): the restatement alone leaves at most 0.25 % that close, and at least 2 % of the samples on
either side.

Measured on the MI355X: logL at most 0.0142 (NVP) and 0.0196 (spline) of B off float64; the flow's part and x inside the flows'
tolerances in every case; at most 4 of 8197 (NVP) and 21 of 16391 (spline) verdicts excluded; the front end's log Z within 1.6 of
its standard errors (0.0005 to 0.0009 with a trained flow, 0.009 through the unit box with an untrained one) of the quadrature,
ESS 0.83 to 0.94 of 2^18 with a trained flow; SMCSampler's log Z over 8 seeds -32.781 +- 0.011 beside the importance-sampled
-32.8054 +- 0.0007 and the quadrature's -32.8064."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gauss_prior_check as gp
from tests import glm_check as gk
from tests import importance_glm_check as igc
from tests.test_gpu_importance import affine, check_sums_from_own_logw, groups_of, nvp_and_oracle, spline_and_oracle, sums_of

pytestmark = pytest.mark.gpu

SPL_TOL = 3e-5
BIG = (3 << 32) + 5   # a sample_offset beyond 2^32
E_ARG, E_UNSUPPORTED = 1, 3
# (flow, x_dim, n, family, sample_offset): box, seed -- tools/importance_glm_cases.py.  The flow widths, rows and families of
# tests/test_gpu_mcmc_glm.py's REPLAY table: every U and both weight placements of the NVP, the spline's NT 1 and 2; n = 40: a
# ragged 64-row pass and three row blocks, so that the spline's wave 3 has none; n = 70: two passes and five row blocks
CASES = {('nvp', 5, 40, 'logistic', 0): (2.5, 7305), ('nvp', 5, 70, 'poisson', BIG): (2.5, 7305),
         ('nvp', 50, 70, 'poisson', 1000): (2.5, 7350), ('nvp', 50, 40, 'logistic', BIG): (2.5, 7350),
         ('nvp', 70, 70, 'logistic', 0): (2.5, 7370), ('nvp', 70, 40, 'poisson', BIG): (2.5, 7370),
         ('nvp', 100, 40, 'poisson', BIG): (3.0, 7400), ('nvp', 100, 70, 'logistic', 0): (3.0, 7400),
         ('spline', 5, 40, 'poisson', BIG): (1.5, 7305), ('spline', 5, 70, 'logistic', 0): (1.5, 7305),
         ('spline', 40, 70, 'logistic', BIG): (1.0, 7340), ('spline', 40, 40, 'poisson', 0): (1.0, 7340)}
NEITHER = {('nvp', 5, 40, 'logistic', 0), ('spline', 5, 70, 'logistic', 0)}   # one case per flow also runs with no box and no prior


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def check_kernel(net, o, case, tol, x_tol):
    """tol(v): the flow's lp tolerance at value v; x_tol(v): its x tolerance at |x| = v"""
    from nnest_amd import flow
    from nnest_amd.device_target import affine_on_device
    name, D, n, family, off = case
    half, seed = CASES[case]
    tile = net._IMPORTANCE_TILE
    M = 2 * tile * groups_of(1 << 30, tile) + (5 if name == 'nvp' else 7)
    groups = groups_of(M, tile)
    assert M > 2 * tile * groups and M % tile != 0, (M, groups)   # more than two passes of the persistent loop, a ragged tail
    sd, mu = affine(D, D)
    data = gk.replay_target(D, n, family)
    prior = gp.replay_prior(D, 1.0)
    draws = flow.importance_fill_noise(M, D, seed=seed, sample_offset=off)
    z = draws.cpu().numpy()
    xo, ldo = o.inverse(z)
    ldo = np.asarray(ldo, np.float64)
    dev = net.device
    sd_t, mu_t = torch.as_tensor(sd, device=dev), torch.as_tensor(mu, device=dev)
    modes = [('box', dict(lo=-np.full(D, half), hi=np.full(D, half)), dict(half=half)),
             ('prior', dict(prior_gauss=prior.hip_gauss_prior), dict(prior=prior))]
    if case in NEITHER:
        modes.append(('neither', {}, {}))
    for mode, kw, rkw in modes:
        what = '%s x_dim %d n %d %s, %s' % (name, D, n, family, mode)
        rs = igc.restated(o, data, sd, mu, **rkw)
        res = net.importance_evidence(None, M, t_std=sd, t_mean=mu, like_glm=data, seed=seed, sample_offset=off, want_samples=True, **kw)
        assert res['groups'] == groups
        assert torch.equal(bits(res['z']), bits(draws)), '%s: z_out is not the exported draws' % what
        x, logl, logw = (res[k].cpu().numpy() for k in ('x', 'logl', 'logw'))
        # logL at the kernel's own x, T applied on the device as the front ends apply it: float64 within B
        t = affine_on_device(res['x'], sd_t, mu_t).cpu().numpy()
        assert np.array_equal(t, rs.T(x))
        ll, B = gk.exact(data, t)[0], gk.bound(data, t)
        assert np.all(np.isfinite(ll)) and np.all(ll != gk.SAFE)
        worst_ll = float(np.max(np.abs(logl - ll) / B))
        # x against the restated inverse
        worst_x = float(np.max(np.abs(x - xo) - x_tol(np.abs(xo))))
        # live / dead against the restatement, but where the verdict hangs on a coordinate near a face
        lw_r = igc.logw(rs, z)
        live_k, live_r = igc.is_live(logw), igc.is_live(lw_r)
        border = igc.near_face(rs, xo, 10.0 * float(np.max(x_tol(np.abs(xo)))))
        assert border.sum() <= 0.01 * M, what
        assert np.array_equal(live_k[~border], live_r[~border]), '%s: live / dead differ' % what
        assert np.all(logw[~live_k] == -np.inf)   # (a dead sample of these targets is outside the box: nothing here is NaN)
        # the flow's part: logw + logb - logL - log pi, the prior's term exact at the kernel's own T(x)
        logpi = gp.exact(prior, t) if mode == 'prior' else np.zeros(M)
        B_pi = gp.bound(prior, t) if mode == 'prior' else np.zeros(M)
        ld_k = ((logw + igc.logb(z)) - logl - logpi)[live_k]
        worst_ld = float(np.max(np.abs(ld_k - ldo[live_k]) - tol(ldo[live_k]) - B_pi[live_k]))
        print('%s: M %d, groups %d; %d verdicts excluded, %d live; logL at most %.3g of B off float64; log|det| %+.3g, x %+.3g over the '
              'tolerance (negative: inside)' % (what, M, groups, int(border.sum()), int(live_k.sum()), worst_ll, worst_ld, worst_x))
        assert worst_ll <= 1.0 and worst_ld <= 0.0 and worst_x <= 0.0, what
        if mode == 'box':
            assert 0 < live_k.sum() < M
        else:
            assert live_k.all()
        # 2. the reduction alone
        check_sums_from_own_logw(res, what)


@pytest.mark.parametrize('case', [c for c in sorted(CASES) if c[0] == 'nvp'], ids=lambda c: '%d-%d-%s' % c[1:4])
def test_nvp_kernel_against_the_restatement(case):
    from tests.test_gpu_mcmc_adapt import measured_tolerances
    from tests.test_gpu_mcmc_mixed import Restated as GaussRestated
    from nnest_amd import flow
    D = case[1]
    nvp, o = nvp_and_oracle(D, D)
    if D <= 50:
        tol, x_tol = (lambda v: 2e-5 + 1e-6 * np.abs(v)), (lambda v: 5e-5 + 0.0 * v)
    else:   # (the flow's error at this width, measured on the kernel that shares its evaluator, on its own likelihood)
        half, seed = CASES[case]
        sd, mu = affine(D, D)
        z0 = flow.importance_fill_noise(70, D, seed=seed, sample_offset=case[4])
        tol, x_tol, _ = measured_tolerances(nvp, GaussRestated(o, sd, mu, half), z0, sd, mu, half, seed, 0)
    check_kernel(nvp, o, case, tol, x_tol)


@pytest.mark.parametrize('case', [c for c in sorted(CASES) if c[0] == 'spline'], ids=lambda c: '%d-%d-%s' % c[1:4])
def test_spline_kernel_against_the_restatement(case):
    D = case[1]
    sp, o = spline_and_oracle(D, D)
    t = lambda v: SPL_TOL * (1.0 + np.abs(v))
    check_kernel(sp, o, case, t, t)


def _flow(name, D, seed):
    return nvp_and_oracle(D, seed)[0] if name == 'nvp' else spline_and_oracle(D, seed)[0]


def _target(D, n, family, seed, mode, half=2.0):
    """(the keywords of a launch on this model, the likelihood): T = affine(D, seed), under the box +-half or a GaussianPrior"""
    sd, mu = affine(D, seed)
    like = gk.make_like(D, n, family, seed)
    kw = dict(t_std=sd, t_mean=mu, like_glm=like.hip_like_glm)
    if mode == 'box':
        kw.update(lo=-np.full(D, half), hi=np.full(D, half))
    elif mode == 'prior':
        kw.update(prior_gauss=gp.replay_prior(D, 1.0).hip_gauss_prior)
    return kw, like


# ---- 3. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,mode,family', [('nvp', 'box', 'poisson'), ('nvp', 'prior', 'logistic'), ('spline', 'box', 'logistic'),
                                              ('spline', 'prior', 'poisson')])
def test_a_run_cut_into_launches_is_the_same_run(name, mode, family):
    from nnest_amd import _lib
    D, M, n = 20, 1003, 70
    net = _flow(name, D, 8)
    kw, like = _target(D, n, family, 8, mode, half=1.0 if name == 'spline' else 2.0)
    kw['seed'] = 42
    off = (1 << 33) + 11
    one = net.importance_evidence(None, M, sample_offset=off, want_samples=True, **kw)
    again = net.importance_evidence(None, M, sample_offset=off, want_samples=True, **kw)
    assert torch.equal(bits(one['sums']), bits(again['sums']))   # the same call twice: the same bits
    bare = net.importance_evidence(None, M, sample_offset=off, **kw)
    assert torch.equal(bits(one['sums']), bits(bare['sums']))   # with and without the per-sample outputs
    cuts = [(0, 400), (400, 13), (413, M - 413)]
    parts = [net.importance_evidence(None, k, sample_offset=off + first, want_samples=True, **kw) for first, k in cuts]
    for key in ('z', 'x', 'logl', 'logw'):
        assert torch.equal(bits(torch.cat([p[key] for p in parts], 0)), bits(one[key])), key
    whole = sums_of(one)
    for merged in (_lib.merge_importance([sums_of(p) for p in parts]),
                   _lib.merge_importance([sums_of(net.importance_evidence(None, k, sample_offset=off + first, **kw)) for first, k in cuts])):
        assert merged[0] == whole[0] and merged[3] == whole[3]
        assert merged[1] == pytest.approx(whole[1], rel=1e-12) and merged[2] == pytest.approx(whole[2], rel=1e-12)
    assert (0 < whole[3] < M) if mode == 'box' else whole[3] == M
    other = net.importance_evidence(None, M, want_samples=True, **kw)   # (another offset: other samples)
    assert not torch.equal(other['z'], one['z'])
    # what lies beyond row n in the padded arrays changes no bit
    data = kw['like_glm']
    ld = data['at'].shape[1]
    r = np.random.RandomState(3)
    dirty = dict(data, at=data['at'].copy(), y=data['y'].copy(), o=data['o'].copy())
    dirty['at'][:, n:] = r.normal(size=(D, ld - n)) * 1e6
    dirty['y'][n:] = 7.0
    dirty['o'][n:] = np.nan
    got = net.importance_evidence(None, M, sample_offset=off, want_samples=True, **dict(kw, like_glm=dirty))
    for key in ('sums', 'z', 'x', 'logl', 'logw'):
        assert torch.equal(bits(got[key]), bits(one[key])), 'rows beyond n are not masked: %s' % key


# ---- 4. small launches ------------------------------------------------------------------------------------------------------------------
def _raw(net, spec, pspec, vecs, outs, partials, sums, M, seed=77, off=5):
    from nnest_amd import _lib
    dev = net.device
    with torch.cuda.device(dev):
        return net._sym['importance_glm'](
            net._h, None if spec is None else ctypes.byref(spec), None if pspec is None else ctypes.byref(pspec), *[_lib.ptr(v) for v in vecs],
            *[_lib.ptr(v) for v in outs], _lib.ptr(partials), _lib.ptr(sums), M, seed, off, _lib.current_stream(dev))


@pytest.mark.parametrize('mode', ['box', 'prior'])
@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_small_launches_and_the_guard_row(name, mode):
    from nnest_amd import _lib, flow
    D = 6
    net = _flow(name, D, 10)
    kw, like = _target(D, 40, 'logistic', 10, mode)
    dev = net.device
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    vec = lambda v: None if v is None else torch.as_tensor(np.asarray(v, np.float32), **f32)
    vecs = [vec(kw['t_std']), vec(kw['t_mean']), vec(kw.get('lo')), vec(kw.get('hi'))]
    spec, keep = flow.glm_spec(kw['like_glm'], dev)
    pspec, pkeep = flow.gauss_prior_spec(kw['prior_gauss'], dev) if mode == 'prior' else (None, None)
    tile = net._IMPORTANCE_TILE
    for M in (0, 1, tile - 1, tile + 1):
        # the per-sample outputs with a guard row behind row M - 1
        z, x = torch.full((M + 1, D), 123.0, **f32), torch.full((M + 1, D), 124.0, **f32)
        logl, logw = torch.full((M + 1,), 125.0, **f64), torch.full((M + 1,), 126.0, **f64)
        groups = groups_of(M, tile)
        assert groups == (M + tile - 1) // tile
        partials, sums = torch.full((3 * groups + 3,), 127.0, **f64), torch.full((4,), 128.0, **f64)
        _lib.check(_raw(net, spec, pspec, vecs, (z, x, logl, logw), partials, sums, M))
        torch.cuda.synchronize()
        assert bool((z[M] == 123.0).all()) and bool((x[M] == 124.0).all()) and float(logl[M]) == 125.0 and float(logw[M]) == 126.0
        assert bool((partials[3 * groups:] == 127.0).all())
        a, s1, s2, n = (float(v) for v in sums.cpu().numpy())
        ra, rs1, rs2, rn = igc.sums(logw[:M].cpu().numpy())
        assert (a, n) == (ra, rn) and s1 == pytest.approx(rs1, rel=1e-12) and s2 == pytest.approx(rs2, rel=1e-12)
        if M == 0:
            assert (a, s1, s2, n) == (-np.inf, 0.0, 0.0, 0.0)
        else:
            assert bool(torch.isfinite(z[:M]).all()) and bool(torch.isfinite(x[:M]).all()) and bool((z[:M] != 123.0).all())
            assert torch.equal(z[:M], flow.importance_fill_noise(M, D, seed=77, sample_offset=5))
            assert bool((logl[:M] <= like.logl0).all())
        # the method, without the per-sample outputs: the same sums, bit for bit
        bare = net.importance_evidence(None, M, seed=77, sample_offset=5, **kw)
        assert sums_of(bare) == (a, s1, s2, n)


# ---- 5. a non-finite sample is dead -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_a_non_finite_sample_is_dead_not_nan(name):
    D, M = 6, 37
    net = _flow(name, D, 10)
    kw, like = _target(D, 40, 'poisson', 10, 'prior')
    mu = np.array(kw['t_mean'], np.float32)
    mu[D - 2] = np.inf
    res = net.importance_evidence(None, M, seed=3, want_samples=True, **dict(kw, t_mean=mu))
    assert sums_of(res) == (-np.inf, 0.0, 0.0, 0.0)
    logw = res['logw'].cpu().numpy()
    assert np.all(logw == -np.inf) and np.all(res['logl'].cpu().numpy() == -1e100)
    assert bool(torch.isfinite(res['x']).all())   # (x is before T)
    # the same launch with the finite T: everything live
    ok = net.importance_evidence(None, M, seed=3, want_samples=True, **kw)
    assert sums_of(ok)[3] == M and torch.equal(ok['z'], res['z']) and torch.equal(ok['x'], res['x'])


# ---- 6. the argument errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nvp', 'spline'])
def test_argument_errors_leave_the_outputs_alone(name):
    from nnest_amd import _lib, flow
    D, M = 5, 9
    net = _flow(name, D, 3)
    dev = net.device
    like = gk.make_like(D, 100, 'logistic', 3)
    data = like.hip_like_glm
    prior = gp.replay_prior(D, 1.0).hip_gauss_prior
    good, keep = flow.glm_spec(data, dev)
    other, keep4 = flow.glm_spec(gk.make_like(4, 100, 'logistic', 3).hip_like_glm, dev)
    pgood, pkeep = flow.gauss_prior_spec(prior, dev)
    pother, pkeep4 = flow.gauss_prior_spec(gp.replay_prior(4, 1.0).hip_gauss_prior, dev)
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    one = torch.ones(D, **f32)

    def spec(**kw):
        s = _lib.GlmSpec(good.at_dev, good.y_dev, good.o_dev, good.logl0, good.n, good.ld, good.D, good.family)
        for key, val in kw.items():
            setattr(s, key, val)
        return s

    def pspec(**kw):
        s = type(pgood)(*[getattr(pgood, f[0]) for f in pgood._fields_])
        for key, val in kw.items():
            setattr(s, key, val)
        return s

    def buffers():
        return ([torch.full((M, D), 123.0, **f32), torch.full((M, D), 123.0, **f32), torch.full((M,), 123.0, **f64),
                 torch.full((M,), 123.0, **f64)], torch.full((3 * M,), 123.0, **f64), torch.full((4,), 123.0, **f64))

    none4 = [None, None, None, None]
    bad_specs = [('glm is NULL', None), ('NULL at_dev', spec(at_dev=None)), ('NULL at_dev', spec(y_dev=None)), ('NULL at_dev', spec(o_dev=None)),
                 ('D=0', spec(D=0)), ('D=129', spec(D=129)), ('n=0', spec(n=0)), ('n=65537', spec(n=65537, ld=65600)),
                 ('ld=64', spec(ld=64)), ('ld=200', spec(ld=200)), ('ld=65600', spec(ld=65600)), ('family=2', spec(family=2)),
                 ('logl0=inf', spec(logl0=float('inf'))), ('logl0=nan', spec(logl0=float('nan')))]
    bad_priors = [('NULL m_dev or r_dev', pspec(m_dev=None)), ('NULL m_dev or r_dev', pspec(r_dev=None)), ('prior: D=0', pspec(D=0)),
                  ('prior: D=129', pspec(D=129)), ("the prior's D=4 is not", pother), ('logc=inf', pspec(logc=float('inf'))),
                  ('logc=nan', pspec(logc=float('nan')))]
    cases = [(what, dict(spec=s)) for what, s in bad_specs] + [(what, dict(pspec=p)) for what, p in bad_priors] + [
        ("the likelihood's D=4 is not the flow's x_dim=5", dict(spec=other)),
        ('M=-1', dict(M=-1)), ('M=1073741825', dict(M=(1 << 30) + 1)),
        ('all or none', dict(drop_out=0)), ('all or none', dict(drop_out=1)), ('all or none', dict(drop_out=2)), ('all or none', dict(drop_out=3)),
        ('NULL sums_dev or partials_dev', dict(no_sums=True)), ('NULL sums_dev or partials_dev', dict(no_partials=True)),
        ('t_std_dev and t_mean_dev: both or neither', dict(vecs=[one, None, None, None])),
        ('t_std_dev and t_mean_dev: both or neither', dict(vecs=[None, one, None, None])),
        ('lo_dev and hi_dev: both or neither', dict(vecs=[None, None, one, None])),
        ('lo_dev and hi_dev: both or neither', dict(vecs=[None, None, None, one])),
        ('a prior together with the box', dict(pspec=pgood, vecs=[None, None, -one, one]))]
    for what, kw in cases:
        outs, partials, sums = buffers()
        args = dict(spec=good, pspec=None, vecs=none4, M=M)
        args.update(kw)
        o = list(outs)
        if 'drop_out' in args:
            o[args['drop_out']] = None
        rc = _raw(net, args['spec'], args['pspec'], args['vecs'], o, None if args.get('no_partials') else partials,
                  None if args.get('no_sums') else sums, args['M'])
        torch.cuda.synchronize()
        words = net._lib.nnest_hip_last_error().decode()
        assert rc == E_ARG and what in words, (what, rc, words)
        for t in outs + [partials, sums]:
            assert bool((t == 123.0).all()), what
    # the calls with nothing wrong run: no prior and no box, a box, a prior
    for p, vecs in ((None, none4), (None, [None, None, -one, one]), (pgood, none4)):
        outs, partials, sums = buffers()
        assert _raw(net, good, p, vecs, outs, partials, sums, M) == 0
        torch.cuda.synchronize()
        assert bool((outs[2] <= like.logl0).all()) and 0 <= float(sums[3]) <= M
    # a GeneralisedNormal base: NNEST_E_UNSUPPORTED from the _check and from the entry, before any launch
    assert net.importance_glm_refusal() is None and net.importance_glm_refusal(D) is None
    assert "the likelihood's D=4 is not the flow's x_dim=5" in net.importance_glm_refusal(4)
    with torch.cuda.device(dev):
        _lib.check(net._sym['set_base'](net._h, ctypes.c_float(8.0)))   # GeneralisedNormal(0, 1, beta = 8)
        assert net._sym['importance_glm_check'](net._h, D) == E_UNSUPPORTED
    assert 'GeneralisedNormal' in net.importance_glm_refusal()
    outs, partials, sums = buffers()
    rc = _raw(net, good, pgood, none4, outs, partials, sums, M)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED and b'GeneralisedNormal' in net._lib.nnest_hip_last_error()
    for t in outs + [partials, sums]:
        assert bool((t == 123.0).all())
    with pytest.raises(_lib.NnestHipError, match='GeneralisedNormal') as e:
        net.importance_evidence(None, M, like_glm=data, prior_gauss=prior)
    assert e.value.code == E_UNSUPPORTED
    with torch.cuda.device(dev):
        _lib.check(net._sym['set_base'](net._h, ctypes.c_float(0.0)))
    assert net.importance_glm_refusal() is None
    # through the Python layer: the library's words in the exception, the binding's own for what never reaches the library
    with pytest.raises(_lib.NnestHipError, match='glm: n=0'):
        net.importance_evidence(None, M, like_glm=dict(data, n=0))
    with pytest.raises(_lib.NnestHipError, match="the likelihood's D=4 is not the flow's x_dim=5"):
        net.importance_evidence(None, M, like_glm=gk.make_like(4, 100, 'logistic', 3).hip_like_glm)
    with pytest.raises(ValueError, match='prior_gauss goes without lo / hi'):
        net.importance_evidence(None, M, like_glm=data, prior_gauss=prior, lo=-np.ones(D), hi=np.ones(D))
    with pytest.raises(ValueError, match='prior_gauss goes only with a like_glm'):
        net.importance_evidence(3, M, prior_gauss=prior)


# ---- 7. the front end -------------------------------------------------------------------------------------------------------------------
M_FRONT, M_HOST = 1 << 18, 1 << 16
LOG2 = float(np.log(2.0))


def _trained(tmp_path, like, prior, flow_name):
    """an MCMCSampler whose flow was trained through the fused run, as tests/test_gpu_mcmc_glm_prior.py test_mcmc_front_end trains it"""
    import nnest_amd
    from tests.test_gpu_mcmc_glm_prior import posterior_draws
    from nnest_amd.priors import GaussianPrior
    rng = np.random.RandomState(3)
    train = posterior_draws(like, prior if isinstance(prior, GaussianPrior) else GaussianPrior(2, 0.0, 2.0), rng, 2000)
    init = (train[:64] - train.mean(0)) / train.std(0)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(2, like, prior=prior, log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.run(200, 64, train, init_samples=init, route='fused', seed=1, adapt_steps=100, global_every=5)
    assert s.mcmc_route == 'fused'
    return s


def _check_front(s, exact, what):
    from scipy.special import logsumexp
    calls = s.total_calls
    fused = s.importance_evidence(M_FRONT, seed=3)
    assert fused['route'] == 'fused' and s.importance_route == 'fused' and s.total_calls == calls + M_FRONT
    host = s.importance_evidence(M_HOST, route='host')
    assert host['route'] == 'host'
    print('%s: fused logz %.4f +- %.4f (ESS %.0f of %d), host %.4f +- %.4f, quadrature %.4f' % (
        what, fused['logz'], fused['logzerr'], fused['ess'], M_FRONT, host['logz'], host['logzerr'], exact))
    # five standard errors stay under log 2, the smallest constant a wrong convention shifts the result by (a box normalisation,
    # logc, logl_const, sum log t_std): a condition of the test -- a flow that misses it wants more samples, not a wider bound
    assert fused['logzerr'] < 0.1 and 5.0 * fused['logzerr'] < LOG2
    assert abs(fused['logz'] - exact) <= 5.0 * fused['logzerr'], (what, fused, exact)
    assert abs(fused['logz'] - host['logz']) <= 5.0 * np.hypot(fused['logzerr'], host['logzerr']), (what, fused, host)
    got = s.importance_evidence(M_FRONT, seed=3, return_samples=True)
    assert got['samples'].shape == (M_FRONT, 2) and got['logz'] == pytest.approx(fused['logz'], rel=1e-11, abs=1e-11)
    const = s._importance_constant(s._ensemble_affine())
    live = igc.is_live(got['logw'])
    assert logsumexp(got['logw'][live]) - np.log(M_FRONT) + const == pytest.approx(got['logz'], rel=1e-11, abs=1e-11)
    return fused


@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_front_end_known_evidence(tmp_path, flow_name, family):
    """D = 2 under GaussianPrior(2, 0, 2): log Z against the grid quadrature of L pi with the normalised pi"""
    from nnest_amd.priors import GaussianPrior
    from tests.test_gpu_mcmc_glm_prior import quadrature
    like = gk.make_like(2, 40, family, 5)
    prior = GaussianPrior(2, 0.0, 2.0)
    exact = quadrature(like, prior, -20.0, 20.0)[0]   # (ten sigma of the prior)
    s = _trained(tmp_path, like, prior, flow_name)
    _check_front(s, exact, '%s %s' % (flow_name, family))


def test_front_end_uniform_prior(tmp_path):
    """the UniformPrior on [-4, 4]^2 is the unnormalised indicator of its box: log Z is the log integral of L over the box"""
    from nnest_amd.priors import UniformPrior
    from tests.test_gpu_mcmc_glm import quadrature
    like = gk.make_like(2, 40, 'poisson', 5)
    s = _trained(tmp_path, like, UniformPrior(2, -4.0, 4.0), 'spline')
    _check_front(s, quadrature(like, -4.0, 4.0)[0], 'spline poisson, UniformPrior')


def test_front_end_nested_unit_box(tmp_path):
    """NestedSampler's convention: the prior is 2^-D on the unit box of x and theta = 5 x, so Z = int_{+-5} L d theta / 10^D"""
    import nnest_amd
    from tests.test_gpu_mcmc_glm import quadrature
    like = gk.make_like(2, 40, 'logistic', 5)
    np.random.seed(2)
    torch.manual_seed(2)
    s = nnest_amd.NestedSampler(2, like, transform=lambda x: 5 * x, log_dir=str(tmp_path), log_level=30, flow='nvp', num_live_points=50)
    _check_front(s, quadrature(like, -5.0, 5.0)[0] - 2 * np.log(10.0), 'nvp logistic, the unit box on x')


def test_front_end_beside_the_annealed_estimate(tmp_path):
    """the two evidence estimators on one model: SMCSampler.logz over 8 seeds (its standard error from their spread) and the
    importance-sampled estimate from the flow SMC trained last; each within five of its own standard errors of the quadrature"""
    from nnest_amd.priors import GaussianPrior
    from tests.test_gpu_mcmc_glm_prior import _smc_logz, quadrature
    like = gk.make_like(2, 40, 'logistic', 5)
    prior = GaussianPrior(2, 0.0, 2.0)
    exact = quadrature(like, prior, -20.0, 20.0)[0]
    s, mean_z, se, var = _smc_logz(tmp_path, like, prior, 'nvp')
    imp = s.importance_evidence(M_FRONT, seed=5)
    print('quadrature %.4f; annealed log Z %.4f +- %.4f over 8 seeds; importance-sampled %.4f +- %.4f (ESS %.0f of %d, route %s)' % (
        exact, mean_z, se, imp['logz'], imp['logzerr'], imp['ess'], M_FRONT, imp['route']))
    assert imp['route'] == 'fused'
    assert abs(mean_z - exact) <= 5.0 * se
    assert abs(imp['logz'] - exact) <= 5.0 * imp['logzerr']


def test_front_end_without_a_prior(tmp_path):
    """a GLMData with no prior: the integral of the likelihood over R^D is not an evidence -- route='fused' refuses in the words a
    Python callable gets, route=None runs on the host"""
    import nnest_amd
    like = gk.make_like(2, 40, 'logistic', 5)
    s = nnest_amd.MCMCSampler(2, like, log_dir=str(tmp_path), log_level=30, flow='nvp')
    s._install_transform(np.zeros(2), np.full(2, 1.5))
    with pytest.raises(ValueError, match='importance_evidence: the fused route does not take a likelihood the kernels do not know'):
        s.importance_evidence(64, route='fused')
    out = s.importance_evidence(512)
    assert out['route'] == 'host' and np.isfinite(out['logz'])
