"""The gradient, curvature and Newton-step kernels of the regression likelihoods (include/nnest_hip.h nnest_glm_curv,
nnest_glm_newton_solve) and GLMData.laplace on the fused route, against the longdouble restatement and the derived
bounds of tests/glm_newton_check.py, and against the host route.

The worst shares of the bounds the tests print, on an MI355X (recorded in DESIGN.md 3.21 too): the curvature -- logL 0.036, gradient
0.034, Hessian 0.072; the solve -- step 0.19, log det 0.26, decrement 0.067, log posterior 0.30, factor 0.49 (all largest at D = 1,
where the bounds are a few ulp); fused against host -- the modes apart by 5.3e-10 of their bound, log Z by 0.0091 of its bound, the
restated decrement at most 0.45 of 2 tol."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import glm_check as gk
from tests import glm_newton_check as nk
from tests.test_glm_laplace import DIMS, ROWS, TOL, the_prior
from tests.test_gpu_glm_pointwise import garbage_in_padding, same_bits

pytestmark = pytest.mark.gpu

SAFE = -1e100
GUARD = 16
SENTINEL = -7.75


def split(out, D):
    out = np.asarray(out)
    return float(out[0]), out[1:1 + D].copy(), out[1 + D:].reshape(D, D).copy()


def share(err, bound):
    """the largest err / bound (0 / 0 counts as 0)"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.max(np.where(err == 0.0, 0.0, err / bound)))


def theta_for(D, n):
    return np.random.RandomState(1000 * D + n).uniform(-1.0, 1.0, D)


def dev_f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def guarded(size):
    return torch.full((size + GUARD,), SENTINEL, dtype=torch.float64, device='cuda')


def untouched(buf, size):
    return bool(torch.all(buf[size:] == SENTINEL))


# ---- 1. the curvature against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', DIMS)
def test_curvature_within_the_bounds(D, family):
    from nnest_amd import _lib, flow
    worst = [0.0, 0.0, 0.0]
    for n in ROWS + ([1000] if D in (5, 65) else []):
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        theta = theta_for(D, n)
        out = flow.glm_curvature(data, theta).cpu().numpy()
        logl, g, H = split(out, D)
        el, eg, eH = nk.exact(data, theta)
        bl, bg, bH = nk.curvature_bounds(data, theta)
        shares = (share(abs(float(logl - el)), bl), share(np.abs((g - eg).astype(np.float64)), bg),
                  share(np.abs((H - eH).astype(np.float64)), bH))
        worst = [max(a, b) for a, b in zip(worst, shares)]
        assert max(shares) <= 1.0, (n, shares)
        assert same_bits(H, H.T), n
        assert same_bits(flow.glm_curvature(garbage_in_padding(data), theta).cpu().numpy(), out), n
        if n == 1000:   # (more than one row group: the merge has something to merge)
            assert _lib.load().nnest_glm_curv_groups(n, D) >= 2
    print('D=%d %s: worst shares of the bounds: logL %.3g, gradient %.3g, Hessian %.3g' % ((D, family) + tuple(worst)))


def test_groups():
    from nnest_amd import _lib
    lib = _lib.load()
    assert lib.nnest_glm_curv_groups(1, 1) == 1 and lib.nnest_glm_curv_groups(64, 128) == 1 and lib.nnest_glm_curv_groups(65, 5) == 2
    assert lib.nnest_glm_curv_groups(65536, 128) >= 2
    for n, D in ((0, 5), (65537, 5), (10, 0), (10, 129)):
        assert lib.nnest_glm_curv_groups(n, D) == -1


# ---- 2. the same call twice; nothing behind the buffers is written ---------------------------------------------------------------------
def raw_calls(data, theta, prior_data):
    """both entries through the raw library on guarded buffers: (out, partials, step, chol, info, sizes)"""
    from nnest_amd import _lib, flow
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    D = len(theta)
    spec, keep = flow.glm_spec(data, dev)
    G = lib.nnest_glm_curv_groups(int(data['n']), D)
    sizes = (1 + D + D * D, G * (1 + D + D * (D + 1) // 2), D, D * D, 4)
    bufs = [guarded(s) for s in sizes]
    th = dev_f64(theta)
    st = _lib.current_stream(dev)
    _lib.check(lib.nnest_glm_curv(ctypes.byref(spec), _lib.ptr(th), _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), D, st))
    pspec, pkeep = flow.gauss_prior_spec(prior_data, dev) if prior_data is not None else (None, None)
    _lib.check(lib.nnest_glm_newton_solve(_lib.ptr(bufs[0]), ctypes.byref(pspec) if pspec is not None else None, _lib.ptr(th),
                                          _lib.ptr(bufs[2]), _lib.ptr(bufs[3]), _lib.ptr(bufs[4]), D, st))
    torch.cuda.synchronize()
    return bufs, sizes


@pytest.mark.parametrize('D,n,family', [(5, 70, 'logistic'), (65, 1000, 'poisson'), (128, 200, 'logistic'), (33, 17, 'poisson')])
def test_twice_the_same_bits_and_guards(D, n, family):
    data = gk.make_like(D, n, family, D + n).hip_like_glm
    prior = the_prior(D).hip_gauss_prior
    theta = theta_for(D, n)
    first, sizes = raw_calls(data, theta, prior)
    second, _ = raw_calls(data, theta, prior)
    for a, b, size, what in zip(first, second, sizes, ('out', 'partials', 'step', 'chol', 'info')):
        assert untouched(a, size) and untouched(b, size), what
        assert same_bits(a[:size].cpu().numpy(), b[:size].cpu().numpy()), what
        assert bool(torch.all(torch.isfinite(a[:size]))), what
    assert float(first[4][3]) == 0.0


# ---- 3. a non-finite coordinate --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_theta(bad, family):
    from nnest_amd import flow
    for D, n, k in ((5, 70, 3), (65, 200, 64), (128, 1000, 0)):
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        theta = theta_for(D, n)
        theta[k] = bad
        curv = flow.glm_curvature(data, theta)
        assert float(curv[0]) == SAFE
        for prior in (None, the_prior(D).hip_gauss_prior):
            step, chol, info = flow.glm_newton_solve(curv, theta, prior=prior)
            info = info.cpu().numpy()
            assert info[3] == 2.0 and info[0] == SAFE and info[1] == 0.0 and info[2] == 0.0
            assert bool(torch.all(step == 0.0)) and bool(torch.all(chol == 0.0))


# ---- 4. the solve against a longdouble Cholesky solve ----------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', DIMS)
def test_solve_within_the_bounds(D, family):
    from nnest_amd import flow
    worst = [0.0, 0.0, 0.0, 0.0, 0.0]
    for n, with_prior in ((200, False), (200, True), (70, True), (1, True)):
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        prior = the_prior(D).hip_gauss_prior if with_prior else None
        theta = theta_for(D, n)
        curv = flow.glm_curvature(data, theta)
        step, chol, info = (t.cpu().numpy() for t in flow.glm_newton_solve(curv, theta, prior=prior))
        logl, g, H = split(curv.cpu().numpy(), D)
        ref = nk.newton(g, H, theta, prior)
        assert info[3] == 0.0 and np.isfinite(ref['step_rel']) and np.isfinite(ref['logdet_abs']), (n, with_prior, ref['kappa'])
        Hp = ref['H'].astype(np.float64)
        # (Higham, Theorem 10.3: the computed factor is the exact one of a matrix within D gamma_{D + 1} ||H||_2 of H)
        back = np.linalg.norm(chol @ chol.T - Hp, 2) / (D * nk.gamma(D + 1.0) * np.linalg.norm(Hp, 2) + 2 * nk.U * np.linalg.norm(Hp, 2))
        shares = (share(np.linalg.norm((step - ref['step']).astype(np.float64)), ref['step_rel'] * ref['step_norm']),
                  share(abs(float(info[2] - ref['logdet'])), ref['logdet_abs']),
                  share(abs(float(info[1] - ref['decrement'])), ref['decrement_abs']),
                  share(abs(float(info[0] - (nk.LD(logl) + ref['logpi']))), ref['logpi_abs'] + 2 * nk.U * abs(float(info[0]))),
                  float(back))
        worst = [max(a, b) for a, b in zip(worst, shares)]
        assert max(shares) <= 1.0, (n, with_prior, shares)
        assert np.all(np.triu(chol, 1) == 0.0) and np.all(np.diag(chol) > 0.0)
    print('D=%d %s: worst shares of the bounds: step %.3g, log det %.3g, decrement %.3g, log posterior %.3g, factor %.3g'
          % ((D, family) + tuple(worst)))


@pytest.mark.parametrize('D,n', [(5, 1), (33, 17), (64, 63), (128, 70)])
def test_singular_curvature_is_status_one(D, n):
    """n < D without a prior: H has rank n at most.  The input is legal, and the status is what it is for"""
    from nnest_amd import flow
    for family in gk.FAMILIES:
        data = gk.make_like(D, n, family, D + n).hip_like_glm
        theta = theta_for(D, n)
        curv = flow.glm_curvature(data, theta)
        step, chol, info = flow.glm_newton_solve(curv, theta)
        info = info.cpu().numpy()
        assert info[3] == 1.0 and info[0] == float(curv[0]) and info[1] == 0.0 and info[2] == 0.0
        assert bool(torch.all(step == 0.0)) and bool(torch.all(chol == 0.0))
        with pytest.raises(ValueError, match='GaussianPrior'):
            gk.make_like(D, n, family, D + n).laplace(route='fused')


# ---- 5. the fused route against the host route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', gk.FAMILIES)
@pytest.mark.parametrize('D', DIMS)
def test_fused_route_against_host(D, family):
    prior = the_prior(D)
    worst = [0.0, 0.0, 0.0]
    for n in ROWS:
        like = gk.make_like(D, n, family, D + n)
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            f, h = like.laplace(prior=prior, route='fused'), like.laplace(prior=prior, route='host')
        assert f.converged and h.converged and f.route == 'fused' and h.route == 'host'
        decs = [nk.decrement(like.hip_like_glm, prior.hip_gauss_prior, fit.mode) for fit in (f, h)]
        assert max(decs) <= 2 * TOL, (n, decs)
        # f(theta) - f* <= lambda^2 near the optimum and strong convexity, (lam_min / 2) |theta - theta*|^2 <= f(theta) - f*: each mode
        # is within sqrt(2 tol / lam_min) of the optimum, the two within twice that; a factor 2 to spare
        lam_min = np.linalg.eigvalsh(h.precision)[0]
        b_mode = 4.0 * np.sqrt(2.0 * TOL / lam_min)
        b_logz = 2.0 * TOL + nk.curvature_bounds(like.hip_like_glm, f.mode)[0] + nk.logdet_bound(f.precision)
        shares = (np.linalg.norm(f.mode - h.mode) / b_mode, abs(f.logz - h.logz) / b_logz, max(decs) / (2 * TOL))
        worst = [max(a, b) for a, b in zip(worst, shares)]
        assert shares[0] <= 1.0 and shares[1] <= 1.0, (n, shares)
        assert f.iterations <= 10 and same_bits(f.precision, f.precision.T)
    print('D=%d %s: worst shares: mode distance %.3g, log Z %.3g, restated decrement %.3g' % ((D, family) + tuple(worst)))


def test_default_route_is_fused_and_the_line_search_runs():
    like = gk.make_like(5, 200, 'logistic', 3)
    fit = like.laplace(theta0=np.full(5, 6.0))
    ref = like.laplace(route='host', theta0=np.full(5, 6.0))
    assert fit.route == 'fused' and fit.converged and fit.halvings >= 1 and fit.logz is None
    assert (fit.iterations, fit.halvings) == (ref.iterations, ref.halvings)
    assert np.linalg.norm(fit.mode - ref.mode) <= 4.0 * np.sqrt(2.0 * TOL / np.linalg.eigvalsh(ref.precision)[0])


# ---- 6. the front end ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def front_end_truth():
    from nnest_amd.priors import GaussianPrior
    from tests.test_gpu_mcmc_glm_prior import quadrature
    like = gk.make_like(2, 40, 'logistic', 5)
    prior = GaussianPrior(2, 0.0, 2.0)
    return like, prior, quadrature(like, prior, -20.0, 20.0)   # (ten sigma of the prior)


@pytest.mark.parametrize('flow_name', ['nvp', 'spline'])
def test_mcmc_front_end_from_a_laplace_fit(tmp_path, flow_name):
    """test_mcmc_front_end of tests/test_gpu_mcmc_glm_prior.py with the Laplace fit's draws in the place of its hand-written Newton loop"""
    import nnest_amd
    like, prior, (_, mean, cov) = front_end_truth()
    fit = like.laplace(prior=prior)
    assert fit.converged and fit.route == 'fused'
    N, S, A = 64, 600, 100
    train = fit.sample(2000, seed=3)
    init = (train[:N] - train.mean(0)) / train.std(0)
    np.random.seed(1)
    torch.manual_seed(1)
    s = nnest_amd.MCMCSampler(2, like, prior=prior, log_dir=str(tmp_path), log_level=30, flow=flow_name)
    s.run(S, N, train, init_samples=init, route='fused', seed=1, adapt_steps=A, global_every=5)
    assert s.mcmc_route == 'fused'
    x = s.samples[:, A + 1:, :].astype(np.float64)
    m = x.mean(1)
    se = m.std(0, ddof=1) / np.sqrt(N)
    off = np.abs(m.mean(0) - mean) / se
    print('%s: posterior mean off by at most %.2f standard errors (largest standard error %.3g)' % (flow_name, off.max(), se.max()))
    assert np.all(off <= 5.0), off


def test_laplace_evidence_against_quadrature(caplog):
    import logging
    from nnest_amd import evaluation
    like, prior, (logz, _, _) = front_end_truth()
    with caplog.at_level(logging.INFO, logger='nnest_amd.evaluation'):
        out = evaluation.laplace_evidence(like, prior)
    print('Laplace log Z %.4f, quadrature %.4f' % (out['logz'], logz))
    assert out['converged'] and out['fit'].route == 'fused' and abs(out['logz'] - logz) <= 0.05
    assert any(rec.getMessage().startswith('Laplace: log Z [') for rec in caplog.records)


# ---- argument errors leave the outputs alone -------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_alone():
    from nnest_amd import _lib, flow
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    D, n = 5, 70
    data = gk.make_like(D, n, 'logistic', 1).hip_like_glm
    spec, keep = flow.glm_spec(data, dev)
    pspec, pkeep = flow.gauss_prior_spec(the_prior(D).hip_gauss_prior, dev)
    th = dev_f64(theta_for(D, n))
    out, partials, step, chol, info = (guarded(s) for s in (1 + D + D * D, 1 + D + D * (D + 1) // 2, D, D * D, 4))
    st = _lib.current_stream(dev)
    p = _lib.ptr

    def refused(rc, needle):
        torch.cuda.synchronize()
        assert rc != _lib.NNEST_OK and needle in lib.nnest_hip_last_error().decode(), (rc, lib.nnest_hip_last_error())
        for buf in (out, partials, step, chol, info):
            assert bool(torch.all(buf == SENTINEL))

    refused(lib.nnest_glm_curv(None, p(th), p(out), p(partials), D, st), 'NULL')
    refused(lib.nnest_glm_curv(ctypes.byref(spec), None, p(out), p(partials), D, st), 'NULL')
    refused(lib.nnest_glm_curv(ctypes.byref(spec), p(th), None, p(partials), D, st), 'NULL')
    refused(lib.nnest_glm_curv(ctypes.byref(spec), p(th), p(out), None, D, st), 'NULL')
    refused(lib.nnest_glm_curv(ctypes.byref(spec), p(th), p(out), p(partials), D + 1, st), 'D=')
    bad = _lib.GlmSpec(spec.at_dev, spec.y_dev, spec.o_dev, spec.logl0, spec.n, spec.ld, spec.D, 2)
    refused(lib.nnest_glm_curv(ctypes.byref(bad), p(th), p(out), p(partials), D, st), 'family')
    for args in ((None, None, p(th), p(step), p(chol), p(info)), (p(out), None, None, p(step), p(chol), p(info)),
                 (p(out), None, p(th), None, p(chol), p(info)), (p(out), None, p(th), p(step), None, p(info)),
                 (p(out), None, p(th), p(step), p(chol), None)):
        refused(lib.nnest_glm_newton_solve(*(args + (D, st))), 'NULL')
    refused(lib.nnest_glm_newton_solve(p(out), None, p(th), p(step), p(chol), p(info), 0, st), 'D=')
    refused(lib.nnest_glm_newton_solve(p(out), None, p(th), p(step), p(chol), p(info), 129, st), 'D=')
    refused(lib.nnest_glm_newton_solve(p(out), ctypes.byref(pspec), p(th), p(step), p(chol), p(info), D + 1, st), 'D=')
