"""CPU checks of the ensemble sampler's definition (tests/ensemble_check.py restates nnest_ensemble_steps): the restated stretch move
keeps an exactly sampled target, the invariance statistics reject two wrong moves (so the GPU invariance tests can fail), and the
front-end refuses fewer than 2 D walkers as emcee does."""
import numpy as np
import pytest

from tests.ensemble_check import latent_target, numpy_draws, stretch_run
from tests.slice_invariance import ALPHA, assert_invariant, min_corrected_p, stationarity_pvalues

D, N, S = 3, 6000, 40
RHO, SIG = 0.5, 0.6


def gauss_logl(x):
    """equicorrelated Gaussian, correlation RHO, scale SIG"""
    x = np.asarray(x, np.float64) / SIG
    s1, s2 = x.sum(1), (x * x).sum(1)
    return -0.5 * (s2 - RHO * s1 * s1 / (1.0 + (D - 1) * RHO)) / (1.0 - RHO)


def in_box(x):
    return np.all(np.abs(np.asarray(x, np.float64)) <= 1.0, axis=1)


def exact(rng, n):
    """n draws of the Gaussian truncated to [-1, 1]^D, by rejection (float64)"""
    cov = SIG * SIG * ((1 - RHO) * np.eye(D) + RHO * np.ones((D, D)))
    out, have = [], 0
    while have < n:
        x = rng.multivariate_normal(np.zeros(D), cov, size=4 * n)
        x = x[in_box(x)]
        out.append(x)
        have += len(x)
    return np.concatenate(out)[:n]


# toy flows x = f^-1(z): affine, and an elementwise sinh after an affine map (a log-det that varies with z)
L = np.array([[1.2, 0.0, 0.0], [0.3, 0.8, 0.0], [-0.2, 0.4, 1.5]])
B = np.array([0.1, -0.2, 0.05])
C = 2.0


def affine_inv(z):
    z = np.asarray(z, np.float64)
    return z @ L.T + B, np.full(len(z), np.log(abs(np.linalg.det(L))))


def affine_fwd(x):
    return np.linalg.solve(L, (np.asarray(x) - B).T).T


def sinh_inv(z):
    y, ld = affine_inv(z)
    return np.sinh(C * y) / C, ld + np.sum(np.log(np.cosh(C * y)), axis=1)


def sinh_fwd(x):
    return affine_fwd(np.arcsinh(C * np.asarray(x)) / C)


FLOWS = {'identity': (lambda z: (np.asarray(z, np.float64), np.zeros(len(z))), lambda x: x),
         'affine': (affine_inv, affine_fwd), 'sinh': (sinh_inv, sinh_fwd)}


def run_move(flow, seed, jacobian=None, logdet_sign=1.0):
    inv, fwd = FLOWS[flow]
    rng = np.random.RandomState(seed)
    x0 = exact(rng, N)
    z0 = fwd(x0).astype(np.float32)
    lp_fn = latent_target(inv, gauss_logl, in_box, logdet_sign=logdet_sign)
    lp0 = lp_fn(z0)
    assert np.all(np.isfinite(lp0))
    z, _, _, _ = stretch_run(z0, lp0, numpy_draws(rng, N, S), lp_fn, jacobian)
    x, _ = inv(z)
    return stationarity_pvalues(x, exact(rng, N))


@pytest.mark.parametrize('flow', ['identity', 'affine', 'sinh'])
def test_restated_move_keeps_its_target(flow):
    assert_invariant(run_move(flow, 11), what='stretch move, %s flow' % flow)


def test_statistics_reject_the_wrong_jacobian_factor():
    p = run_move('identity', 12, jacobian=D)
    assert min_corrected_p(p) <= ALPHA, p


def test_statistics_reject_the_flipped_logdet():
    p = run_move('sinh', 13, logdet_sign=-1.0)
    assert min_corrected_p(p) <= ALPHA, p


def test_fewer_than_two_d_walkers_refused():
    from nnest_amd.ensemble import EnsembleSampler
    s = EnsembleSampler.__new__(EnsembleSampler)   # (no flow: the check comes first, as emcee's)
    s.x_dim, s.num_derived = 5, 0
    with pytest.raises(RuntimeError, match='fewer walkers than twice the number of dimensions'):
        s._ensemble_sample(10, 9)
    with pytest.raises(RuntimeError, match='fewer walkers than twice the number of dimensions'):
        s._ensemble_sample(10, None, init_samples=np.zeros((4, 5)))
