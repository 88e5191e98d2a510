"""tests/cholesky_check.py on the CPU: the closed-form gradient of the 'choleksy' flow pinned to the reference's autograd gradients
(tests/golden/cholesky_*.npz grads[0]) tensor by tensor, its passes to the numpy oracle's, and its float32 evaluation through the
checker the GPU kernels are held to (tests/nvp_vjp_check.py assert_vjp_close)."""
import glob
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import cholesky_check as cc
from tests import nvp_train_check as ntc
from tests import nvp_vjp_check as vc

FILES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'cholesky_*.npz')))


@pytest.mark.parametrize('path', FILES, ids=[os.path.basename(p)[9:-4] for p in FILES])
def test_closed_form_gradient_vs_the_references_autograd(path):
    """the fixture is the reference's float32 evaluation: held to R from this module's float32 evaluation (the checker's rule)"""
    g = np.load(path)
    D = int(g['D'])
    data = g['X'][g['perms'][0][:100]] + np.float32(float(g['jitter'])) * g['noises'][0][:100]
    loss, grad = cc.loss_grad(g['w0'], data, D)
    _, g32 = cc.loss_grad(g['w0'], data, D, dt=np.float32)
    assert abs(loss - float(g['losses'][0])) < 1e-6 * (1 + abs(loss))
    R = vc.rtol(g32, None, grad, None, cc.shapes(D))
    assert R == ntc.BOUNDS['rtol_min']
    vc.assert_vjp_close(g['grads'][0], None, grad, None, cc.shapes(D), R, None, os.path.basename(path))
    o = orc.Cholesky(D, g['w0'])
    y, ld = cc.forward(g['w0'], g['x'], D)
    assert np.max(np.abs(y - o.forward(g['x'], f64=True)[0])) < 1e-9 and np.max(np.abs(cc.log_probs(g['w0'], g['x'], D) - g['lp'])) < 2e-5 * (
        1 + np.max(np.abs(g['lp'])))
    x, ldi = cc.inverse(g['w0'], g['z'], D)
    assert np.max(np.abs(x - g['xb'])) < 1e-5 * (1 + np.max(np.abs(x))) and np.all(ld + ldi == 0)


@pytest.mark.parametrize('D', [1, 2, 33, 128])
def test_gradient_against_a_finite_difference_and_the_float32_reach(D):
    """every tensor's largest-gradient element against a central difference of the loss in float64, both bases; and the float32
    evaluation inside the checker with R no more than its cap"""
    w = cc.case_weights(D)
    assert w[-D:].min() == -3 and (D == 1 or w[-D:].max() == 25)
    X = np.random.RandomState(D).uniform(-1, 1, size=(37, D)).astype(np.float32)
    for beta in (0.0, 8.0):
        loss, grad, terms = cc.loss_grad(w, X, D, beta, terms=True)
        _, g32 = cc.loss_grad(w, X, D, beta, dt=np.float32)
        assert terms.shape == (D * (D - 1) // 2,) and np.all(terms >= np.abs(grad[D:D + terms.size]) * (1 - 1e-12))
        R = vc.rtol(g32, None, grad, None, cc.shapes(D))
        assert R <= vc.R_CAP
        vc.assert_vjp_close(g32, None, grad, None, cc.shapes(D), R, None, 'd%d beta %g' % (D, beta))
        for name, s in vc._slices(cc.shapes(D)):
            if s.stop == s.start:
                continue
            i = s.start + int(np.argmax(np.abs(grad[s])))
            h = 1e-3 * max(1.0, abs(float(w[i])))        # float32 weights: a step that float32 represents, taken exactly
            wp, wm = w.copy(), w.copy()
            wp[i], wm[i] = np.float32(w[i] + h), np.float32(w[i] - h)
            step = float(wp[i]) - float(wm[i])
            fd = (cc.loss_grad(wp, X, D, beta)[0] - cc.loss_grad(wm, X, D, beta)[0]) / step
            # truncation h^2 f''' / 6: the loss is a polynomial of degree <= 8 in a bias or lower entry, smooth in u
            assert abs(fd - grad[i]) < 2e-4 * abs(grad[i]), (name, fd, grad[i])


def test_float32_inverse_is_forward_substitution():
    D = 33
    w = cc.case_weights(D)
    X = np.random.RandomState(2).uniform(-1, 1, size=(65, D)).astype(np.float32)
    z = cc.forward(w, X, D)[0].astype(np.float32)
    x64 = cc.inverse(w, z, D)[0]
    assert np.max(np.abs(cc.inverse32(w, z, D) - x64) / (1 + np.abs(x64))) < 1e-5


def test_float32_round_trip_is_the_recorded_one():
    """what float32 loses on inverse(forward(x)) over the rows of the GPU test: below the passes' 1e-5 up to x_dim 33, F32_ROUND_TRIP_128
    (within a factor 2: another BLAS sums in another order) at x_dim 128 -- the figure the GPU test's round-trip bound and its cap
    are derived from; the float32 inverse itself stays at 1e-5 of the float64 inverse of the same z at every x_dim"""
    for D in (1, 2, 33, 128):
        w = cc.case_weights(D)
        worst = max(cc.round_trip32(w, X, D) for _, X in cc.pass_rows(D))
        print('x_dim %d: float32 round trip %.3g' % (D, worst))
        if D < 128:
            assert worst < 1e-5, (D, worst)
        else:
            assert cc.F32_ROUND_TRIP_128 / 2 <= worst <= 2 * cc.F32_ROUND_TRIP_128, worst
        for _, X in cc.pass_rows(D)[:4]:
            z = cc.forward(w, X, D)[0].astype(np.float32)
            x64 = cc.inverse(w, z, D)[0]
            assert np.max(np.abs(cc.inverse32(w, z, D) - x64) / (1 + np.abs(x64))) < 1e-5, D
    assert cc.ROUND_TRIP_CAP == 20 * cc.F32_ROUND_TRIP_128
