"""CPU pins of the float64 spline oracle (oracle/spline_grad.py) that the GPU training tests of the spline flow are held to:
its log-probs equal the C oracle's float64 log-probs at every shape of the GPU tables (tail rows and saturated logits included),
its gradient equals the reference's autograd gradients in tests/golden/spline_*.npz tensor by tensor, and the per-tensor
comparator (tests/spline_grad_check.py) rejects errors that the old whole-vector criterion lets through."""
import glob
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import spline_grad as sg
from tests import spline_grad_check as sgc

G = os.path.join(os.path.dirname(__file__), 'golden')
FILES = sorted(glob.glob(os.path.join(G, 'spline_*.npz')))
IDS = [os.path.basename(p)[7:-4] for p in FILES]
SHAPES = sorted(set([(D, H, B) for D, H, B, _ in sgc.ROWS_TABLE + sgc.TILES_TABLE] +
                    [(D, H, B) for D, H, B, _, _ in sgc.VJP_TABLE]))


def initialised(D, H, B, seed, n=64):
    """fresh weights with the ActNorm data-dependent initialisation (C oracle) on n rows of sgc.make_rows"""
    w, P = sgc.random_weights(D, H, B, seed=seed)
    rng = np.random.RandomState(seed)
    X = sgc.make_rows(rng, n, D)
    o = orc.Spline(D, H, B, 8, 3.0, w, P)
    o.forward(X, data_init=True)
    return o, X


@pytest.mark.parametrize('D,H,B', SHAPES, ids=['d%d_h%d_b%d' % s for s in SHAPES])
def test_log_probs_equal_the_c_oracle(D, H, B):
    o, X = initialised(D, H, B, seed=D + 7 * B)
    shapes = sg.layer_shapes(D, H, B, 8)
    assert sg.num_params(D, H, B, 8) == o.n
    for tag, w in (('plain', o.w), ('saturated', sgc.saturate(o.w, shapes))):
        st = {}
        lp, loss = sg.log_probs(w, o.P, X, D, H, B, stats=st)
        oc = orc.Spline(D, H, B, 8, 3.0, w, o.P)
        lpc, lossc = oc.log_probs(X, f64=True)
        assert np.all(np.isfinite(lp)), tag
        assert np.max(np.abs(lp - lpc) / np.maximum(np.abs(lpc), 1.0)) <= 1e-11, tag
        assert abs(loss - lossc) <= 1e-11 * max(abs(lossc), 1.0), tag
        assert st['n_tail'] > 0, tag                       # rows in the linear tails
        if tag == 'saturated':
            assert st['max_logit'] > 20, st                # past softplus's threshold, softmax saturated


def fixture_grads(g):
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    for k in range(2):
        w = g['w_init'] if k == 0 else g['ws'][0]
        sl = slice(100 * k, 100 * (k + 1))        # (as test_gpu_spline.py::test_loss_and_gradient_vs_reference_autograd)
        data = g['X'][g['perms'][0][sl]] + np.float32(g['jitter']) * g['noises'][0][sl]
        yield k, w, data, D, H, B, K


# the reference computes in float32: its autograd gradient is within ~1e-5 of each tensor's scale of the float64 one (measured
# worst: 7e-4 of the scale of flow.flows.4.L at spline_d2 step 1, a tensor 500x below the largest; 1.6e-6 of the largest there)
REF_RTOL_T, REF_FLOOR = 1e-3, 5e-6


@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_gradient_equals_the_reference_autograd(path):
    g = np.load(path)
    for k, w, data, D, H, B, K in fixture_grads(g):
        shapes = sg.layer_shapes(D, H, B, K)
        assert [n for n, _ in shapes] == [str(s) for s in g['keys']]
        loss, g64 = sg.loss_grad(w, g['P'], data, D, H, B, K, float(g['tail']))
        assert abs(loss - g['losses'][k]) < 2e-6 * (1 + abs(g['losses'][k]))
        worst = sgc.assert_grad_close(g['grads'][k], g64, shapes, REF_RTOL_T, REF_FLOOR, '%s step %d' % (IDS[FILES.index(path)], k))
        print('%s step %d: worst error / bound %.3g' % (path, k, worst))


def test_comparator_power():
    """on the fixture gradient (spline_d5, step 0): a 1 % error in one small tensor (each of the three with the smallest gradients,
    ~1 % of the largest) and the gradient of a minibatch with one row
    dropped are rejected per tensor; the old whole-vector criterion accepts the first"""
    g = np.load(os.path.join(G, 'spline_d5.npz'))
    k, w, data, D, H, B, K = next(fixture_grads(g))
    shapes = sg.layer_shapes(D, H, B, K)
    sl = sgc.tensor_slices(shapes)
    g64 = sg.loss_grad(w, g['P'], data, D, H, B, K, float(g['tail']))[1]
    gref = g['grads'][0].astype(np.float64)
    sgc.assert_grad_close(gref, g64, shapes, REF_RTOL_T, REF_FLOOR)
    assert sgc.whole_vector_ok(gref, g64)
    top = np.max(np.abs(g64))
    small = sorted(sl, key=lambda n: np.max(np.abs(g64[sl[n]])))[:3]    # flows.5.f1.net.0.bias, flows.8.f1.net.0.bias / .weight
    for name in small:
        assert np.max(np.abs(g64[sl[name]])) < 0.02 * top, name         # ~1 % of the largest gradient
        bad = gref.copy()
        bad[sl[name]] *= 1.01
        assert sgc.whole_vector_ok(bad, g64), name                      # the old criterion does not see it
        with pytest.raises(AssertionError, match=name.replace('.', r'\.')):
            sgc.assert_grad_close(bad, g64, shapes, REF_RTOL_T, REF_FLOOR)
    dropped = sg.loss_grad(w, g['P'], data[1:], D, H, B, K, float(g['tail']))[1]
    with pytest.raises(AssertionError):
        sgc.assert_grad_close(dropped, g64, shapes, REF_RTOL_T, REF_FLOOR)


def test_vjp_is_the_gradient_of_its_scalar():
    """vjp with gz = z/M and gld = -1/M is the gradient of the training loss (N(0,I) base: log p = -|z|^2/2 + logdet + c); dL/dx
    against central differences of the float64 forward"""
    import torch
    D, H, B = 5, 10, 2
    o, X = initialised(D, H, B, seed=3, n=16)
    z, _ = sg.forward(torch.tensor(o.w.astype(np.float64)), o.P, torch.tensor(X.astype(np.float64)), D, H, B, 8, 3.0)
    M = X.shape[0]
    gw, gx = sg.vjp(o.w, o.P, X, D, H, B, 8, 3.0, z.numpy() / M, -1.0 / M)
    np.testing.assert_allclose(gw, sg.loss_grad(o.w, o.P, X, D, H, B)[1], rtol=1e-10, atol=1e-12)
    rng = np.random.RandomState(0)
    gz, gld = rng.randn(M, D), 0.7

    def L(x):
        with torch.no_grad():
            zz, ld = sg.forward(torch.tensor(o.w.astype(np.float64)), o.P, torch.tensor(x), D, H, B, 8, 3.0)
        return float((zz.numpy() * gz).sum() + gld * ld.sum())
    gw, gx = sg.vjp(o.w, o.P, X, D, H, B, 8, 3.0, gz, gld)
    x0, h = X.astype(np.float64), 1e-6
    for (r, c) in ((0, 0), (3, 4), (11, 2)):
        xp, xm = x0.copy(), x0.copy()
        xp[r, c] += h
        xm[r, c] -= h
        assert abs((L(xp) - L(xm)) / (2 * h) - gx[r, c]) < 1e-6 * (1 + abs(gx[r, c]))


def test_adam_is_torch_adam():
    import torch
    rng = np.random.RandomState(1)
    w0 = rng.randn(50)
    p = torch.nn.Parameter(torch.tensor(w0))
    opt = torch.optim.Adam([p], lr=1e-3, weight_decay=1e-6)
    ws, gs = [], []
    for i in range(4):
        gi = rng.randn(50) * (0.1 if i % 2 else 1.0)
        ws.append(p.detach().numpy().copy())
        gs.append(gi)
        p.grad = torch.tensor(gi)
        opt.step()
        np.testing.assert_allclose(sg.adam(ws, gs, 1e-3, 1e-6), p.detach().numpy(), rtol=0, atol=1e-15)


def test_spline_loss_grad_and_fd_grad_agree():
    """oracle.Spline.loss_grad (this module) against the C oracle's float64 finite differences"""
    g = np.load(os.path.join(G, 'spline_d5.npz'))
    k, w, data, D, H, B, K = next(fixture_grads(g))
    o = orc.Spline(D, H, B, K, float(g['tail']), w, g['P'])
    loss, grad = o.loss_grad(data)
    assert abs(loss - o.log_probs(data, f64=True)[1]) < 1e-12 * (1 + abs(loss))
    idx = np.argsort(-np.abs(grad))[:40:4]
    err = np.abs(o.fd_grad(data, idx) - grad[idx]) / np.max(np.abs(grad))
    # central differences of a piecewise-smooth loss (LeakyReLU kinks, bin edges): exact to O(h^2) unless a row crosses a kink
    # within +-h, then O(h) off
    assert np.sum(err < 1e-6) >= len(idx) // 2 and np.max(err) < 1e-3, err
