"""GPU parity for the 'choleksy' flow (reference SingleSpeedCholeksy, networks.py:162-239): passes, every gradient element and
Adam steps against fixtures produced by the reference (tests/golden/cholesky_*.npz), and a nested-sampling run on it."""
import glob
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import oracle as orc  # noqa: E402  (checker only)

G = os.path.join(os.path.dirname(__file__), 'golden')
FILES = sorted(glob.glob(os.path.join(G, 'cholesky_*.npz')))


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('path', FILES, ids=[os.path.basename(p)[9:-4] for p in FILES])
def test_cholesky_vs_reference_fixture(path):
    from nnest_amd.cholesky import HipCholesky
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    g = np.load(path)
    D = int(g['D'])
    net = HipCholesky(D)
    assert list(net.state_dict().keys()) == [str(k) for k in g['keys']]
    ident, _ = net.forward(g['x'])
    assert rel(cpu(ident), g['x']) < 2e-6                 # identity initialisation (networks.py:183-189)
    net.load_packed(g['w0'])
    z, ld = net.forward(g['x'])
    assert rel(cpu(z), g['z']) < 1e-5 and rel(cpu(ld), g['ldf']) < 1e-5
    xb, ldi = net.inverse(g['z'])
    assert rel(cpu(xb), g['xb']) < 1e-5 and rel(cpu(ldi), g['ldi']) < 1e-5
    assert rel(cpu(net.log_probs(g['x'])), g['lp']) < 2e-5
    o = orc.Cholesky(D, g['w0'])
    assert rel(cpu(net.inverse(g['z'])[0]), o.inverse(g['z'], f64=True)[0]) < 1e-5
    X, jitter = g['X'], float(g['jitter'])
    data = X[g['perms'][0][:100]] + np.float32(jitter) * g['noises'][0][:100]
    loss, grad = net.loss_grad(data)
    assert abs(float(loss) - g['losses'][0]) < 2e-5 * (1 + abs(g['losses'][0]))
    assert np.max(np.abs(cpu(grad) - g['grads'][0])) < 5e-5 * (1e-3 + np.max(np.abs(g['grads'][0])))
    res = net.train_epochs(X, X[:23], torch.from_numpy(g['perms'].astype(np.int64)), torch.from_numpy(g['noises']), jitter=jitter,
                           batch=100, max_epochs=2, patience=50)
    np.testing.assert_allclose(res['losses'].numpy()[:2, 0] * X.shape[0], g['losses'].reshape(2, -1).sum(axis=1), rtol=3e-5)
    if res['best_epoch'] == 2:
        dref, dour = g['ws'][-1] - g['w0'], net.store_packed() - g['w0']
        assert np.sqrt(np.mean((dour - dref) ** 2)) < 0.05 * np.sqrt(np.mean(dref ** 2))


def test_nested_run_on_the_cholesky_flow(tmp_path):
    from nnest_amd.likelihoods import Gaussian
    from nnest_amd.nested import NestedSampler
    np.random.seed(3)
    torch.manual_seed(3)
    like = Gaussian(2, 0.9, lim=3)
    s = NestedSampler(2, like, transform=lambda x: 3 * x, log_dir=str(tmp_path), num_live_points=300, log_level=30, flow='choleksy')
    assert type(s.trainer.netG).__name__ == 'HipCholesky' and s._fused_like_id is None
    s.run(mcmc_num_chains=20, train_iters=100, mcmc_steps=10)
    assert abs(s.logz - math.log(1 / 36.0)) <= 0.5, s.logz   # unit-mass Gaussian inside [-3, 3]^2 (up to ~1 % truncation)


# ---- against float64 at the sizes the fixtures do not reach -------------------------------------------------------------------------
PASS_RTOL = 1e-5          # this file's bound on the passes
LOSS_RTOL = 2e-5          # ... and on the loss


def _within(got, want, rtol=PASS_RTOL):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / (rtol * (1.0 + np.abs(want)))))


def _chol_adam_steps(net, w, grads, lr, wd, what):
    """nnest_chol_adam_step keeps its moments to itself: each w' is held to the float64 step from float64 moments carried here,
    within nvp_train_check's weight bound 2 ulp(w) + 64 eps32 |update| (the float32 moments are exact to 4 eps32 of their terms,
    far inside the 64)"""
    from tests import nvp_train_check as ntc
    m, v, worst = np.zeros(w.size), np.zeros(w.size), 0.0
    for k, g in enumerate(grads):
        net.adam_step(torch.from_numpy(g).to(net.device), lr, wd)
        w1 = net.store_packed()
        gi = g.astype(np.float64) + float(np.float32(wd)) * w.astype(np.float64)
        m, v = m + (gi - m) * ntc.C1, ntc.B2 * v + ntc.C2 * gi ** 2
        bc1, bc2 = 1.0 - 0.9 ** (k + 1), 1.0 - 0.999 ** (k + 1)
        update = (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + ntc.ADAM_EPS)
        tol = ntc.BOUNDS['w_ulps'] * ntc.ulp32(w) + ntc.BOUNDS['w_rel'] * np.abs(update)
        d = np.abs(w1.astype(np.float64) - (w.astype(np.float64) - update))
        i = int(np.argmax(d / tol))
        assert d[i] <= tol[i], '%s step %d: weight[%d] %.9g, the float64 step gives %.9g' % (what, k + 1, i, w1[i], (w - update)[i])
        worst, w = max(worst, float(d[i] / tol[i])), w1
    return worst


@pytest.mark.parametrize('D', [1, 2, 33, 128])
def test_cholesky_passes_and_gradient_vs_float64(D):
    """One thread per row (the passes) or per parameter (the gradient, which inverts the triangular index with a sqrtf) at x_dim 1,
    2, 33 and 128 -- 8128 lower entries --, rows 1 / 63 / 64 / 65 / 1000, minibatches 1 / 37 / 128, unconstrained_diag from -3 to 25
    (across the softplus switch at 20), both bases, against tests/cholesky_check.py in float64.  Gradients per tensor, relative to
    the tensor's largest entry, within R = max(3e-5, 10 x the float32 evaluation's own ratio) (tests/nvp_vjp_check.py)."""
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.distributions import GeneralisedNormal
    from tests import cholesky_check as cc
    from tests import nvp_vjp_check as vc
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    net = HipCholesky(D)
    w = cc.case_weights(D)
    net.load_packed(w)
    assert np.array_equal(net.store_packed(), w)
    rng = np.random.RandomState(70 + D)      # (the minibatches and the Adam gradients; the rows of the passes are cc.pass_rows)
    worst = {}
    # what float32 loses on inverse(forward(x)) at these weights, over all the rows of the passes (a property of L's conditioning, so
    # judged once per x_dim, not per batch of rows: a batch just under 1e-5 says nothing else about the next one)
    f32 = max(cc.round_trip32(w, X, D) for _, X in cc.pass_rows(D))
    rt = PASS_RTOL if f32 <= PASS_RTOL else 10.0 * f32
    assert rt <= cc.ROUND_TRIP_CAP and (D > 33 or rt == PASS_RTOL), (D, rt)
    for N, X in cc.pass_rows(D):
        z64, ld64 = cc.forward(w, X, D)
        z, ld = net.forward(X)
        worst['forward'] = max(worst.get('forward', 0), _within(cpu(z), z64), _within(cpu(ld), ld64))
        zin = z64.astype(np.float32)
        x64, ldi64 = cc.inverse(w, zin, D)
        xi, ldi = net.inverse(zin)
        worst['inverse'] = max(worst.get('inverse', 0), _within(cpu(xi), x64), _within(cpu(ldi), ldi64))
        worst['log_probs'] = max(worst.get('log_probs', 0), _within(cpu(net.log_probs(X)), cc.log_probs(w, X, D)))
        # inverse(forward(x)) = x.  What comes back is L^-1 of a float32 z: rounding z alone moves x by ulp(z) / diag, and diag goes
        # down to softplus(-3) + 1e-3 = 0.05 under a bias of order 1, so the float64 x is out of float32's reach at 1e-5 from x_dim
        # ~100 on (the float32 restatement, forward then forward substitution, measures 1.3e-5 at x_dim 128:
        # tests/test_cholesky_check.py::test_float32_round_trip_is_the_recorded_one).  The bound is 1e-5 wherever float32 reaches it,
        # else 10 x what the float32 restatement loses over the rows of the passes (the rule of nvp_vjp_check.py), and never above ROUND_TRIP_CAP:
        # an input on which float32 loses more than twice the recorded figure is not one this test accepts.
        xb, ldb = net.inverse(z)
        worst['round trip'] = max(worst.get('round trip', 0), _within(cpu(xb), X.astype(np.float64), rt))
        assert np.all(np.abs(cpu(ld).astype(np.float64) + cpu(ldb)) <= PASS_RTOL * (1 + np.abs(ld64)))       # the two log-dets cancel
        assert max(worst.values()) <= 1.0, (D, N, worst)
    shapes = cc.shapes(D)
    nl = D * (D - 1) // 2
    for beta, Ms in ((0.0, (1, 37, 128)), (8.0, (37,) if D == 33 else ())):
        net.set_base(GeneralisedNormal(torch.zeros(D), torch.ones(D), torch.tensor(beta)) if beta else None)
        for M in Ms:
            what = 'd%d m%d beta %g' % (D, M, beta)
            X = rng.uniform(-1, 1, size=(M, D)).astype(np.float32)
            loss, grad = net.loss_grad(X)
            g = cpu(grad).astype(np.float64)
            loss64, g64, terms = cc.loss_grad(w, X, D, beta, terms=True)
            _, g32 = cc.loss_grad(w, X, D, beta, dt=np.float32)
            assert abs(float(loss) - loss64) < LOSS_RTOL * (1 + abs(loss64)), (what, float(loss), loss64)
            R = vc.rtol(g32, None, g64, None, shapes)
            assert R <= vc.R_CAP, (what, R)
            worst['gradient'] = max(worst.get('gradient', 0), vc.assert_vjp_close(g, None, g64, None, shapes, R, None, what)[0])
            if beta:
                worst['log_probs beta 8'] = _within(cpu(net.log_probs(X)), cc.log_probs(w, X, D, beta))
                assert worst['log_probs beta 8'] <= 1.0
            if D == 128:
                # every lower entry (i, j) on its own: against the float64 sum over the rows of gy[r, i] x[r, j], relative to the sum
                # of the products' magnitudes -- what a float32 sum of that element can lose -- so that an entry far below its
                # tensor's largest is held too: the index inversion at every q
                lo = slice(D, D + nl)
                R_el = max(3e-5, 10 * float(np.max(np.abs(g32 - g64)[lo] / terms)))
                ratio = np.abs(g - g64)[lo] / (R_el * terms)
                q = int(np.argmax(ratio))
                i, j = (int(a[q]) for a in np.tril_indices(D, -1))
                assert ratio[q] <= 1.0, '%s: lower[%d] = (%d, %d): %.9g vs float64 %.9g (R %.3g)' % (what, q, i, j, g[lo][q], g64[lo][q], R_el)
                worst['lower entries'] = max(worst.get('lower entries', 0), float(ratio[q]))
    net.set_base(None)
    grads = [(rng.randn(w.size) * 10.0 ** rng.uniform(-6, 0, w.size)).astype(np.float32) for _ in range(2)]
    worst['adam'] = _chol_adam_steps(net, w, grads, 1e-3, 1e-6, 'd%d' % D)
    print('cholesky d%d worst error / bound: %s' % (D, '  '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
