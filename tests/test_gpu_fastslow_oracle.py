"""The fast/slow hierarchies (HipFastSlowNVP, HipFastSlowSpline: Trainer(num_slow=...)) against a float64 composite
(oracle/nvp_grad.py FastSlow; pinned on the CPU to the reference's autograd gradients by tests/test_nvp_vjp_check.py) at the edges of
fastslow.py's interleaving: one slow or one fast dimension, sixteen of either, unequal sides (the shorter one zero-padded, its
real-looking gradients nulled by the coupling mask).  The loss, every gradient tensor by tensor (tests/nvp_vjp_check.py: R from the
float32 composite on the same input, parameters the masks never reach exactly zero), the three stages' log-determinants, and one
optimiser step of _train_epoch.

R_step, measured on the first GPU run (test_fast_slow_one_adam_step prints it): the float32 composite taking the same first Adam step
on the CPU is off the float64 step by 6.2e-5 of a tensor's largest update at (S 1, F 16) and by 1.7e-4 at (S 7, F 9, 17 rows), hence
R_step = 10 x that, 6.2e-4 and 1.7e-3.  The first step of Adam is lr gi / (|gi| + 1e-8) with gi = g + wd w: +-lr for every parameter
whose gradient is far above 1e-8, where all that is left is half an ulp of a weight of order 1 against an update of 1e-3 (the 6.2e-5:
a parity-masked first-layer weight of -1.08, gradient exactly 0); where gi is small the step is steep in it -- at (7, 9) the worst
element has g64 = 9.7e-7 against wd w = -3.0e-7, and the float32 composite's gradient error of 8.6e-9 there moves the step by
1e-8 * 8.6e-9 / (6.7e-7)^2 = 1.7e-4 of lr.  The kernels' worst error / bound against those R_step: 0.10 and 0.41.
Run with  pytest -m gpu -s  to see the error / bound ratios."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import nvp_grad as ng  # noqa: E402  (checker only)
from oracle import spline_grad as sg  # noqa: E402
from tests import nvp_train_check as ntc  # noqa: E402
from tests import nvp_vjp_check as vc  # noqa: E402

LOSS_RTOL = 3e-5           # tests/test_gpu_fastslow.py's bound on the loss and the log-probabilities
KNOT_MARGIN = 1e-5         # tests/test_gpu_spline_grad.py MARGIN: rows whose spline inputs come this close to a knot are kept out
WORST = {}


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import fastslow
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    yield fastslow
    print('\nfastslow_oracle worst error / bound: ' + '  '.join('%s %.3g' % kv for kv in sorted(WORST.items())))


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print('%s: worst error / bound %.3g' % (key, ratio))


def cpu(t):
    return t.detach().cpu().numpy()


def ident(case):
    return '_'.join('%s%d' % kv for kv in zip('sfhblm' if len(case) == 6 else 'sfhbm', case))


def start(hip, S, F, H, B, L, M, seed):
    """(net at its own init x 1.7, those weights as store_packed() returns them, the float64 composite, rows away from relu kinks)"""
    net = hip.HipFastSlowNVP(F, S, H, B, L, seed=seed)
    net.load_packed((net.store_packed() * 1.7).astype(np.float32))
    w = net.store_packed()
    fs = ng.FastSlow(S, F, H, B, L)
    assert [(n, tuple(s)) for n, s in net.layer_shapes()] == [(n, tuple(s)) for n, s, _ in fs.layer_shapes()] and w.size == fs.n
    rng = np.random.RandomState(100 * S + F + M)
    X = rng.uniform(-1, 1, size=(M, S + F)).astype(np.float32)
    spare = rng.uniform(-1, 1, size=(vc.MAX_REPLACED, S + F)).astype(np.float32)

    def disagree(X, rows):
        return vc.kink(fs.loss_grad(w, X[rows], dtype=torch.float32)[1], fs.loss_grad(w, X[rows])[1])

    X, _ = vc.away_from_kinks(X, spare, disagree, ident((S, F, H, B, L, M)))
    return net, w, fs, X


@pytest.mark.parametrize('case', vc.FASTSLOW_CASES, ids=[ident(c) for c in vc.FASTSLOW_CASES])
def test_fast_slow_gradient_vs_float64(hip, case):
    S, F, H, B, L, M = case
    net, w, fs, X = start(hip, S, F, H, B, L, M, seed=11)
    used = net.used_mask()
    loss, grads = net.loss_grad(X)
    g = net.reference_gradient(grads)
    loss64, g64 = fs.loss_grad(w, X)
    _, g32 = fs.loss_grad(w, X, dtype=torch.float32)
    assert abs(float(loss) - loss64) < LOSS_RTOL * (1 + abs(loss64)), (float(loss), loss64)
    assert np.all(g64[~used] == 0) and np.all(g[~used] == 0)
    R = vc.rtol(g32, None, g64, None, fs.layer_shapes(), ~used)
    assert R <= vc.R_CAP, R
    note('gradient', vc.assert_vjp_close(g, None, g64, None, fs.layer_shapes(), R, ~used, ident(case))[0])
    # the padding of the interleaved coupling receives nothing: what _cmask nulls never reaches the optimiser
    gC = cpu(grads[2])
    assert not gC[net._coupling_mask() == 0].any()
    # log-probabilities and the three stages' log-determinants
    lp64, (lds64, ldf64, ldc64) = fs.log_probs(w, X, parts=True)
    lp = cpu(net.log_probs(X)).astype(np.float64)
    assert np.all(np.abs(lp - lp64) < LOSS_RTOL * (1 + np.abs(lp64)))
    z, ld = net.forward(X)
    z64 = cpu(z).astype(np.float64)
    assert np.all(np.abs(cpu(ld) - (lds64 + ldf64 + ldc64)) < LOSS_RTOL * (1 + np.abs(lds64 + ldf64 + ldc64)))
    x = torch.from_numpy(X).to(net.device)
    zs, lds = net.slow.forward(x[:, :S].contiguous())
    zf, ldf = net.fast.forward(x[:, S:].contiguous())
    _, ldc = net.coupling.forward(net._interleave(zs, zf))
    for got, want in ((lds, lds64), (ldf, ldf64), (ldc, ldc64)):
        assert np.all(np.abs(cpu(got) - want) < LOSS_RTOL * (1 + np.abs(want)))
    # log_probs = N(0, I) at z + the three log-determinants: the padding constant of the interleaved coupling is in it
    want = -0.5 * (z64 ** 2).sum(axis=1) - (S + F) * sg.LOG_2PI_HALF + cpu(lds) + cpu(ldf) + cpu(ldc)
    assert np.all(np.abs(lp - want) < LOSS_RTOL * (1 + np.abs(want)))
    note('log_probs', np.max(np.abs(lp - lp64) / (LOSS_RTOL * (1 + np.abs(lp64)))))


def test_fast_slow_refuses_more_than_sixteen_interleaved_pairs(hip):
    from nnest_amd import _lib
    with pytest.raises(_lib.NnestHipError):
        hip.HipFastSlowNVP(2, 17, 16, 3, 1)
    with pytest.raises(_lib.NnestHipError):
        hip.HipFastSlowNVP(17, 2, 16, 3, 1)


def adam_step(w, g, lr, wd, f32):
    if f32:
        return vc.adam_reference(w, np.zeros_like(w), np.zeros_like(w), 0, np.asarray(g, np.float32), lr, wd)[0].astype(np.float64)
    return sg.adam(w, [g], lr, wd)


@pytest.mark.parametrize('case', vc.FASTSLOW_STEP_CASES, ids=[ident(c) for c in vc.FASTSLOW_STEP_CASES])
def test_fast_slow_one_adam_step(hip, case):
    """one _train_epoch of a single minibatch against one float64 Adam step from the float64 gradient: per tensor on the used
    entries, relative to the tensor's largest update, within R_step = max(3e-5, 10 x what the float32 composite taking the same step
    on the CPU shows) -- the module header has the measured values"""
    S, F, H, B, L, M = case
    net, w, fs, X = start(hip, S, F, H, B, L, M, seed=12)
    used = net.used_mask()
    x = torch.from_numpy(X).to(net.device)
    tot = net._train_epoch(lambda epoch, lo, hi: x[lo:hi], 0, M, M, ntc.LR, ntc.WD)
    w1 = net.store_packed()
    assert np.array_equal(w1[~used], w[~used])
    loss64, g64 = fs.loss_grad(w, X)
    _, g32 = fs.loss_grad(w, X, dtype=torch.float32)
    assert abs(float(tot) - loss64) < LOSS_RTOL * (1 + abs(loss64))
    w64 = w.astype(np.float64)
    d64, d32, d = adam_step(w64, g64, ntc.LR, ntc.WD, False) - w64, adam_step(w, g32, ntc.LR, ntc.WD, True) - w64, w1.astype(np.float64) - w64
    shapes = fs.layer_shapes()
    worst32 = vc.worst_ratios(d32, None, d64, None, shapes, ~used)[0]
    R_step = max(ntc.BOUNDS['rtol_min'], ntc.BOUNDS['rtol_factor'] * worst32)
    i = int(np.argmax(np.where(used, np.abs(d32 - d64), 0.0)))
    print('%s: float32 composite step off by %.3g of a tensor\'s largest update: R_step %.3g (most at %s: g64 %.3g, g32 - g64 %.3g, w %.3g)' % (
        ident(case), worst32, R_step, [n for n, s, o in shapes if o <= i < o + int(np.prod(s))][0], g64[i], g32[i] - g64[i], w[i]))
    assert R_step <= 1e-2, R_step      # (1 % of an update: a wrong sign is 200 %, step 2's bias correction 47 %, a missing weight decay 100 % where g ~ 0)
    d64m = np.where(used, d64, 0.0)
    note('adam step', vc.assert_vjp_close(np.where(used, d, 0.0), None, d64m, None, shapes, R_step, ~used, ident(case) + ' step')[0])
    for stage in (net.fast, net.slow, net.coupling):
        assert stage.adam_step_count() == 1


@pytest.mark.parametrize('case', vc.FASTSLOW_SPLINE_CASES, ids=[ident(c) for c in vc.FASTSLOW_SPLINE_CASES])
def test_fast_slow_spline_gradient_vs_float64(hip, case):
    """FastSlowSpline: the spline stages per tensor at the spline tests' tolerance (spline_grad_check.GPU_RTOL_T, GPU_FLOOR), rows kept
    away from knots as there; the hidden-64 coupling with the checker above"""
    S, F, H, B, M = case
    net = hip.HipFastSlowSpline(F, S, H, B, seed=21)
    rng = np.random.RandomState(10 * S + F)
    pool = rng.uniform(-1, 1, size=(2 * M + 64, S + F)).astype(np.float32)
    net.forward(pool[:max(M, 32)])                       # the ActNorm data-dependent initialisation of both stages
    assert net.data_dep_init_done
    w, P = net.store_packed(), net.P
    fs = ng.FastSlow(S, F, H, B, 1, kind='spline', P=P, K=net.slow.K, tail=net.slow.tail_bound)
    assert [(n, tuple(s)) for n, s in net.layer_shapes()] == [(n, tuple(s)) for n, s, _ in fs.layer_shapes()] and w.size == fs.n
    wf, ws = w[:fs.n_fast], w[fs.n_fast:fs.n_fast + fs.n_slow]
    ok = (sg.log_probs(ws, P['slow'], pool[:, :S], S, H, B, fs.K, fs.tail, margins=True)[2] > KNOT_MARGIN) & \
        (sg.log_probs(wf, P['fast'], pool[:, S:], F, 16, B, fs.K, fs.tail, margins=True)[2] > KNOT_MARGIN)
    rows = pool[ok]
    assert rows.shape[0] >= M + vc.MAX_REPLACED, int(ok.sum())
    lo = fs.n_fast + fs.n_slow

    def disagree(X, r):      # relu kinks of the coupling's translate net
        return vc.kink(fs.loss_grad(w, X[r], dtype=torch.float32)[1][lo:], fs.loss_grad(w, X[r])[1][lo:])

    X, _ = vc.away_from_kinks(rows[:M], rows[M:M + vc.MAX_REPLACED], disagree, ident(case))
    used = net.used_mask()
    net.data_dep_init_done = True
    loss, grads = net.loss_grad(X)
    g = net.reference_gradient(grads)
    loss64, g64 = fs.loss_grad(w, X)
    _, g32 = fs.loss_grad(w, X, dtype=torch.float32)
    assert abs(float(loss) - loss64) < LOSS_RTOL * (1 + abs(loss64)), (float(loss), loss64)
    assert np.all(g64[~used] == 0) and np.all(g[~used] == 0)
    stages, coupling = vc.assert_fastslow_spline_close(g, g64, g32, fs, ~used, ident(case))
    note('spline stages', stages)
    note('spline coupling', coupling)
