"""nnest_nvp_vjp (train_kernel in its vector-Jacobian mode) and nnest_nvp_adam_step held to float64 on their own, not through the
fast/slow hierarchy that is their only caller in the package.

The contract (include/nnest_hip.h): L = <gz, z(X)> + gld * sum_rows logdet(X)  ->  dL/dw in packed order, dL/dx [M, D].  Every one of
train_kernel's 28 (NT, NH, L) instantiations and its three LDS layouts is run once (tests/nvp_vjp_check.py VJP_TABLE), with gz ~ N(0, 1)
and gld = 0.37, against oracle/nvp_grad.py in float64: dw tensor by tensor, dx row by row, parameters that are zero by construction
exactly zero, every element of dx written and nothing behind it.  The bound R comes from the float32 restatement on the same input
(tests/nvp_vjp_check.py has the rule; tests/test_nvp_vjp_check.py runs the same table through the checker on the CPU).  Run with
pytest -m gpu -s  to see the error / bound ratios."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import nvp_grad as ng  # noqa: E402  (checker only)
from tests import nvp_train_check as ntc  # noqa: E402
from tests import nvp_vjp_check as vc  # noqa: E402

IDS = [vc.row_id(c) for c in vc.VJP_TABLE]
WORST = {}
SENTINEL = -777.25
TAIL = 64


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import flow
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    yield flow
    print('\nnvp_vjp worst error / bound: ' + '  '.join('%s %.3g' % kv for kv in sorted(WORST.items())))


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def cpu(t):
    return t.detach().cpu().numpy()


def fresh(hip, c, w):
    nvp = hip.HipNVP(c.D, c.H, c.B, c.L, scale=c.scale, seed=0)
    nvp.load_packed(w)
    if c.beta:
        from nnest_amd.distributions import GeneralisedNormal
        nvp.set_base(GeneralisedNormal(torch.zeros(c.D), torch.ones(c.D), torch.tensor(c.beta)))
    assert [(n, tuple(s), o) for n, s, o in nvp.layer_shapes()] == [(n, tuple(s), o) for n, s, o in vc.layer_shapes(c)]
    return nvp


def kernel_vjp(nvp, X, gz, gld):
    """HipNVP.vjp with dx written into the head of a buffer of M D + TAIL sentinels -> (dw, dx [M, D], the tail) as numpy arrays"""
    M, D = X.shape
    dev = nvp.device
    x, g = torch.from_numpy(X).to(dev), torch.from_numpy(np.ascontiguousarray(gz, np.float32)).to(dev)
    buf = torch.full((M * D + TAIL,), SENTINEL, dtype=torch.float32, device=dev)
    grad = torch.full((nvp._native_params,), SENTINEL, dtype=torch.float32, device=dev)
    from nnest_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(nvp._sym['vjp'](nvp._h, _lib.ptr(x), _lib.ptr(g), ctypes.c_float(gld), M, _lib.ptr(grad), _lib.ptr(buf),
                                   _lib.current_stream(dev)))
    out = cpu(buf)
    native = cpu(grad)
    assert not np.any(native == SENTINEL), 'dw: native entries never written: %s' % np.flatnonzero(native == SENTINEL)[:8]
    if nvp._pidx is not None:            # what the zero padding of a hidden width that is no tile width receives: nothing
        pad = np.ones(native.size, bool)
        pad[nvp._pidx] = False
        assert not native[pad].any(), 'dw: a padded entry has a gradient'
    return cpu(nvp._from_native_dev(grad)), out[:M * D].reshape(M, D), out[M * D:]


def reference(c, w, X, gz, gld):
    """(float32 restatement (dw, dx), float64 (dw, dx), R) for this input"""
    a, b = vc.oracle_vjp(c, w, X, gz, gld, f32=True), vc.oracle_vjp(c, w, X, gz, gld)
    return a, b, vc.rtol(a[0], a[1], b[0], b[1], vc.layer_shapes(c), vc.vjp_masked(c))


@pytest.mark.parametrize('c', vc.VJP_TABLE, ids=IDS)
def test_vjp_every_instantiation(hip, c):
    w, X, gz, _ = vc.screened_vjp_inputs(c)
    nvp = fresh(hip, c, w)
    assert nvp.train_form_for(1, one_cu=True) == ('single', c.imglds), vc.row_id(c)      # (IMGLDS does not depend on the rows)
    gw, gx, tail = kernel_vjp(nvp, X, gz, vc.GLD)
    written = gx != SENTINEL
    assert written.all(), 'dx: %d of %d elements never written, the first at %s' % ((~written).sum(), gx.size, np.argwhere(~written)[0])
    assert np.all(tail == SENTINEL), 'dx: written behind row M - 1 at offset %d' % int(np.flatnonzero(tail != SENTINEL)[0])
    _, (gw64, gx64), R = reference(c, w, X, gz, vc.GLD)
    assert R <= vc.R_CAP
    dw, dx = vc.assert_vjp_close(gw, gx, gw64, gx64, vc.layer_shapes(c), R, vc.vjp_masked(c), vc.row_id(c))
    print('%s %s IMGLDS %d: worst error / bound dw %.3g dx %.3g (R %.3g)' % ((vc.row_id(c), vc.instantiation(c), c.imglds, dw, dx, R)))
    note('dw', dw)
    note('dx', dx)
    # the public wrapper returns the same
    gw2, gx2 = nvp.vjp(torch.from_numpy(X).to(nvp.device), torch.from_numpy(gz).to(nvp.device), vc.GLD)
    assert np.array_equal(cpu(gw2), gw) and np.array_equal(cpu(gx2), gx)


@pytest.mark.parametrize('c', vc.LINEAR_ROWS, ids=[vc.row_id(c) for c in vc.LINEAR_ROWS])
def test_vjp_is_linear_in_its_cotangent(hip, c):
    """vjp(gz, 0) + vjp(0, gld) = vjp(gz, gld) within the checker's bound of the latter, and vjp(0, 0) is exactly zero: a gld that
    leaks into the gz path (or the reverse) shows in the parts"""
    w, X, gz, _ = vc.screened_vjp_inputs(c)
    nvp = fresh(hip, c, w)
    zero = np.zeros_like(gz)
    both, only_gz, only_gld, none = (kernel_vjp(nvp, X, g, l)[:2] for g, l in ((gz, vc.GLD), (gz, 0.0), (zero, vc.GLD), (zero, 0.0)))
    assert not none[0].any() and not none[1].any()
    shapes, masked = vc.layer_shapes(c), vc.vjp_masked(c)
    worst = [0.0, 0.0]
    for g, l, got in ((gz, 0.0, only_gz), (zero, vc.GLD, only_gld)):          # each part against float64 on its own ...
        _, (gw64, gx64), R = reference(c, w, X, g, l)
        worst = np.maximum(worst, vc.assert_vjp_close(got[0], got[1], gw64, gx64, shapes, R, masked, '%s gld %g' % (vc.row_id(c), l)))
    _, (gw64, gx64), R = reference(c, w, X, gz, vc.GLD)                       # ... and their sum as the whole
    worst = np.maximum(worst, vc.assert_vjp_close(only_gz[0].astype(np.float64) + only_gld[0], only_gz[1].astype(np.float64) + only_gld[1],
                                                  gw64, gx64, shapes, R, masked, vc.row_id(c) + ' sum of the parts'))
    vc.assert_vjp_close(both[0], both[1], gw64, gx64, shapes, R, masked, vc.row_id(c))
    note('linear dw', worst[0])
    note('linear dx', worst[1])


@pytest.mark.parametrize('c', vc.LOSS_GRAD_ROWS, ids=[vc.row_id(c) for c in vc.LOSS_GRAD_ROWS])
def test_vjp_reproduces_loss_grad(hip, c):
    """gz = dE/dz / M from the GPU's own forward, gld = -1 / M: dw is loss_grad's gradient within 2 R (the two entries share the
    kernel: this is the mode switch alone -- and, at hidden 64 with two hidden layers and 128 rows, the split over two launches)"""
    w, X, _, _ = vc.screened_vjp_inputs(c)
    nvp = fresh(hip, c, w)
    z, _ = nvp.forward(X)
    gz = ng.base_denergy(cpu(z).astype(np.float64), c.beta) / c.M
    loss, g = nvp.loss_grad(X)
    gw, _, _ = kernel_vjp(nvp, X, gz.astype(np.float32), -1.0 / c.M)
    shapes, masked = vc.layer_shapes(c), vc.vjp_masked(c)
    l64, g64 = ng.loss_grad(w, X, c.D, c.H, c.B, c.L, c.scale, c.beta)
    g32 = ng.loss_grad(w, X, c.D, c.H, c.B, c.L, c.scale, c.beta, dtype=torch.float32)[1]
    R = vc.rtol(g32, None, g64, None, shapes, masked)
    assert R <= vc.R_CAP
    assert abs(float(loss) - l64) < ntc.BOUNDS['loss'] * (1 + abs(l64))
    note('loss_grad dw', vc.assert_vjp_close(cpu(g), None, g64, None, shapes, R, masked, vc.row_id(c) + ' loss_grad')[0])
    note('vjp as loss_grad', vc.assert_vjp_close(gw, None, cpu(g).astype(np.float64), None, shapes, 2 * R, masked, vc.row_id(c))[0])


def native_state(nvp):
    """(w, exp_avg, exp_avg_sq) as the handle holds them, padding included, and the step count"""
    from nnest_amd import _lib
    w, m, v = nvp._native_buffer(), nvp._native_buffer(), nvp._native_buffer()
    st = _lib.current_stream(nvp.device)
    with torch.cuda.device(nvp.device):
        _lib.check(nvp._lib.nnest_nvp_store_weights(nvp._h, w.ctypes.data_as(ctypes.c_void_p), st))
        _lib.check(nvp._lib.nnest_nvp_store_adam(nvp._h, m.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p), st))
    return w, m, v, nvp.adam_step_count()


@pytest.mark.parametrize('D,H,B,L', vc.ADAM_SHAPES, ids=['d%d_h%d_b%d_l%d' % s for s in vc.ADAM_SHAPES])
def test_adam_step_from_a_known_gradient(hip, D, H, B, L):
    """nnest_nvp_adam_step (adam_packed_dev_kernel, the step count on the device): three steps from gradients drawn here, each held
    to the float64 step from the state before it; the entries that pad a hidden width to a tile width stay zero"""
    c = vc.row(D, H, B, L, 1, None)
    nvp = fresh(hip, c, ntc.start_weights(c))
    rng = np.random.RandomState(D + H)
    pad = None
    if nvp._pidx is not None:
        pad = np.ones(nvp._native_params, bool)
        pad[nvp._pidx] = False
    assert (pad is not None) == (H == 10)
    pre = native_state(nvp)
    assert pre[3] == 0 and not pre[1].any() and not pre[2].any()
    for k in range(3):
        # gradients over six decades, as the tensors of a flow have them
        g = (rng.randn(nvp.num_params) * 10.0 ** rng.uniform(-6, 0, nvp.num_params)).astype(np.float32)
        nvp.adam_step(torch.from_numpy(g).to(nvp.device), ntc.LR, ntc.WD)
        post = native_state(nvp)
        r = vc.check_adam_step(pre, post, nvp._to_native(g), ntc.LR, ntc.WD, 'd%d h%d step %d' % (D, H, k + 1))
        for key, ratio in zip(('adam exp_avg', 'adam exp_avg_sq', 'adam weight'), r):
            note(key, ratio)
        if pad is not None:
            assert not post[0][pad].any() and not post[1][pad].any() and not post[2][pad].any(), 'a padded entry moved'
        assert np.array_equal(nvp.store_packed(), nvp._from_native(post[0]))
        pre = post
    # the passes run on the stepped weights (the fragment images were rebuilt)
    X = rng.uniform(-1, 1, size=(5, D)).astype(np.float32)
    z64, ld64 = ng.passes(nvp.store_packed(), X, D, H, B, L)
    z, ld = nvp.forward(X)
    assert np.max(np.abs(cpu(z) - z64)) < 3e-5 * (1 + np.max(np.abs(z64))) and np.max(np.abs(cpu(ld) - ld64)) < 3e-5 * (1 + np.max(np.abs(ld64)))


@pytest.mark.parametrize('D,H,B,L,batch,cap', [(8, 64, 2, 2, 100, 96), (40, 32, 2, 3, 128, 112)], ids=['h64_l2_batch100', 'h32_l3_d40_batch128'])
def test_minibatches_one_workgroup_cannot_stage_train_through_the_host_loop(hip, D, H, B, L, batch, cap):
    """where 128 rows of staging do not fit a compute unit (rows_per_launch < 128) loss_grad and vjp split the batch over launches,
    and train_epochs, whose one-launch loop cannot, drives such minibatches from the host: the same weights, bit for bit, as
    loss_grad + adam_step per minibatch here"""
    from nnest_amd import _lib
    c = vc.row(D, H, B, L, batch, 0)
    assert vc.rows_per_launch(c) == cap < batch and vc.expected_imglds(c) == 0
    w0 = ntc.start_weights(c)
    nvp, chain = fresh(hip, c, w0), fresh(hip, c, w0)
    assert nvp.train_form_for(cap) == ('single', 0)
    with pytest.raises(_lib.NnestHipError):
        nvp.train_form_for(cap + 1)
    rng = np.random.RandomState(D)
    n_train = batch + 50
    X, xv = rng.uniform(-1, 1, size=(n_train, D)).astype(np.float32), rng.uniform(-1, 1, size=(16, D)).astype(np.float32)
    perm = rng.permutation(n_train)
    res = nvp.train_epochs(X, xv, torch.from_numpy(perm[None].astype(np.int64)), batch=batch, max_epochs=1, lr=ntc.LR, weight_decay=ntc.WD)
    assert res['epochs_run'] == 1 and res['best_epoch'] == 1 and np.isfinite(res['best_validation_loss'])
    total = 0.0
    for lo in range(0, n_train, batch):
        rows = X[perm[lo:lo + batch]]
        loss, g = chain.loss_grad(rows)
        l64 = ng.loss_grad(chain.store_packed(), rows, D, H, B, L)[0]
        assert abs(float(loss) - l64) < ntc.BOUNDS['loss'] * (1 + abs(l64))
        chain.adam_step(g, ntc.LR, ntc.WD)
        total += float(loss)
    assert np.array_equal(nvp.store_packed(), chain.store_packed()) and nvp.adam_step_count() == chain.adam_step_count() == 2
    assert abs(float(res['losses'][0, 0]) * n_train - total) < 1e-5 * abs(total)


@pytest.mark.parametrize('D,H,L,batch', [(8, 64, 2, 100), (40, 32, 3, 128)], ids=['h64_l2_batch100', 'h32_l3_d40_batch128'])
def test_trainer_runs_such_a_shape_past_one_chunk_of_epochs(hip, D, H, L, batch):
    """Trainer.train cuts a run into launches of 128 epochs, which the host-driven loop does not take: at the default batch_size 100
    (hidden 64, two hidden layers: 96 rows per launch) and at 128 (hidden 32, three, x_dim 40: 112) such a flow must train 140 epochs
    in one call (epoch_loop_on_host), every epoch logged, the loss going down"""
    from nnest_amd import trainer
    assert 140 > trainer.EPOCH_CHUNK
    t = trainer.Trainer(D, hidden_dim=H, num_blocks=2, num_layers=L, batch_size=batch, flow='nvp', log_dir=None, log_level=30, learning_rate=1e-3)
    rng = np.random.RandomState(D)
    live = rng.uniform(-1, 1, size=(150, D)) * np.linspace(0.2, 1.0, D)        # 135 training rows: two minibatches
    assert vc.rows_per_launch(vc.row(D, H, 2, L, batch, 0)) < batch
    assert t.netG.epoch_loop_on_host(batch, 135) and not t.netG.epoch_loop_on_host(batch, 64) and getattr(t.netG, 'epoch_chunk', 128) == 128
    t.train(live, max_iters=140, jitter=0.01, patience=1000, rng_seed=3)
    assert t.losses.shape == (140, 2) and np.all(np.isfinite(t.losses)) and t.total_iters == 140
    assert t.netG.adam_step_count() == 280 and t.losses[-1, 1] < t.losses[0, 1]
    assert 1 <= t.best_validation_epoch <= 140 and t.best_validation_loss == pytest.approx(float(t.losses[:, 1].min()), rel=1e-6)
    with pytest.raises(ValueError, match='one call'):       # a continued chunk is refused by name, before anything runs
        t.netG.train_epochs(live[:135], live[135:], torch.zeros(1, 135, dtype=torch.int64), batch=batch, max_epochs=1, epoch_offset=128, resume=True)
