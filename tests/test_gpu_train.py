"""GPU parity tests of the training kernel (K5, nnest_nvp_train / nnest_nvp_loss_grad) against the golden
fixtures recorded from the reference's Trainer._train / Trainer.train (oracle/gen_golden.py G4, G7) and
against the oracle.  Tolerances are those the oracle itself meets against the same fixtures
(tests/test_oracle_golden.py), stated inline."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import oracle as orc  # noqa: E402  (checker only)

G = os.path.join(os.path.dirname(__file__), 'golden')
TRAIN_FILES = sorted(glob.glob(os.path.join(G, 'train_*.npz')))
RUN_FILES = sorted(glob.glob(os.path.join(G, 'trainrun_*.npz')))


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import flow
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return flow


@pytest.mark.parametrize('path', TRAIN_FILES, ids=[os.path.basename(p)[6:-4] for p in TRAIN_FILES])
def test_loss_and_gradient_vs_golden(hip, path):
    """loss.backward() of the reference (trainer.py:394-400): every gradient element."""
    g = np.load(path)
    D, H, B, L = int(g['D']), int(g['H']), int(g['B']), int(g['L'])
    nvp = hip.HipNVP(D, H, B, L)
    X, batch, jitter = g['X'], int(g['batch']), float(g['jitter'])
    n = X.shape[0]
    k = 0
    for e in range(g['perms'].shape[0]):
        for b in range(0, n, batch):
            nvp.load_packed(g['w0'] if k == 0 else g['ws'][k - 1])
            idx = g['perms'][e][b:b + batch]
            data = X[idx] + np.float32(jitter) * g['noises'][e][b:b + batch]
            loss, grad = nvp.loss_grad(data)
            gref = g['grads'][k]
            assert abs(float(loss) - g['losses'][k]) < 2e-5 * (1 + abs(g['losses'][k]))
            err = np.max(np.abs(grad.cpu().numpy() - gref))
            assert err < 3e-5 * (1e-3 + np.max(np.abs(gref))), (k, err)
            # exact zeros of the reference (masked-out weights) are exact zeros here too
            assert np.all(grad.cpu().numpy()[gref == 0] == 0)
            k += 1


@pytest.mark.parametrize('path', TRAIN_FILES, ids=[os.path.basename(p)[6:-4] for p in TRAIN_FILES])
def test_train_epochs_vs_golden_steps(hip, path):
    """Two epochs of Trainer._train with the reference's recorded shuffle and jitter noise: losses, Adam
    moments and weights after the last step."""
    g = np.load(path)
    D, H, B, L = int(g['D']), int(g['H']), int(g['B']), int(g['L'])
    nvp = hip.HipNVP(D, H, B, L)
    nvp.load_packed(g['w0'])
    X = g['X']
    n = X.shape[0]
    E = g['perms'].shape[0]
    res = nvp.train_epochs(X, X, torch.from_numpy(g['perms']), torch.from_numpy(g['noises']), jitter=float(g['jitter']),
                           batch=int(g['batch']), max_epochs=E, patience=50, lr=float(g['lr']),
                           weight_decay=float(g['weight_decay']))
    assert res['epochs_run'] == E
    losses = res['losses'].cpu().numpy()
    # reference's epoch train loss = sum(batch means)/len(dataset)  (trainer.py:403)
    np.testing.assert_allclose(losses[:, 0], g['ref_epoch_losses'], rtol=3e-5, atol=1e-6)
    steps_per_epoch = (n + int(g['batch']) - 1) // int(g['batch'])
    assert nvp.adam_step_count() == E * steps_per_epoch
    m, v = nvp.adam_moments()
    assert np.max(np.abs(m - g['ms'][-1])) < 5e-5 * (1e-3 + np.max(np.abs(g['ms'][-1])))
    assert np.max(np.abs(v - g['vs'][-1])) < 2e-4 * (1e-6 + np.max(np.abs(g['vs'][-1])))
    # validation on X itself after the last epoch (trainer.py:405-418)
    assert abs(losses[-1, 1] - float(g['valid_loss'])) < 3e-5 * (1 + abs(float(g['valid_loss'])))
    # weights: best-validation restore picks an epoch; compare with the reference weights of that epoch
    w = nvp.store_packed()
    wref = g['ws'][res['best_epoch'] * steps_per_epoch - 1]
    moved = np.sqrt(np.mean((wref - g['w0']) ** 2))
    assert np.sqrt(np.mean((w - wref) ** 2)) < 0.1 * moved
    gnoise = np.abs(g['grads'][-1]) > 1e-3 * np.max(np.abs(g['grads'][-1]))
    assert np.max(np.abs(w - wref)[gnoise]) < 1e-3  # lr = 1e-3: well-conditioned elements track closely


def test_product_kernel_adam_steps_one_by_one_vs_golden(hip):
    """The PRODUCT training kernel (train_kernel_rows: what Trainer.train launches at the reference's default shape) held to the
    reference's recorded Adam trajectory STEP BY STEP (round-4 verdict: only single-step gradients and two-epoch end states were
    tight, and loss_grad runs the single-workgroup kernel).  train_d50.npz holds the weights after each of the six optimizer steps of
    two epochs (trainer.py:384-403); here every step is one launch of the epoch loop over exactly that minibatch's rows (the
    reference's shuffle order and jitter noise), the Adam state carried in the handle.  After every step: the weights of every
    element whose gradient is not at rounding level within 2e-5 of the largest weight, Adam's moments to the fixtures."""
    g = np.load(os.path.join(G, "train_d50.npz"))
    D, H, B, L = int(g['D']), int(g['H']), int(g['B']), int(g['L'])
    nvp = hip.HipNVP(D, H, B, L)
    nvp.load_packed(g['w0'])
    X, batch = g['X'], int(g['batch'])
    n = X.shape[0]
    k = 0
    solid = np.ones(nvp.num_params, bool)   # elements whose gradient stood clear of rounding in every step so far
    for e in range(g['perms'].shape[0]):
        for mb in range((n + batch - 1) // batch):
            rows = g['perms'][e][mb * batch:(mb + 1) * batch]
            M = rows.shape[0]
            noise = torch.from_numpy(np.ascontiguousarray(g['noises'][e][mb * batch:mb * batch + M][None]))
            perm = torch.arange(M, dtype=torch.int32)[None]
            res = nvp.train_epochs(X[rows], X[:16], perm, noise, jitter=float(g['jitter']), batch=batch, max_epochs=1, patience=50,
                                   lr=float(g['lr']), weight_decay=float(g['weight_decay']), finalize=False, resume=k > 0,
                                   epoch_offset=k, result=res['result'] if k > 0 else None)
            assert res['epochs_run'] == k + 1 and nvp.adam_step_count() == k + 1
            # the epoch's training loss as the reference logs it is this step's batch loss / rows (trainer.py:403)
            assert abs(float(res['losses'].cpu().numpy()[0, 0]) * M - float(g['losses'][k])) < 3e-5 * (1 + abs(float(g['losses'][k])))
            w = nvp.store_packed()
            gk = np.abs(g['grads'][k])
            solid &= gk > 1e-3 * gk.max()
            wmax = np.max(np.abs(g['ws'][k]))
            assert np.max(np.abs(w - g['ws'][k])[solid]) <= 2e-5 * wmax, (k, np.max(np.abs(w - g['ws'][k])[solid]) / wmax)
            # (an element whose gradient is at rounding level can take Adam's first steps with the other sign: +- lr; bounded, rare)
            assert np.max(np.abs(w - g['ws'][k])) <= 2.5 * float(g['lr']) * (k + 1)
            assert np.mean(np.abs(w - g['ws'][k]) > 2e-5 * wmax) < 0.02
            m, v = nvp.adam_moments()
            assert np.max(np.abs(m - g['ms'][k])) < 5e-5 * (1e-3 + np.max(np.abs(g['ms'][k])))
            assert np.max(np.abs(v - g['vs'][k])) < 2e-4 * (1e-6 + np.max(np.abs(g['vs'][k])))
            k += 1
    assert k == g['ws'].shape[0]


@pytest.mark.parametrize('path', RUN_FILES, ids=[os.path.basename(p)[9:-4] for p in RUN_FILES])
def test_train_run_vs_golden(hip, path):
    """Trainer.train (split, epochs, early stopping, best restore) with the recorded split/shuffles/noise."""
    g = np.load(path)
    D = int(g['D'])
    nvp = hip.HipNVP(D, int(g['H']), int(g['B']), int(g['L']))
    nvp.load_packed(g['w0'])
    live, ps = g['live'], g['perm_split']
    N = live.shape[0]
    n_valid = int(np.ceil(0.1 * N))
    Xv = live[ps[:n_valid]]
    Xt = live[ps[n_valid:]]
    E = int(g['max_iters'])
    res = nvp.train_epochs(Xt, Xv, torch.from_numpy(g['perms']), torch.from_numpy(g['noises']), jitter=float(g['jitter']),
                           batch=int(g['batch']), max_epochs=E, patience=int(g['patience']), lr=float(g['lr']),
                           weight_decay=float(g['weight_decay']))
    assert res['epochs_run'] == int(g['epochs_run'])
    assert res['best_epoch'] == int(g['best_validation_epoch'])
    losses = res['losses'].cpu().numpy()[:res['epochs_run']]
    tol = 2e-4 if res['epochs_run'] <= 10 else 2e-3  # logged with 4 decimals; Adam amplifies rounding over many steps
    np.testing.assert_allclose(losses[:, 0], g['train_losses_logged'], atol=tol)
    np.testing.assert_allclose(losses[:, 1], g['valid_losses_logged'], atol=tol)
    assert abs(res['best_validation_loss'] - float(g['best_validation_loss'])) < tol
    w = nvp.store_packed()
    moved = np.sqrt(np.mean((g['w_final'] - g['w0']) ** 2))
    assert np.sqrt(np.mean((w - g['w_final']) ** 2)) < 0.25 * moved
    # the forward image used by the inference kernels was rebuilt from the restored weights
    o = orc.NVP(D, int(g['H']), int(g['B']), int(g['L']), w)
    x = live[:32].astype(np.float32)
    z, ld = nvp.forward(x)
    zo, ldo = o.forward(x)
    assert np.max(np.abs(z.cpu().numpy() - zo)) < 2e-5


def test_training_is_bitwise_reproducible_and_inkernel_noise_trains(hip):
    """Same inputs + seed -> identical weights (no atomics in the gradient path); in-kernel jitter noise
    lowers the validation loss on a simple target."""
    rng = np.random.RandomState(0)
    D = 50
    X = (rng.normal(size=(1000, D)) * 0.2).astype(np.float32)
    Xt, Xv = X[:900], X[900:]
    E = 12
    perm = torch.stack([torch.randperm(900) for _ in range(E)]).int()
    outs = []
    for _ in range(2):
        nvp = hip.HipNVP(D, 16, 3, 1, seed=3)
        res = nvp.train_epochs(Xt, Xv, perm, None, seed=11, jitter=0.01, batch=100, max_epochs=E, patience=50)
        outs.append((nvp.store_packed(), res))
    assert np.array_equal(outs[0][0], outs[1][0])
    losses = outs[0][1]['losses'].cpu().numpy()
    assert outs[0][1]['epochs_run'] == E
    assert losses[-1, 1] < losses[0, 1] - 1e-3
    assert np.all(np.isfinite(losses))


def test_patience_stops_early(hip):
    rng = np.random.RandomState(1)
    D = 6
    X = rng.uniform(-1, 1, size=(40, D)).astype(np.float32)
    Xv = rng.uniform(-1, 1, size=(6, D)).astype(np.float32) * 3.0  # validation set off-distribution: it gets worse
    E = 400
    perm = torch.stack([torch.randperm(40) for _ in range(E)]).int()
    nvp = hip.HipNVP(D, 16, 3, 1, seed=5)
    res = nvp.train_epochs(X, Xv, perm, None, seed=1, jitter=0.0, batch=100, max_epochs=E, patience=5, lr=1e-2)
    assert res['epochs_run'] < E
    # counter is reset to 0 on improvement, incremented every epoch, stop when counter > patience
    # (trainer.py:205-209, :223-225): the run ends `patience` epochs after the best one
    assert res['epochs_run'] == res['best_epoch'] + 5
    losses = res['losses'].cpu().numpy()[:res['epochs_run']]
    assert abs(losses[res['best_epoch'] - 1, 1] - res['best_validation_loss']) < 1e-7
    assert np.all(losses[res['best_epoch']:, 1] >= res['best_validation_loss'])


def test_training_jitter_vs_oracle(hip):
    from nnest_amd import _lib
    rng = np.random.RandomState(2)
    X = rng.uniform(-1, 1, size=(500, 20))
    xd = torch.from_numpy(X).cuda()
    out = torch.zeros(1, dtype=torch.float64, device='cuda')
    _lib.check(_lib.load().nnest_training_jitter(_lib.ptr(xd), 500, 20, _lib.ptr(out), _lib.current_stream(xd.device)))
    assert abs(float(out) - orc.training_jitter(X)) < 1e-12


def test_l2_norm_and_explicit_standard_normal_base(hip, tmp_path):
    """Trainer.train(l2_norm=...) (trainer.py:395-399) adds 2 * l2_norm * w to every gradient, which is Adam's coupled
    weight decay with weight_decay + 2 * l2_norm; base_dist = MultivariateNormal(0, I) is the default base."""
    from nnest_amd.trainer import Trainer
    rng = np.random.RandomState(0)
    D, N, E = 5, 230, 3
    live = rng.uniform(-1, 1, size=(N, D))
    split = rng.permutation(N)
    perms = np.stack([rng.permutation(N - 23) for _ in range(E)]).astype(np.int32)
    noises = rng.normal(size=(E, N - 23, D)).astype(np.float32)
    outs = []
    for l2, wd in ((0.01, 1e-6), (0.0, 1e-6 + 0.02)):
        base = torch.distributions.MultivariateNormal(torch.zeros(D), torch.eye(D))
        t = Trainer(D, log_dir=None, learning_rate=1e-3, weight_decay=wd, seed=1, log_level=30, base_dist=base, flow='nvp')
        t.train(live, max_iters=E, jitter=0.01, split=split, perms=perms, noises=noises, l2_norm=l2)
        outs.append(t.netG.store_packed())
    assert np.max(np.abs(outs[0] - outs[1])) < 1e-7
    w0 = Trainer(D, log_dir=None, seed=1, log_level=30, flow='nvp').netG.store_packed()
    o = orc.NVP(D, 16, 3, 1, w0)
    o.train(live, split, perms, noises, 0.01, E, wd=1e-6 + 0.02)
    d_ref, d_our = o.w - w0, outs[0] - w0
    assert np.sqrt(np.mean((d_our - d_ref) ** 2)) < 0.03 * np.sqrt(np.mean(d_ref ** 2))
    with pytest.raises(NotImplementedError):
        Trainer(D, log_dir=None, base_dist=torch.distributions.MultivariateNormal(torch.ones(D), torch.eye(D)))


@pytest.mark.parametrize('D,L,N,batch', [(50, 1, 1000, 100), (7, 2, 230, 64), (100, 1, 500, 128), (2, 0, 100, 100), (20, 1, 333, 100)])
def test_grid_training_vs_single_workgroup(hip, D, L, N, batch):
    """K5 on eight compute units (train_kernel_grid: one workgroup per 16-row tile, global staging, two grid barriers per
    minibatch) against the single-workgroup kernel (NNEST_TRAIN_ONE_CU): weights, Adam moments, per-epoch losses and the
    early-stopping state, with in-kernel jitter noise, a ragged last minibatch and a chunk boundary in the middle.  The
    contractions run in the same order in both; what differs is where hipcc fuses a multiply-add, i.e. the last bit of a few
    elementwise results, which 12 epochs of Adam steps carry along -- so: equal to 1e-4 of the largest element, and the grid
    kernel equal to ITSELF bit for bit (the property replica training relies on)."""
    rng = np.random.RandomState(D + L)
    live = rng.normal(size=(N, D)) * 0.3
    nv = N // 10
    E = 12
    perms = torch.stack([torch.randperm(N - nv, generator=torch.Generator().manual_seed(e)) for e in range(E)]).int()
    out = {}
    for key, one_cu in (('one', True), ('grid', False), ('grid2', False)):
        nvp = hip.HipNVP(D, 16, 3, L, seed=5)
        kw = dict(seed=77, jitter=0.02, batch=batch, patience=4, lr=1e-3, weight_decay=1e-6, one_cu=one_cu)
        r1 = nvp.train_epochs(live[nv:], live[:nv], perms[:5], None, max_epochs=5, finalize=False, **kw)
        r2 = nvp.train_epochs(live[nv:], live[:nv], perms[5:], None, max_epochs=E - 5, epoch_offset=5, resume=True,
                              result=r1['result'], finalize=True, **kw)
        m, v = nvp.adam_moments()
        out[key] = (nvp.store_packed(), m, v, r1['losses'].cpu().numpy(), r2['losses'].cpu().numpy(), r2['epochs_run'],
                    r2['best_epoch'], r2['stopped'], nvp.adam_step_count(), r2['best_validation_loss'])
    a, b, c = out['one'], out['grid'], out['grid2']
    for x, y in zip(b[:5], c[:5]):
        assert np.array_equal(x, y)                 # deterministic down to the last bit
    assert b[5:] == c[5:]
    for x, y in zip(a[:5], b[:5]):
        assert np.max(np.abs(x - y)) <= 1e-4 * (1e-3 + np.max(np.abs(x)))
    assert a[5:9] == b[5:9] and abs(a[9] - b[9]) <= 1e-5 * abs(a[9])
    assert a[5] >= 6 and a[8] > 0 and np.all(np.isfinite(a[3]))
