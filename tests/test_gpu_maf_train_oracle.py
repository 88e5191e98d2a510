"""MAF training held to the float64 oracle optimizer step by optimizer step, at all twelve maf_grad_kernel<NT,L> (NT 1..4 x L 0..2) and
both routes behind them.

Per row of tests/maf_train_check.py's TRAIN_TABLE, on a fresh HipMAF with the start weights loaded (default init x 1.7; the base set
on the beta row), two chains of four optimizer steps, every step judged by nvp_train_check.check_step from the kernel's own state
before it (teacher forcing) with the MAF's float64 oracle and mask:
  stepwise   loss_grad (maf_grad_kernel + maf_reduce_kernel): the returned loss and gradient held directly to float64 -- whole vector,
             tensor by tensor, masked elements exactly 0 -- then adam_step (adam + maf_repack_kernel) and the state after it;
  epoch      nnest_maf_train_epoch with n_train = M, batch = M (and batch = 128 > M on the rows marked for it): maf_grad_kernel +
             maf_update_kernel (tile sum, Adam, both image writes through the position maps); the state before and after, and the
             accumulated loss.
After every step of either chain both images must follow the weights: forward and log_probs of 16 fresh rows against the float64
oracle at the new weights within the loss bound, and the round trip inverse(forward(x)) <= 1e-5 (the flow criterion of
tests/test_gpu_maf.py).  The bounds are those of tests/maf_train_check.py (none is set from a kernel's output); the float32 MAF
oracle passes the same checks on the same inputs in tests/test_maf_train_check.py.

The worst error / bound ratios per (NT, L) and route are printed at module teardown, one line each in the layout of
profiles/maf_train_oracle/ratios.txt, which holds those of the first run:
    pytest tests/test_gpu_maf_train_oracle.py -m gpu -s | grep '^maf_train_oracle' | cut -d' ' -f2-"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from tests import maf_train_check as mtc  # noqa: E402
from tests import nvp_train_check as ntc  # noqa: E402

WORST = {}
ROUND_TRIP = 1e-5


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import maf
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    yield maf
    for key in sorted(WORST):
        print('\nmaf_train_oracle %-14s %s' % (key, '  '.join('%s %.3g' % kv for kv in sorted(WORST[key].items()))), end='')
    print()


def note(c, route, **ratios):
    w = WORST.setdefault('%d %d %s' % (ntc.tiles(c.D), c.L, route), {})
    for k, r in ratios.items():
        w[k] = max(w.get(k, 0.0), r)


def fresh(hip, c):
    m = hip.HipMAF(c.D, c.H, c.B, c.L, seed=0)
    m.load_packed(ntc.start_weights(c))
    if c.beta:
        from nnest_amd.distributions import GeneralisedNormal
        m.set_base(GeneralisedNormal(torch.zeros(c.D), torch.ones(c.D), torch.tensor(c.beta)))
    assert [(n, tuple(s), o) for n, s, o in m.layer_shapes()] == [(n, tuple(s), o) for n, s, o in ntc.HostFlow(c).layer_shapes()]
    return m


def state(m):
    mm, vv = m.adam_moments()
    return m.store_packed(), mm, vv, m.adam_step_count()


def train_epoch(m, rows, batch, lr=ntc.LR, wd=ntc.WD):
    """nnest_maf_train_epoch over rows [n_train, D] (already in loader order, jitter applied) in minibatches of `batch`: the summed loss"""
    from nnest_amd import _lib
    rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(m.device)
    tot = torch.zeros((), dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        _lib.check(m._lib.nnest_maf_train_epoch(m._h, _lib.ptr(rows), rows.shape[0], int(batch), ctypes.c_float(lr), ctypes.c_float(wd),
                                                _lib.ptr(tot), _lib.current_stream(m.device)))
    return float(tot)


def images_follow(m, c, w_post, fresh_rows, what):
    """the forward image (forward, log_probs) and, through the round trip, the group-wise inverse on it, at the weights after the step"""
    ev = mtc.make_oracle(c, w_post)
    tol = mtc.BOUNDS['loss']
    z, ld = m.forward(fresh_rows)
    z64, ld64 = ev.forward(fresh_rows, f64=True)
    lp64 = ev.log_probs(fresh_rows, f64=True)
    out = {}
    for name, got, want in (('forward', z.cpu().numpy(), z64), ('logdet', ld.cpu().numpy(), ld64),
                            ('log_probs', m.log_probs(fresh_rows).cpu().numpy(), lp64)):
        ratio = np.abs(got.astype(np.float64) - want) / (tol * (1 + np.abs(want)))
        assert np.all(np.isfinite(got)) and np.max(ratio) < 1, '%s: %s of fresh rows off the float64 oracle at the new weights: error / bound %.3g' % (
            what, name, float(np.max(ratio)))
        out[name] = float(np.max(ratio))
    xb, _ = m.inverse(z)
    rt = float(torch.max(torch.abs(xb - torch.from_numpy(fresh_rows).to(xb.device))))
    assert rt <= ROUND_TRIP, '%s: round trip %.3g' % (what, rt)
    out['round_trip'] = rt / ROUND_TRIP
    return out


def chain_inputs(c):
    steps, _ = ntc.step_inputs(c)
    return steps, np.random.RandomState(7 + c.D).uniform(-1, 1, size=(16, c.D)).astype(np.float32)


@pytest.mark.parametrize('c', mtc.TRAIN_TABLE, ids=mtc.IDS)
def test_stepwise_route_vs_float64(hip, c):
    """maf_grad_kernel<NT,L> + maf_reduce_kernel, then adam_step"""
    m = fresh(hip, c)
    steps, rows16 = chain_inputs(c)
    shapes = m.layer_shapes()
    pre = state(m)
    assert pre[3] == 0 and not pre[1].any() and not pre[2].any()
    for k, s in enumerate(steps):
        what = '%s stepwise step %d' % (ntc.case_id(c), k + 1)
        s = mtc.away_from_kinks(c, pre[0], s)
        loss, grad = m.loss_grad(s['data'])
        rg = mtc.check_gradient(c, pre[0], s['data'], float(loss[0]), grad.cpu().numpy(), shapes, what=what)
        m.adam_step(grad, ntc.LR, ntc.WD)
        post = state(m)
        r = mtc.check_step(c, pre, post, s['data'], shapes, what=what)
        ri = images_follow(m, c, post[0], rows16, what)
        note(c, 'stepwise', returned_grad_whole=rg['grad_whole'], returned_grad_tensor=rg['grad_tensor'], train_loss=rg['train_loss'],
             grad_whole=r['grad_whole'], grad_tensor=r['grad_tensor'], exp_avg_sq=r['v'], weight=r['w'], **ri)
        pre = post


def epoch_cases():
    return [pytest.param(c, b, id='%s_batch%d' % (ntc.case_id(c), b)) for c in mtc.TRAIN_TABLE for b in c.batches]


@pytest.mark.parametrize('c,batch', epoch_cases())
def test_epoch_route_vs_float64(hip, c, batch):
    """maf_grad_kernel<NT,L> + maf_update_kernel: one minibatch per call of nnest_maf_train_epoch"""
    m = fresh(hip, c)
    steps, rows16 = chain_inputs(c)
    shapes = m.layer_shapes()
    pre = state(m)
    assert pre[3] == 0 and not pre[1].any() and not pre[2].any()
    for k, s in enumerate(steps):
        what = '%s epoch route batch %d step %d' % (ntc.case_id(c), batch, k + 1)
        s = mtc.away_from_kinks(c, pre[0], s)
        tot = train_epoch(m, s['data'], batch)
        post = state(m)
        r = mtc.check_step(c, pre, post, s['data'], shapes, what=what)
        lt = ntc.check_train_loss(tot / c.M, c.M, r['loss64'], bounds=mtc.BOUNDS, what=what)
        ri = images_follow(m, c, post[0], rows16, what)
        note(c, 'epoch', grad_whole=r['grad_whole'], grad_tensor=r['grad_tensor'], exp_avg_sq=r['v'], weight=r['w'], train_loss=lt, **ri)
        pre = post


@pytest.mark.parametrize('c,batch,n_train', mtc.EPOCH_CASES, ids=[ntc.case_id(e[0]) for e in mtc.EPOCH_CASES])
def test_one_launch_of_three_minibatches_equals_three_launches(hip, c, batch, n_train):
    """one call over minibatches (batch, batch, r) against three calls of one minibatch each: one producer per element and fixed
    summation orders, so w, exp_avg, exp_avg_sq and the step count agree bit for bit (beside the x_dim 7 / 50 / 100 rows of
    tests/test_gpu_maf.py::test_maf_epoch_call_equals_the_stepwise_loop)"""
    rows = np.random.RandomState(c.D + n_train).uniform(-1, 1, size=(n_train, c.D)).astype(np.float32)
    one, chain = fresh(hip, c), fresh(hip, c)
    tot = train_epoch(one, rows, batch)
    parts = [train_epoch(chain, rows[lo:lo + batch], batch) for lo in range(0, n_train, batch)]
    assert len(parts) == 3 and 0 < n_train - 2 * batch < batch
    a, b = state(one), state(chain)
    assert a[3] == b[3] == 3
    for name, x, y in zip(('w', 'exp_avg', 'exp_avg_sq'), a[:3], b[:3]):
        assert np.array_equal(x, y), '%s: %d elements differ, by up to %.3g' % (name, int(np.sum(x != y)), float(np.max(np.abs(x - y))))
    assert abs(tot - sum(parts)) <= 1e-6 * abs(sum(parts)), (tot, parts)


@pytest.mark.parametrize('n_valid', [1, 17, mtc.VALID_CASE.M + 17])
def test_validation_loss_through_train_epochs(hip, n_valid):
    """HipMAF.train_epochs, one epoch of one minibatch: losses[0, 1] n_valid against float64 at the weights after the step.  With
    n_valid <= batch that is -mean(log_probs); beyond it valid_sum's documented rule, the SUM of the means of the pieces of `batch`
    rows (maf.py), restated in float64"""
    c = mtc.VALID_CASE
    batch = c.M
    m = fresh(hip, c)
    steps, xv = ntc.step_inputs(c, steps=1, n_valid=n_valid)
    s = steps[0]
    res = m.train_epochs(s['xtrain'], xv, torch.from_numpy(np.ascontiguousarray(s['perm'][None])), torch.from_numpy(np.ascontiguousarray(s['noise'][None])),
                         jitter=ntc.JITTER, batch=batch, max_epochs=1, patience=50, lr=ntc.LR, weight_decay=ntc.WD)
    assert res['epochs_run'] == 1 and res['best_epoch'] == 1 and m.adam_step_count() == 1
    w_post = m.store_packed()
    losses = res['losses'].cpu().numpy()
    what = '%s n_valid %d' % (ntc.case_id(c), n_valid)
    if n_valid <= batch:
        lv = ntc.check_valid_loss(losses[0, 1], xv, w_post, mtc.make_oracle(c), bounds=mtc.BOUNDS, what=what, evaluator=mtc.evaluator(c))
    else:
        lp = mtc.make_oracle(c, w_post).log_probs(xv, f64=True)
        want = -sum(float(np.mean(lp[lo:lo + batch])) for lo in range(0, n_valid, batch))
        got = float(losses[0, 1]) * n_valid
        lv = abs(got - want) / (mtc.BOUNDS['loss'] * (1 + abs(want)))
        assert lv < 1, '%s: validation loss %.9g vs float64 %.9g' % (what, got, want)
    loss64 = mtc.make_oracle(c, ntc.start_weights(c)).loss_grad(s['data'], f64=True)[0]
    lt = ntc.check_train_loss(losses[0, 0], c.M, loss64, bounds=mtc.BOUNDS, what=what)
    note(c, 'epoch', valid_loss=lv, train_loss=lt)
