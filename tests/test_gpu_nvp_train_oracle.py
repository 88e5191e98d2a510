"""The three kernels of nnest_nvp_train's epoch loop (train_kernel_rows<U>, train_kernel_grid<NT,1,L>, train_kernel<NT,NH,L,IMGLDS>)
held to the float64 oracle optimizer step by optimizer step, at every instantiation of the first two and every IMGLDS of the third.

Per table row of tests/nvp_train_check.py: the form is asserted through nnest_nvp_train_form (HipNVP.train_form_for), then a chain of
four launches of ONE minibatch each (n_train = M, max_epochs 1, a random permutation, explicit jitter noise, the Adam state carried
in the handle).  (w, exp_avg, exp_avg_sq, step) are read before and after every launch and given to check_step, which recovers the
kernel's gradient from the first moment and judges the step from the kernel's own state before it; the two logged losses are held
to float64 as well.  The bounds, and why they are what they are, are in tests/nvp_train_check.py; the float32 oracle passes the
same checks on the same inputs in tests/test_nvp_train_check.py.  Run with  pytest -m gpu -s  to see the error / bound ratios
(profiles/nvp_train_oracle/ratios.txt holds those of the first run)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from tests import nvp_train_check as ntc  # noqa: E402

WORST = {}


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import flow
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    yield flow
    for key in sorted(WORST):
        print('\nnvp_train_oracle %-12s %s' % (key, '  '.join('%s %.3g' % kv for kv in sorted(WORST[key].items()))), end='')
    print()


def note(form, **ratios):
    w = WORST.setdefault('%s %d' % form, {})
    for k, r in ratios.items():
        w[k] = max(w.get(k, 0.0), r)


def fresh(hip, c):
    nvp = hip.HipNVP(c.D, c.H, c.B, c.L, scale=c.scale, seed=0)
    nvp.load_packed(ntc.start_weights(c))
    if c.beta:
        from nnest_amd.distributions import GeneralisedNormal
        nvp.set_base(GeneralisedNormal(torch.zeros(c.D), torch.ones(c.D), torch.tensor(c.beta)))
    assert [(n, tuple(s), o) for n, s, o in nvp.layer_shapes()] == [(n, tuple(s), o) for n, s, o in ntc.HostFlow(c).layer_shapes()]
    return nvp


def state(nvp):
    m, v = nvp.adam_moments()
    return nvp.store_packed(), m, v, nvp.adam_step_count()


def launch(nvp, c, k, xtrain, xvalid, perm, noise, batch, res):
    """launch k of a chain: one epoch over xtrain in minibatches of `batch`, nothing restored at its end"""
    return nvp.train_epochs(xtrain, xvalid, torch.from_numpy(np.ascontiguousarray(perm[None])), torch.from_numpy(np.ascontiguousarray(noise[None])),
                            jitter=ntc.JITTER, batch=batch, max_epochs=1, patience=50, lr=ntc.LR, weight_decay=ntc.WD, epoch_offset=k,
                            resume=k > 0, finalize=False, result=res['result'] if k > 0 else None, one_cu=c.one_cu)


def run_chain(hip, c, batch):
    nvp = fresh(hip, c)
    assert nvp.train_form_for(batch, one_cu=c.one_cu) == c.form, ntc.case_id(c)
    o = ntc.make_oracle(c)
    steps, xv = ntc.step_inputs(c)
    shapes, res = nvp.layer_shapes(), None
    pre = state(nvp)
    assert pre[3] == 0 and not pre[1].any() and not pre[2].any()
    for k, s in enumerate(steps):
        what = '%s batch %d step %d' % (ntc.case_id(c), batch, k + 1)
        s = ntc.away_from_kinks(c, pre[0], s)
        res = launch(nvp, c, k, s['xtrain'], xv, s['perm'], s['noise'], batch, res)
        assert res['epochs_run'] == k + 1 and not res['stopped'], what
        post = state(nvp)
        r = ntc.check_step(pre, post, s['data'], o, ntc.LR, ntc.WD, shapes, what=what)
        losses = res['losses'].cpu().numpy()
        lt = ntc.check_train_loss(losses[0, 0], c.M, r['loss64'], what=what)
        lv = ntc.check_valid_loss(losses[0, 1], xv, post[0], o, what=what)
        note(c.form, grad_whole=r['grad_whole'], grad_tensor=r['grad_tensor'], exp_avg_sq=r['v'], weight=r['w'], train_loss=lt, valid_loss=lv)
        pre = post


def cases(table):
    return [pytest.param(c, b, id='%s_batch%d' % (ntc.case_id(c), b)) for c in table for b in c.batches]


@pytest.mark.parametrize('c,batch', cases(ntc.ROWS_TABLE))
def test_rows_form_steps_vs_float64(hip, c, batch):
    run_chain(hip, c, batch)


@pytest.mark.parametrize('c,batch', cases(ntc.GRID_TABLE))
def test_grid_form_steps_vs_float64(hip, c, batch):
    run_chain(hip, c, batch)


@pytest.mark.parametrize('c,batch', cases(ntc.SINGLE_TABLE))
def test_single_workgroup_steps_vs_float64(hip, c, batch):
    run_chain(hip, c, batch)


def test_single_workgroup_rows_reach_every_imglds(hip):
    seen = set()
    for c in ntc.SINGLE_TABLE:
        name, detail = fresh(hip, c).train_form_for(c.batches[0], one_cu=c.one_cu)
        assert name == 'single'
        seen.add(detail)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize('L,M', [(2, 96), (3, 64), (3, 1)])
def test_hidden_64_deep_nets_stage_the_rows_of_the_launch(hip, L, M):
    """train_kernel<1,4,2> / <1,4,3>: a staging area for 128 rows is more LDS than a compute unit has, so it is sized for the launch's
    rows (up to 96 at two hidden layers, 64 at three); loss_grad against float64, whole vector and tensor by tensor"""
    c = ntc.case(8, 64, 2, L, M, ('single', 0))
    assert ntc.expected_form(c) == c.form
    nvp = fresh(hip, c)
    assert nvp.train_form_for(M) == c.form
    steps, _ = ntc.step_inputs(c, steps=1)
    s = ntc.away_from_kinks(c, ntc.start_weights(c), steps[0])
    loss, grad = nvp.loss_grad(s['data'])
    ev = ntc.make_oracle(c, ntc.start_weights(c))
    l64, g64 = ev.loss_grad(s['data'], f64=True)
    g, g32 = grad.cpu().numpy().astype(np.float64), ev.loss_grad(s['data'])[1]
    assert abs(float(loss) - l64) < ntc.BOUNDS['loss'] * (1 + abs(l64))
    assert np.max(np.abs(g - g64)) < ntc.BOUNDS['whole'] * (1e-3 + np.max(np.abs(g64)))
    for name, sl, bound in ntc.tensor_bounds(g64, ntc.gradient_rtol(g32, g64, nvp.layer_shapes()), nvp.layer_shapes()):
        assert np.max(np.abs(g - g64)[sl]) <= bound, name


@pytest.mark.parametrize('c,batch,n_train', ntc.EPOCH_CASES, ids=[ntc.case_id(e[0]) for e in ntc.EPOCH_CASES])
def test_one_launch_of_three_minibatches_equals_the_chain(hip, c, batch, n_train):
    """one epoch of minibatches (batch, batch, r) in one launch against three launches of one minibatch each: one producer per
    element and fixed summation orders, so w, exp_avg and exp_avg_sq must agree bit for bit"""
    rng = np.random.RandomState(c.D + n_train)
    X = rng.uniform(-1, 1, size=(n_train, c.D)).astype(np.float32)
    xv = rng.uniform(-1, 1, size=(ntc.N_VALID, c.D)).astype(np.float32)
    perm = rng.permutation(n_train).astype(np.int32)
    noise = rng.randn(n_train, c.D).astype(np.float32)
    one = fresh(hip, c)
    assert one.train_form_for(batch) == c.form
    r1 = launch(one, c, 0, X, xv, perm, noise, batch, None)
    chain = fresh(hip, c)
    res, total = None, 0.0
    for k, lo in enumerate(range(0, n_train, batch)):
        rows = perm[lo:lo + batch]
        res = launch(chain, c, k, X[rows], xv, np.arange(rows.size, dtype=np.int32), noise[lo:lo + batch], batch, res)
        total += float(res['losses'].cpu().numpy()[0, 0]) * rows.size
    assert k == 2 and rows.size == n_train - 2 * batch
    a, b = state(one), state(chain)
    assert a[3] == b[3] == 3
    for name, x, y in zip(('w', 'exp_avg', 'exp_avg_sq'), a[:3], b[:3]):
        assert np.array_equal(x, y), '%s: %d elements differ, by up to %.3g' % (name, int(np.sum(x != y)), float(np.max(np.abs(x - y))))
    epoch = float(r1['losses'].cpu().numpy()[0, 0]) * n_train
    assert abs(epoch - total) <= 1e-6 * abs(total), (epoch, total)
    assert float(r1['losses'].cpu().numpy()[0, 1]) == float(res['losses'].cpu().numpy()[0, 1])


@pytest.mark.parametrize('n_valid', ntc.VALID_SIZES)
@pytest.mark.parametrize('c', ntc.VALID_CASES, ids=[ntc.case_id(c) for c in ntc.VALID_CASES])
def test_validation_loss_sizes(hip, c, n_valid):
    nvp = fresh(hip, c)
    assert nvp.train_form_for(c.M) == c.form
    steps, xv = ntc.step_inputs(c, steps=1, n_valid=n_valid)
    s = steps[0]
    res = launch(nvp, c, 0, s['xtrain'], xv, s['perm'], s['noise'], c.M, None)
    lv = ntc.check_valid_loss(res['losses'].cpu().numpy()[0, 1], xv, nvp.store_packed(), ntc.make_oracle(c), what='%s n_valid %d' % (ntc.case_id(c), n_valid))
    note(c.form, valid_loss=lv)
