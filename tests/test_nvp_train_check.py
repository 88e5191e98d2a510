"""tests/nvp_train_check.py on the CPU: the float32 oracle (orc.NVP.train_step: the reference's minibatch and torch's Adam in float32)
plays the kernel over every row of the tables the GPU kernels are held to, four steps each, and must pass every check: the standing
proof that the reference alone is inside every bound.  Then planted faults, each of which check_step must catch.

(The float32 oracle forms its bias corrections from the float32 constants 0.9f / 0.999f, torch and the kernels from the doubles: at
step 1 that alone is 6.4e-6 of the update, 54 of the 64 eps32 the weight check allows.  The kernels sit far below it.)"""
import numpy as np
import pytest

from tests import nvp_train_check as ntc

IDS = [ntc.case_id(c) for c in ntc.ALL_TABLES]
RUNS = {}


def adam_f32(w, m, v, t, g, lr=ntc.LR, wd=ntc.WD, bc_step=None, decoupled=False):
    """torch.optim.Adam with coupled weight decay in float32, operation by operation (the faulty kernels below are built from it)"""
    f = np.float32
    step = t + 1 if bc_step is None else bc_step
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    w, m, v, g = (np.asarray(a, np.float32) for a in (w, m, v, g))
    gi = g if decoupled else g + f(wd) * w
    m1 = m + (gi - m) * (f(1) - f(0.9))
    v1 = v * f(0.999) + ((f(1) - f(0.999)) * gi) * gi
    w0 = w * f(1.0 - lr * wd) if decoupled else w
    w1 = w0 - f(lr / bc1) * (m1 / (np.sqrt(v1) * f(1.0 / np.sqrt(bc2)) + f(1e-8)))
    return w1.astype(np.float32), m1.astype(np.float32), v1.astype(np.float32), t + 1


def oracle_run(c):
    """the float32 oracle as the kernel: [(pre, post, step inputs, logged train loss, logged validation loss)]"""
    if c not in RUNS:
        o = ntc.make_oracle(c, ntc.start_weights(c))
        steps, xv = ntc.step_inputs(c)
        out = []
        for s in steps:
            pre = (o.w.copy(), o.m.copy(), o.v.copy(), o.t)
            s = ntc.away_from_kinks(c, pre[0], s)
            loss, _ = o.train_step(s['xtrain'], s['perm'], s['noise'], ntc.JITTER, ntc.LR, ntc.WD)
            out.append((pre, (o.w.copy(), o.m.copy(), o.v.copy(), o.t), s, loss / c.M, o.valid_loss(xv) / xv.shape[0]))
        RUNS[c] = (out, xv, ntc.HostFlow(c).layer_shapes())
    return RUNS[c]


def test_tables_reach_the_forms_they_name():
    for c in ntc.ALL_TABLES + [e[0] for e in ntc.EPOCH_CASES]:
        assert ntc.expected_form(c) == c.form, ntc.case_id(c)
    assert sorted(c.form[1] for c in ntc.ROWS_TABLE if c.form[0] == 'rows') == [1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    assert sorted(c.form[1] for c in ntc.GRID_TABLE) == sorted(10 * nt + l for nt in (1, 2, 3, 4) for l in (0, 1, 2))
    assert all(c.form[0] == 'grid' for c in ntc.GRID_TABLE) and all(c.form[0] == 'single' for c in ntc.SINGLE_TABLE)
    assert set(c.form[1] for c in ntc.SINGLE_TABLE) == {0, 1, 2}
    assert len(set(ntc.ALL_TABLES)) == len(ntc.ALL_TABLES)


@pytest.mark.parametrize('c', ntc.ALL_TABLES, ids=IDS)
def test_float32_oracle_passes_every_check(c):
    run, xv, shapes = oracle_run(c)
    o = ntc.make_oracle(c)
    for k, (pre, post, s, train, valid) in enumerate(run):
        what = '%s step %d' % (ntc.case_id(c), k + 1)
        r = ntc.check_step(pre, post, s['data'], o, ntc.LR, ntc.WD, shapes, what=what)
        ntc.check_train_loss(train, c.M, r['loss64'], what=what)
        ntc.check_valid_loss(valid, xv, post[0], o, what=what)


def test_float32_oracle_needs_no_floor():
    """F: the smallest floor (in units of max|g64| over the vector) under which the float32 oracle's recovered gradient passes the
    per-tensor bound on every table row and step; nvp_train_check.FLOOR_MEASURED records it and BOUNDS['floor'] is 10 x that"""
    need, worst = 0.0, 0.0
    for c in ntc.ALL_TABLES:
        run, _, shapes = oracle_run(c)
        for pre, post, s, _, _ in run:
            ev = ntc.make_oracle(c, pre[0])
            g64 = ev.loss_grad(s['data'], f64=True)[1]
            g32 = ev.loss_grad(s['data'])[1]
            g = ntc.recover_gradient(pre, post, ntc.WD)[0]
            rtol = ntc.gradient_rtol(g32, g64, shapes)
            for _, sl in ntc.tensor_slices(shapes):
                err, scale = np.max(np.abs(g - g64)[sl]), np.max(np.abs(g64[sl]))
                need = max(need, (err - rtol * scale) / np.max(np.abs(g64)))
                worst = max(worst, err / (rtol * scale))
    print('float32 oracle: floor needed %.3g, worst error / (R max|g64|_t) %.3g' % (need, worst))
    assert need <= ntc.FLOOR_MEASURED and ntc.BOUNDS['floor'] == 10 * ntc.FLOOR_MEASURED
    assert worst < 0.2


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
FAULT_CASE = ntc.ROWS_TABLE[5]        # x_dim 64, M 100


def faulty(c, k, fault):
    """step k + 1 of the oracle's run redone by a kernel with one fault: (pre, post, data, shapes, oracle)"""
    run, _, shapes = oracle_run(c)
    pre, _, s, _, _ = run[k]
    ev = ntc.make_oracle(c, pre[0])
    data, kw = s['data'], {}
    if fault == 'last row dropped':
        data = data[:-1]
    elif fault == 'noise shifted':
        data = ntc.jittered(s['xtrain'], s['perm'], np.roll(s['noise'], 1, axis=0))
    elif fault == 'bias correction':
        kw = dict(bc_step=pre[3])
    elif fault == 'decoupled':
        kw = dict(decoupled=True)
    g = ev.loss_grad(data)[1]
    return pre, adam_f32(*pre, g, **kw), s['data'], shapes, ntc.make_oracle(c)


def test_the_numpy_adam_itself_passes():
    for k in range(ntc.STEPS):
        pre, post, data, shapes, o = faulty(FAULT_CASE, k, None)
        ntc.check_step(pre, post, data, o, ntc.LR, ntc.WD, shapes)


def test_fault_one_element_of_the_smallest_tensor():
    """3 x its per-tensor bound on one element of the tensor with the smallest gradients; the whole-vector bound does not see it"""
    c, k = FAULT_CASE, 2
    pre, _, data, shapes, o = faulty(c, k, None)
    ev = ntc.make_oracle(c, pre[0])
    g64, g32 = ev.loss_grad(data, f64=True)[1], ev.loss_grad(data)[1]
    masked = ntc.masked_elements(shapes, g64.size, c.D)
    name, sl, bound = min(ntc.tensor_bounds(g64, ntc.gradient_rtol(g32, g64, shapes), shapes), key=lambda b: b[2])
    i = sl.start + int(np.flatnonzero(~masked[sl])[0])
    g = g32.copy()
    g[i] += np.float32(3 * bound)
    assert np.max(np.abs(g - g64)) < 0.1 * ntc.BOUNDS['whole'] * (1e-3 + np.max(np.abs(g64)))
    with pytest.raises(AssertionError, match=r'gradient %s\[%d\]' % (name.replace('.', r'\.'), i - sl.start)):
        ntc.check_step(pre, adam_f32(*pre, g), data, o, ntc.LR, ntc.WD, shapes)


@pytest.mark.parametrize('fault,message', [('last row dropped', 'gradient flow'), ('noise shifted', 'gradient flow'),
                                           ('bias correction', 'weight flow'), ('decoupled', 'masked flow')])
def test_fault_is_caught(fault, message):
    pre, post, data, shapes, o = faulty(FAULT_CASE, 2, fault)
    with pytest.raises(AssertionError, match=message):
        ntc.check_step(pre, post, data, o, ntc.LR, ntc.WD, shapes)


def test_fault_masked_slot_with_a_moment():
    """an unused scale-net slot of a scale variant (w = m = v = 0) and a masked first-layer column of an affine flow"""
    for c, pick in ((ntc.SINGLE_TABLE[7], 0), (FAULT_CASE, None)):
        pre, post, data, shapes, o = faulty(c, 1, None)
        masked = ntc.masked_elements(shapes, pre[0].size, c.D)
        i = int(np.flatnonzero(masked)[0 if pick is not None else 3])
        if pick is not None:
            assert pre[0][i] == 0 and post[1][i] == 0 and post[2][i] == 0
        for which in (1, 2):
            bad = [a.copy() if isinstance(a, np.ndarray) else a for a in post]
            bad[which][i] += np.float32(1e-12)
            with pytest.raises(AssertionError, match='masked'):
                ntc.check_step(pre, tuple(bad), data, o, ntc.LR, ntc.WD, shapes)


def test_a_row_at_a_relu_kink_is_replaced():
    """a row built to put one hidden unit of a translate net exactly at its kink: away_from_kinks must find and replace it"""
    c = ntc.ROWS_TABLE[1]
    w = ntc.start_weights(c)
    shapes = {name: (shape, off) for name, shape, off in ntc.HostFlow(c).layer_shapes()}
    (H, D), ow = shapes['flow.flows.0.translate_net.0.weight']
    ob = shapes['flow.flows.0.translate_net.0.bias'][1]
    steps, _ = ntc.step_inputs(c, steps=1)
    s = steps[0]
    # block 0 conditions on the odd dimensions: move the row along unit 3's weights until W[3] . (x * mask) + b[3] = 0 in float64
    W3, x = w[ow + 3 * D:ow + 4 * D].astype(np.float64), s['data'][5].astype(np.float64)
    mask = np.arange(D) % 2 == 1
    x[mask] -= W3[mask] * (W3[mask] @ x[mask] + float(w[ob + 3])) / (W3[mask] @ W3[mask])
    kinked = dict(s, xtrain=s['xtrain'].copy(), noise=s['noise'].copy())
    kinked['xtrain'][s['perm'][5]] = x.astype(np.float32)
    kinked['noise'][5] = 0
    kinked['data'] = ntc.jittered(kinked['xtrain'], s['perm'], kinked['noise'])
    pre = abs(W3[mask] @ kinked['data'][5].astype(np.float64)[mask] + float(w[ob + 3]))
    assert pre < 1e-6
    out = ntc.away_from_kinks(c, w, kinked)
    changed = np.flatnonzero(np.any(out['data'] != kinked['data'], axis=1))
    assert list(changed) == [5]
    assert ntc.away_from_kinks(c, w, s) is s


def test_fault_step_count():
    pre, post, data, shapes, o = faulty(FAULT_CASE, 0, None)
    with pytest.raises(AssertionError, match='step count'):
        ntc.check_step(pre, post[:3] + (post[3] + 1,), data, o, ntc.LR, ntc.WD, shapes)


def test_loss_helpers_catch_a_wrong_normalisation():
    c = FAULT_CASE
    run, xv, _ = oracle_run(c)
    pre, post, s, train, valid = run[0]
    o = ntc.make_oracle(c)
    loss64 = ntc.make_oracle(c, pre[0]).loss_grad(s['data'], f64=True)[0]
    with pytest.raises(AssertionError, match='train loss'):
        ntc.check_train_loss(train * c.M / (c.M - 1), c.M, loss64)
    with pytest.raises(AssertionError, match='validation loss'):
        ntc.check_valid_loss(valid * xv.shape[0], xv, post[0], o)
