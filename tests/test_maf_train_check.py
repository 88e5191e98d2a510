"""tests/maf_train_check.py on the CPU: the float32 MAF oracle (orc.NVP(kind='maf').train_step: the minibatch and torch's Adam in
float32) plays the kernel over every row of the table the GPU kernels are held to, four steps each, and must pass every check of
nvp_train_check.check_step with the MAF's evaluator and mask: the standing proof that the reference alone is inside every bound.
Then the table itself (all twelve maf_grad_kernel<NT,L>, by the restated dispatch rule), the floor measurement, and planted faults,
each of which must be caught.

(The float32 oracle forms its bias corrections from the float32 constants 0.9f / 0.999f, the kernels from the doubles: see the header
of tests/test_nvp_train_check.py.)"""
import numpy as np
import pytest

from tests import maf_train_check as mtc
from tests import nvp_train_check as ntc
from tests.test_nvp_train_check import adam_f32

RUNS = {}


def oracle_run(c):
    """the float32 MAF oracle as the kernel: [(pre, post, step inputs, logged train loss, logged validation loss)]"""
    if c not in RUNS:
        o = mtc.make_oracle(c, ntc.start_weights(c))
        steps, xv = ntc.step_inputs(c)
        out = []
        for s in steps:
            pre = (o.w.copy(), o.m.copy(), o.v.copy(), o.t)
            s = mtc.away_from_kinks(c, pre[0], s)
            loss, _ = o.train_step(s['xtrain'], s['perm'], s['noise'], ntc.JITTER, ntc.LR, ntc.WD)
            out.append((pre, (o.w.copy(), o.m.copy(), o.v.copy(), o.t), s, loss / c.M, o.valid_loss(xv) / xv.shape[0]))
        RUNS[c] = (out, xv, ntc.HostFlow(c).layer_shapes())
    return RUNS[c]


def test_table_reaches_all_twelve_instantiations():
    """every row passes the library's limits as restated, names the (NT, L) it runs, and the B 3 rows alone cover NT 1..4 x L 0..2"""
    for c in mtc.TRAIN_TABLE + [e[0] for e in mtc.EPOCH_CASES]:
        inst = mtc.expected_instantiation(c)
        assert inst is not None and c.form == ('maf', 10 * inst[0] + inst[1]) and c.H == 16, ntc.case_id(c)
        assert c.B == 3 or mtc.instantiation(c.D, c.H, 3, c.L, c.M) is None or c.B in (1, 5), ntc.case_id(c)
    twelve = {(nt, l) for nt in (1, 2, 3, 4) for l in (0, 1, 2)}
    assert {mtc.expected_instantiation(c) for c in mtc.TRAIN_TABLE if c.B == 3} == twelve
    assert {mtc.expected_instantiation(c) for c in mtc.TRAIN_TABLE} == twelve
    assert {2, 32, 33, 64, 65, 96, 97, 128} <= {c.D for c in mtc.TRAIN_TABLE}
    assert {c.M for c in mtc.TRAIN_TABLE} == {1, 16, 17, 37, 100, 101, 128}
    assert {c.B for c in mtc.TRAIN_TABLE} == {1, 3, 5} and [c.beta for c in mtc.TRAIN_TABLE if c.beta] == [8.0]
    assert sum(1 for c in mtc.TRAIN_TABLE if c.batches == (c.M, 128)) >= 2
    assert len(set(mtc.TRAIN_TABLE)) == len(mtc.TRAIN_TABLE) <= 18
    assert {mtc.expected_instantiation(e[0])[0] for e in mtc.EPOCH_CASES} >= {3} and {e[0].L for e in mtc.EPOCH_CASES} >= {0}
    # the rule refuses what the library refuses: hidden widths other than 16, L 3, x_dim 129, an image beyond one CU's LDS
    assert mtc.instantiation(20, 32, 3, 1) is None and mtc.instantiation(20, 16, 3, 3) is None
    assert mtc.instantiation(129, 16, 3, 1) is None and mtc.instantiation(128, 16, 5, 2) is None and mtc.instantiation(128, 16, 3, 2) == (4, 2)


def test_gpu_maf_rows_reach_nt3():
    """the x_dim rows tests/test_gpu_maf.py runs the passes, the fused eval, the Metropolis kernel and the epoch call at include
    65 <= x_dim <= 96: maf_pass_kernel<3,1>, both maf_mh_kernel<3,1,*> (history on: DBG; the fused eval has it off) and the repack and
    position maps of that shape (DISPATCH_MAF switches on NT alone)"""
    from tests import test_gpu_maf as tgm

    def dims(test):
        marks = [m for m in getattr(tgm, test).pytestmark if m.name == 'parametrize' and m.args[0].split(',')[0] == 'D']
        assert len(marks) == 1, test
        return [row[0] for row in marks[0].args[1]]

    assert {ntc.tiles(D) for D in dims('test_maf_passes_vs_oracle')} == {1, 2, 3, 4}
    for test in ('test_maf_fused_eval_vs_oracle', 'test_maf_metropolis_kernel_vs_oracle', 'test_maf_epoch_call_equals_the_stepwise_loop'):
        assert 3 in {ntc.tiles(D) for D in dims(test)}, test


@pytest.mark.parametrize('c', mtc.TRAIN_TABLE, ids=mtc.IDS)
def test_float32_maf_oracle_passes_every_check(c):
    run, xv, shapes = oracle_run(c)
    o = mtc.make_oracle(c)
    for k, (pre, post, s, train, valid) in enumerate(run):
        what = '%s step %d' % (ntc.case_id(c), k + 1)
        r = mtc.check_step(c, pre, post, s['data'], shapes, what=what)
        ntc.check_train_loss(train, c.M, r['loss64'], bounds=mtc.BOUNDS, what=what)
        ntc.check_valid_loss(valid, xv, post[0], o, bounds=mtc.BOUNDS, what=what, evaluator=mtc.evaluator(c))
        mtc.check_gradient(c, pre[0], s['data'], train * c.M, mtc.make_oracle(c, pre[0]).loss_grad(s['data'])[1], shapes, what=what)


def test_float32_maf_oracle_needs_no_floor():
    """F: the smallest floor (in units of max|g64| over the vector) under which the float32 MAF oracle's recovered gradient passes the
    per-tensor bound on every table row and step; maf_train_check.MAF_FLOOR_MEASURED records it and BOUNDS['floor'] is 10 x that"""
    need, worst, kinked = 0.0, 0.0, 0
    for c in mtc.TRAIN_TABLE:
        run, _, shapes = oracle_run(c)
        plain, _ = ntc.step_inputs(c)
        for (pre, post, s, _, _), s0 in zip(run, plain):
            kinked += int(s['data'] is not s0['data'] and not np.array_equal(s['data'], s0['data']))
            ev = mtc.make_oracle(c, pre[0])
            g64 = ev.loss_grad(s['data'], f64=True)[1]
            g32 = ev.loss_grad(s['data'])[1]
            g = ntc.recover_gradient(pre, post, ntc.WD)[0]
            rtol = ntc.gradient_rtol(g32, g64, shapes, mtc.BOUNDS)
            for _, sl in ntc.tensor_slices(shapes):
                err, scale = np.max(np.abs(g - g64)[sl]), np.max(np.abs(g64[sl]))
                need = max(need, (err - rtol * scale) / np.max(np.abs(g64)))
                if scale > 0:
                    worst = max(worst, err / (rtol * scale))
    print('float32 MAF oracle: floor needed %.3g, worst error / (R max|g64|_t) %.3g, steps with a replaced row %d' % (need, worst, kinked))
    assert need <= mtc.MAF_FLOOR_MEASURED and mtc.BOUNDS['floor'] == 10 * mtc.MAF_FLOOR_MEASURED
    assert {k: v for k, v in mtc.BOUNDS.items() if k != 'floor'} == {k: v for k, v in ntc.BOUNDS.items() if k != 'floor'}
    assert worst < 0.2


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
FAULT_CASE = mtc.row(D=64, L=1, M=101)    # six full 16-row tiles and one of five rows
FAULT_STEP = 2


def fault_inputs(c=FAULT_CASE, k=FAULT_STEP):
    run, _, shapes = oracle_run(c)
    pre, _, s, _, _ = run[k]
    ev = mtc.make_oracle(c, pre[0])
    return pre, s['data'], shapes, ev, ev.loss_grad(s['data'])[1], ev.loss_grad(s['data'], f64=True)[1]


def test_the_numpy_adam_itself_passes():
    for k in range(ntc.STEPS):
        pre, data, shapes, _, g32, _ = fault_inputs(k=k)
        mtc.check_step(FAULT_CASE, pre, adam_f32(*pre, g32), data, shapes)


def test_fault_last_ragged_tile_dropped():
    """(a) the rows of the last, ragged 16-row tile never reach the sums (the mean still divides by M)"""
    c = FAULT_CASE
    pre, data, shapes, ev, _, _ = fault_inputs()
    full = 16 * (c.M // 16)
    assert 0 < c.M - full < 16
    g = (ev.loss_grad(data[:full])[1] * np.float32(full / c.M)).astype(np.float32)
    with pytest.raises(AssertionError, match='gradient flow'):
        mtc.check_step(c, pre, adam_f32(*pre, g), data, shapes)
    with pytest.raises(AssertionError, match='gradient'):
        mtc.check_gradient(c, pre[0], data, ev.loss_grad(data)[0], g, shapes)


def test_fault_masked_element_with_a_gradient():
    """(b) one masked element given 1e-3 of the largest gradient (a wrong mask degree, a wrong slot)"""
    c = FAULT_CASE
    pre, data, shapes, ev, g32, g64 = fault_inputs()
    i = int(np.flatnonzero(mtc.masked(c))[7])
    g = g32.copy()
    g[i] = np.float32(1e-3 * np.max(np.abs(g64)))
    with pytest.raises(AssertionError, match='masked flow'):
        mtc.check_step(c, pre, adam_f32(*pre, g), data, shapes)
    with pytest.raises(AssertionError, match='masked elements'):
        mtc.check_gradient(c, pre[0], data, ev.loss_grad(data)[0], g, shapes)


@pytest.mark.parametrize('c', [mtc.row(D=5, L=2, M=100), mtc.row(D=64, L=2, M=17)], ids=ntc.case_id)
def test_fault_smallest_tensor_scaled_by_one_percent(c):
    """(c) every element of the tensor with the smallest gradients 1 % too large, at two rows where that tensor (a translate net's
    first-layer bias) has under 1 % of the vector's largest gradient.  The whole-vector rule test_gpu_maf.py holds the gradient to,
    max|g - go| < 2e-4 max|go|, does not see it (the gap this module closes); the per-tensor bound does."""
    pre, data, shapes, ev, g32, g64 = fault_inputs(c)
    name, sl = min(ntc.tensor_slices(shapes), key=lambda t: np.max(np.abs(g64[t[1]])))
    ratio = np.max(np.abs(g64[sl])) / np.max(np.abs(g64))
    assert 0 < ratio < 0.01, ratio
    g = g32.copy()
    g[sl] *= np.float32(1.01)
    assert np.max(np.abs(g - g32)) < 0.5 * mtc.OLD_WHOLE_VECTOR_RULE * np.max(np.abs(g32))        # the old rule passes it
    assert np.max(np.abs(g - g64)) < ntc.BOUNDS['whole'] * (1e-3 + np.max(np.abs(g64)))           # and so does the whole-vector bound here
    with pytest.raises(AssertionError, match='gradient %s' % name.replace('.', r'\.')):
        mtc.check_step(c, pre, adam_f32(*pre, g), data, shapes)
    with pytest.raises(AssertionError, match='gradient %s' % name.replace('.', r'\.')):
        mtc.check_gradient(c, pre[0], data, ev.loss_grad(data)[0], g, shapes)


@pytest.mark.parametrize('layer', [0, 2, 4])
def test_fault_bias_tensors_of_the_two_nets_swapped(layer):
    """(d) the scale net's and the translate net's bias gradients of one block in each other's place (a wrong job target)"""
    c = FAULT_CASE
    pre, data, shapes, ev, g32, _ = fault_inputs()
    sl = {name: s for name, s in ntc.tensor_slices(shapes)}
    a, b = sl['flow.flows.1.scale_net.%d.bias' % layer], sl['flow.flows.1.translate_net.%d.bias' % layer]
    g = g32.copy()
    g[a], g[b] = g32[b], g32[a]
    with pytest.raises(AssertionError, match=r'gradient flow\.flows\.1\.\w+_net\.%d\.bias' % layer):
        mtc.check_step(c, pre, adam_f32(*pre, g), data, shapes)


def test_fault_bias_correction_one_step_late():
    """(e) Adam's bias corrections taken at step t instead of t + 1"""
    c = FAULT_CASE
    pre, data, shapes, _, g32, _ = fault_inputs()
    assert pre[3] == FAULT_STEP >= 1
    with pytest.raises(AssertionError, match='weight flow'):
        mtc.check_step(c, pre, adam_f32(*pre, g32, bc_step=pre[3]), data, shapes)
