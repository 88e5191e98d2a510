"""oracle/nvp_grad.py and tests/nvp_vjp_check.py on the CPU.  The float64 restatement is pinned to the C oracle (passes, log_probs and
loss_grad in every scale mode and base), to the reference's own autograd gradients of the fast/slow hierarchies (tests/golden/) and to
a finite difference of its dL/dx; then its float32 evaluation plays nnest_nvp_vjp over every row of VJP_TABLE and must pass the checker
the kernel is held to; then planted faults, each of which the checker must catch."""
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
from oracle import nvp_grad as ng  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import nvp_train_check as ntc  # noqa: E402
from tests import nvp_vjp_check as vc  # noqa: E402

G = os.path.join(os.path.dirname(__file__), 'golden')
IDS = [vc.row_id(c) for c in vc.VJP_TABLE]
# one shape per (L, scale): (D, H, B, L)
PIN_SHAPES = {0: (21, 16, 3), 1: (9, 32, 3), 2: (20, 64, 5), 3: (128, 16, 2)}
RUNS = {}


def run(c):
    """(w, X, gz, rows replaced, float32 (dw, dx), float64 (dw, dx), layer shapes, masked)"""
    if c not in RUNS:
        w, X, gz, replaced = vc.screened_vjp_inputs(c)
        RUNS[c] = (w, X, gz, replaced, vc.oracle_vjp(c, w, X, gz, vc.GLD, f32=True), vc.oracle_vjp(c, w, X, gz, vc.GLD), vc.layer_shapes(c),
                   vc.vjp_masked(c))
    return RUNS[c]


# ---- pins of the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.0, 8.0])
@pytest.mark.parametrize('scale', ['', 'translate', 'constant'])
@pytest.mark.parametrize('L', [0, 1, 2, 3])
def test_float64_restatement_vs_the_c_oracle(L, scale, beta):
    """float64 against float64: 1e-12 relative is ~1e4 roundings of 1e-16 (the two sum in different orders)"""
    D, H, B = PIN_SHAPES[L]
    c = ntc.case(D, H, B, L, 37, None, scale=scale, beta=beta)
    w = ntc.start_weights(c)
    X = np.random.RandomState(L).uniform(-1, 1, size=(37, D)).astype(np.float32)
    o = ntc.make_oracle(c, w)
    z, ld = o.forward(X, f64=True)
    z2, ld2 = ng.passes(w, X, D, H, B, L, scale)
    assert np.max(np.abs(z - z2)) <= 1e-12 * (1 + np.max(np.abs(z))) and np.max(np.abs(ld - ld2)) <= 1e-12 * (1 + np.max(np.abs(ld)))
    if scale == 'constant':
        assert np.any(w[-B:] != 0) and np.all(np.abs(ld2 - w[-B:].astype(np.float64).sum()) < 1e-12)   # s, not s D, per ScaleLayer
    lp, lp2 = o.log_probs(X, f64=True), ng.log_probs(w, X, D, H, B, L, scale, beta)
    assert np.max(np.abs(lp - lp2)) <= 1e-12 * (1 + np.max(np.abs(lp)))
    loss, g = o.loss_grad(X, f64=True)
    loss2, g2 = ng.loss_grad(w, X, D, H, B, L, scale, beta)
    assert abs(loss - loss2) <= 1e-12 * (1 + abs(loss))
    shapes = ntc.HostFlow(c).layer_shapes()
    masked = ntc.masked_elements(shapes, w.size, D)
    assert np.all(g2[masked] == 0) and np.all(g[masked] == 0)
    for name, s in ntc.tensor_slices(shapes):
        assert np.max(np.abs(g - g2)[s]) <= 1e-12 * np.max(np.abs(g[s])), name


def fixture_model(path):
    g = np.load(path)
    spline = 'spline' in os.path.basename(path)
    fs = ng.FastSlow(int(g['S']), int(g['F']), 16, 3, 1, kind='spline' if spline else 'nvp',
                     P={'fast': g['P_fast'], 'slow': g['P_slow']} if spline else None)
    data = g['X'][g['perms'][0][:100]] + np.float32(float(g['jitter'])) * g['noises'][0][:100]
    return g, fs, data


FS_FILES = sorted(glob.glob(os.path.join(G, 'fastslow_*.npz')) + glob.glob(os.path.join(G, 'fastslowspline_*.npz')))


@pytest.mark.parametrize('path', FS_FILES, ids=[os.path.basename(p)[:-4] for p in FS_FILES])
def test_fast_slow_composite_vs_the_references_autograd(path):
    """the reference's float32 autograd gradient of its own first minibatch, tensor by tensor: the fixture is one float32 evaluation,
    this module's float32 evaluation another, so the fixture is held to R from the latter (the checker's rule); spline stages at
    the spline tests' per-tensor tolerance"""
    g, fs, data = fixture_model(path)
    assert [n for n, _, _ in fs.layer_shapes()] == [str(k) for k in g['keys']] and fs.n == g['w_init'].size
    loss64, g64 = fs.loss_grad(g['w_init'], data)
    loss32, g32 = fs.loss_grad(g['w_init'], data, dtype=torch.float32)
    assert abs(loss64 - float(g['losses'][0])) < 1e-6 * (1 + abs(loss64))       # a float32 mean of ~100 terms of size ~loss
    masked = g64 == 0
    assert np.all(g['grads'][0][masked] == 0)
    if fs.kind == 'spline':
        vc.assert_fastslow_spline_close(g['grads'][0], g64, g32, fs, masked, os.path.basename(path))
        return
    R = vc.rtol(g32, None, g64, None, fs.layer_shapes(), masked)
    assert R <= vc.R_CAP, R
    vc.assert_vjp_close(g['grads'][0], None, g64, None, fs.layer_shapes(), R, masked, os.path.basename(path))


@pytest.mark.parametrize('path', [p for p in FS_FILES if 'spline' not in os.path.basename(p)],
                         ids=[os.path.basename(p)[:-4] for p in FS_FILES if 'spline' not in os.path.basename(p)])
def test_fast_slow_composite_vs_the_numpy_oracle(path):
    g, fs, _ = fixture_model(path)
    for tag in ('init', 'trained'):
        lp = orc.FastSlowNVP(fs.S, fs.F, 16, 3, 1, g['w_' + tag]).log_probs(g['x'], f64=True)
        lp2, lds = fs.log_probs(g['w_' + tag], g['x'], parts=True)
        assert np.max(np.abs(lp - lp2)) <= 1e-12 * (1 + np.max(np.abs(lp)))
        assert np.max(np.abs(lds[0] + lds[1] + lds[2] - g['ldf_' + tag])) < 2e-5 * (1 + np.max(np.abs(g['ldf_' + tag])))


def test_dx_against_a_central_finite_difference():
    """dL/dx of vjp in float64 against (L(x + h e) - L(x - h e)) / 2h, element by element: h = 1e-5 leaves a truncation error of
    h^2 |L'''| / 6 ~ 1e-10 and a rounding error of 1e-16 |L| / h ~ 1e-10, so 1e-7 of the row's scale is a wide margin for a smooth L
    (the rows are screened away from relu kinks, where L has no third derivative)"""
    c = vc.row(7, 16, 3, 2, 5, 2, scale='constant')
    w, X, gz, _ = vc.screened_vjp_inputs(c)
    _, gx = vc.oracle_vjp(c, w, X, gz, vc.GLD)

    def scalar(x):
        z, ld = ng.passes(w, x, c.D, c.H, c.B, c.L, c.scale)
        return float((z * gz.astype(np.float64)).sum() + vc.GLD * ld.sum())

    h, fd = 1e-5, np.empty_like(gx)
    for r in range(c.M):
        for d in range(c.D):
            e = np.zeros((c.M, c.D))
            e[r, d] = h
            fd[r, d] = (scalar(X.astype(np.float64) + e) - scalar(X.astype(np.float64) - e)) / (2 * h)
    assert np.all(np.abs(fd - gx) <= 1e-7 * np.max(np.abs(gx), axis=1, keepdims=True))


def test_loss_grad_is_the_special_case_of_vjp():
    c = vc.VJP_TABLE[-1]            # base_beta 8
    w, X, _, _ = vc.vjp_inputs(c)
    z, _ = ng.passes(w, X, c.D, c.H, c.B, c.L, c.scale)
    g = ng.loss_grad(w, X, c.D, c.H, c.B, c.L, c.scale, c.beta)[1]
    gv = vc.oracle_vjp(c, w, X, 8 * np.abs(z) ** 7 * np.sign(z) / c.M, -1.0 / c.M)[0]
    assert np.array_equal(g, gv)
    assert not np.allclose(g, ng.loss_grad(w, X, c.D, c.H, c.B, c.L, c.scale, 0.0)[1])


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_table_covers_every_instantiation_and_every_lds_layout():
    first = vc.VJP_TABLE[:vc.N_INSTANTIATIONS]
    assert sorted(vc.instantiation(c) for c in first) == sorted(vc.TRAIN_SHAPES) and len(vc.TRAIN_SHAPES) == 28
    for c in vc.VJP_TABLE:
        assert vc.expected_imglds(c) == c.imglds, vc.row_id(c)
        # the same rule as the training tables' (checked there against nnest_nvp_train_form on the GPU)
        assert ntc.expected_form(ntc.case(c.D, c.H, c.B, c.L, c.M, None, scale=c.scale, one_cu=True)) == ('single', c.imglds)
        assert vc.instantiation(c) in vc.TRAIN_SHAPES
    assert set(c.imglds for c in vc.VJP_TABLE) == {0, 1, 2}
    assert {1, 2, 31, 32, 33, 65, 97, 128} <= set(c.D for c in vc.VJP_TABLE)
    assert {10, 24, 40} <= set(c.H for c in vc.VJP_TABLE) and {1, 2, 3, 5} <= set(c.B for c in vc.VJP_TABLE)
    assert {1, 16, 17, 37, 100, 128} <= set(c.M for c in vc.VJP_TABLE)
    assert {'', 'translate', 'constant'} == set(c.scale for c in vc.VJP_TABLE) and any(c.beta == 8 for c in vc.VJP_TABLE)
    assert any(c.B == 1 and c.H == 64 and c.L == 1 for c in vc.VJP_TABLE)
    # the shapes whose staging area is sized by the rows of the launch, below and above what one launch stages
    deep = [(vc.instantiation(c), c.M, vc.rows_per_launch(c)) for c in vc.VJP_TABLE if vc.rows_per_launch(c) < 128]
    assert sorted(deep) == [((1, 4, 2), 17, 96), ((1, 4, 2), 128, 96), ((1, 4, 3), 37, 64), ((1, 4, 3), 128, 64), ((2, 2, 3), 1, 112),
                            ((2, 2, 3), 128, 112)]
    assert len(set(vc.VJP_TABLE)) == len(vc.VJP_TABLE)
    for c in vc.LINEAR_ROWS + vc.LOSS_GRAD_ROWS:
        assert c in vc.VJP_TABLE
    assert [c.scale for c in vc.LINEAR_ROWS] == ['', 'constant']
    assert vc.LOSS_GRAD_ROWS[1].M > vc.rows_per_launch(vc.LOSS_GRAD_ROWS[1]) and vc.LOSS_GRAD_ROWS[2].beta == 8


@pytest.mark.parametrize('c', vc.VJP_TABLE, ids=IDS)
def test_float32_restatement_passes_every_row(c):
    w, X, gz, replaced, (gw32, gx32), (gw64, gx64), shapes, masked = run(c)
    assert replaced <= vc.MAX_REPLACED
    R = vc.rtol(gw32, gx32, gw64, gx64, shapes, masked)
    assert R <= vc.R_CAP, R
    dw, dx = vc.assert_vjp_close(gw32, gx32, gw64, gx64, shapes, R, masked, vc.row_id(c))
    assert max(dw, dx) <= 1.0 / ntc.BOUNDS['rtol_factor'] + 1e-12
    if c.scale == 'constant':
        assert np.all(gw64[-c.B:] != 0) and np.all(w[-c.B:] != 0)


def test_measured_float32_ratios_are_the_recorded_ones():
    """F32_WORST_DW / F32_WORST_DX in the checker's header: re-measured here (another BLAS sums in another order: a factor 3)"""
    worst = np.max([vc.worst_ratios(r[4][0], r[4][1], r[5][0], r[5][1], r[6], r[7]) for r in map(run, vc.VJP_TABLE)], axis=0)
    print('float32 restatement over VJP_TABLE: worst dw ratio %.3g, worst dx ratio %.3g; rows replaced %d' % (
        worst[0], worst[1], sum(run(c)[3] for c in vc.VJP_TABLE)))
    assert worst[0] <= 3 * vc.F32_WORST_DW and worst[1] <= 3 * vc.F32_WORST_DX
    assert 10 * 3 * max(vc.F32_WORST_DW, vc.F32_WORST_DX) <= ntc.BOUNDS['rtol_min']     # so R is the 3e-5 minimum on every row


def test_the_base_distribution_does_not_enter_the_vjp():
    a, b = run(vc.VJP_TABLE[-1]), run(vc.VJP_TABLE[5])
    assert vc.VJP_TABLE[-1][:6] == vc.VJP_TABLE[5][:6] and np.array_equal(a[1], b[1])
    assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1])


# ---- the checker has teeth -----------------------------------------------------------------------------------------------------
def fails(c, gw, gx, match):
    w, X, gz, _, (gw32, gx32), (gw64, gx64), shapes, masked = run(c)
    R = vc.rtol(gw32, gx32, gw64, gx64, shapes, masked)
    vc.assert_vjp_close(gw32, gx32, gw64, gx64, shapes, R, masked)           # the unperturbed result passes ...
    with pytest.raises(AssertionError, match=match):                          # ... the perturbed one does not
        vc.assert_vjp_close(gw, gx, gw64, gx64, shapes, R, masked)


ODD = vc.VJP_TABLE[1]            # x_dim 33, 37 rows
CONSTANT = vc.VJP_TABLE[32]      # scale='constant', x_dim 21


def test_one_dx_element_off_by_a_thousandth_of_its_row():
    gw, gx = run(ODD)[4]
    gx = gx.copy()
    gx[5, 7] += 1e-3 * np.max(np.abs(gx[5]))
    fails(ODD, gw, gx, r'dx\[5, 7\]')


def test_dx_of_the_last_row_missing():
    gw, gx = run(ODD)[4]
    gx = gx.copy()
    gx[-1] = 0
    fails(ODD, gw, gx, r'dx\[36, ')


def test_dx_of_the_last_column_missing_at_odd_x_dim():
    gw, gx = run(ODD)[4]
    gx = gx.copy()
    gx[:, -1] = 0
    fails(ODD, gw, gx, r'dx\[\d+, 32\]')


@pytest.mark.parametrize('c', [ODD, CONSTANT], ids=['affine', 'constant'])
def test_gld_dropped(c):
    w, X, gz = run(c)[:3]
    gw, gx = vc.oracle_vjp(c, w, X, gz, 0.0, f32=True)
    fails(c, gw, gx, 'dw ')


def test_scale_layer_scalar_missing_its_m_gld_term():
    gw, gx = run(CONSTANT)[4]
    gw = gw.copy()
    gw[-CONSTANT.B:] -= CONSTANT.M * vc.GLD
    fails(CONSTANT, gw, gx, r'flows\.\d\.scale')


def test_parity_classes_of_gz_swapped():
    c = vc.VJP_TABLE[5]          # x_dim 50
    w, X, gz = run(c)[:3]
    swapped = np.empty_like(gz)
    swapped[:, 0::2], swapped[:, 1::2] = gz[:, 1::2], gz[:, 0::2]
    gw, gx = vc.oracle_vjp(c, w, X, swapped, vc.GLD, f32=True)
    fails(c, gw, gx, 'd[wx]')


def test_a_masked_parameter_with_a_gradient():
    gw, gx = run(ODD)[4]
    gw = gw.copy()
    gw[int(np.flatnonzero(run(ODD)[7])[3])] = 1e-30
    fails(ODD, gw, gx, 'zero by construction')


def test_kink_screen_replaces_rows_and_stops_at_its_cap():
    X = np.zeros((12, 3), np.float32)
    spare = np.ones((vc.MAX_REPLACED, 3), np.float32)
    X[[2, 5]] = 7
    out, n = vc.away_from_kinks(X, spare, lambda X, rows: bool(np.any(X[rows] == 7)))
    assert n == 2 and np.all(out[[2, 5]] == 1) and np.all(out[[0, 1, 3]] == 0)
    X[:9] = 7
    with pytest.raises(AssertionError, match='relu kink'):
        vc.away_from_kinks(X, spare, lambda X, rows: bool(np.any(X[rows] == 7)))


# ---- the Adam-step check -------------------------------------------------------------------------------------------------------
def test_adam_step_check_passes_the_float32_step_and_catches_faults():
    rng = np.random.RandomState(3)
    n, lr, wd = 500, 1e-3, 1e-6
    w, m, v, t = rng.randn(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), 0
    for k in range(3):
        g = (rng.randn(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        w1, m1, v1, t1 = vc.adam_reference(w, m, v, t, g, lr, wd)
        vc.check_adam_step((w, m, v, t), (w1, m1, v1, t1), g, lr, wd)
        with pytest.raises(AssertionError, match='step count'):
            vc.check_adam_step((w, m, v, t), (w1, m1, v1, t), g, lr, wd)
        with pytest.raises(AssertionError, match='exp_avg'):               # weight decay left out of the moments
            vc.check_adam_step((w, m, v, t), vc.adam_reference(w, m, v, t, g, lr, 0.0), g, lr, 1e-2)
        with pytest.raises(AssertionError, match='weight'):                # the bias correction of another step
            bad = vc.adam_reference(w, m, v, t + 1, g, lr, wd)
            vc.check_adam_step((w, m, v, t), (bad[0], m1, v1, t1), g, lr, wd)
        w, m, v, t = w1, m1, v1, t1
