"""nnest_nvp_vjp held to float64, and what the gradient tests of the side flows share: the shape table, the checker and the Adam-step
check used by tests/test_nvp_vjp_check.py (CPU: the float32 restatement plays the kernel), tests/test_gpu_nvp_vjp.py,
tests/test_gpu_fastslow_oracle.py and tests/test_gpu_cholesky.py.

The contract (include/nnest_hip.h): with L = <gz, z(X)> + gld * sum_rows logdet(X), nnest_nvp_vjp returns dL/dw in packed order and
dL/dx [M, D].  The yardstick is oracle/nvp_grad.py in float64.  assert_vjp_close judges

  dw   per state_dict tensor t:  max|gw - gw64|_t <= R max|gw64|_t; parameters whose gradient is zero by construction must be exactly 0
  dx   per row r:                |gx - gx64|[r, d] <= R max|gx64[r]|

with R = max(3e-5, 10 x the float32 restatement's worst such ratio ON THE SAME INPUT) -- the rule tests/nvp_train_check.py holds this
kernel's loss_grad to; the 10 is that file's allowance for another summation order.  R is measured against the float32 restatement,
never against the kernel.  No floor and no whole-vector term: every bound is relative to the tensor's, or the row's, own scale.

Measured on the CPU over VJP_TABLE (test_nvp_vjp_check.py::test_float32_restatement_passes_every_row re-measures them): the float32
restatement's worst ratio is 1.0e-6 for a tensor (x_dim 2, one row) and 6.5e-7 for a row (F32_WORST_DW, F32_WORST_DX), so ten times
it stays below the 3e-5 minimum and R is 3e-5 on every row of the table; against that R the restatement's worst error / bound is
0.033 (dw) and 0.022 (dx), and no row of the table needs a replacement.

Rows at a relu kink (a translate net's hidden unit within float32 rounding of 0 switches on in one precision and off in the other)
are replaced before a case runs, as nvp_train_check.away_from_kinks does it: a row whose own float32 and float64 gradients disagree
by more than that file's KINK is exchanged for a spare row, at most MAX_REPLACED per case; more is a failure, not a skip."""
import collections

import numpy as np

from tests import nvp_train_check as ntc

GLD = 0.37                   # the cotangent of sum_rows logdet in every vjp case
MAX_REPLACED = 8
F32_WORST_DW = 1.0e-6        # float32 restatement against float64 over VJP_TABLE: worst max|dw32 - dw64|_t / max|dw64|_t
F32_WORST_DX = 6.5e-7        # ... worst |dx32 - dx64| / max|dx64[row]|
R_CAP = 1e-4                 # no case may need more than this: a restatement that far off is an ill-conditioned input, not a bound

Row = collections.namedtuple('Row', 'D H B L M scale beta imglds')


def row(D, H, B, L, M, imglds, scale='', beta=0.0):
    return Row(D, H, B, L, M, scale, float(beta), imglds)


def row_id(c):
    return 'd%d_h%d_b%d_l%d_m%d' % c[:5] + ('_' + c.scale if c.scale else '') + ('_beta%g' % c.beta if c.beta else '')


def instantiation(c):
    """(NT, NH, L) of train_kernel for a row: NT 16-slot tiles per parity class, NH 16-wide tiles of the native hidden width"""
    return ntc.tiles(c.D), ntc.native_hidden(c.H) // 16, c.L


# nnest_train.hip TRAIN_SHAPES
TRAIN_SHAPES = [(nt, 1, l) for l in (0, 1, 2, 3) for nt in (1, 2, 3, 4)] + [(nt, 2, l) for l in (0, 1, 2, 3) for nt in (1, 2)] + \
    [(1, 4, l) for l in (0, 1, 2, 3)]

LDS_BYTES = 160 * 1024


def stage_tiles(c):
    """column tiles of train_kernel's staging area (StageMap::count)"""
    NT, NH, L = instantiation(c)
    return 2 * NT + 2 * (L + 1) * NH


def expected_imglds(c):
    """train_imglds' rule, restated: how many of the two fragment images live in LDS next to a staging area of 128 rows"""
    NT, NH, L = instantiation(c)
    net_floats = 256 * NH * (2 * NT + L * NH) + 16 * (NH * (1 + L) + NT)
    image = c.B * 2 * net_floats * 4
    stage = stage_tiles(c) * 128 * 16 * 4
    return 2 if stage + 2 * image <= LDS_BYTES - 256 else 1 if stage + image <= LDS_BYTES - 256 else 0


def rows_per_launch(c):
    """rows one launch stages (train_rows_per_launch): 128 wherever that fits a compute unit's LDS, else the largest multiple of 16
    that does -- a larger batch is split over launches and summed"""
    tile, room = stage_tiles(c) * 16 * 16 * 4, LDS_BYTES - 512          # (the kernel's own __shared__ variables take 312 bytes)
    return 128 if 8 * tile <= room else (room // tile) * 16


# One row for each of the 28 instantiations, then the extra rows.  Together: x_dim odd and at the tile edges (1, 2, 31, 32, 33, 65, 97,
# 128), hidden widths that are no tile width (10, 24, 40: zero-padded), num_blocks 1, 2, 3, 5, M 1, 16, 17, 37, 100, 128, every IMGLDS.
VJP_TABLE = [
    # native hidden 16                                    (NT, NH, L)
    row(1, 16, 3, 0, 16, 2),                            # (1, 1, 0)  x_dim 1: block 0 conditions on nothing
    row(33, 10, 2, 0, 37, 2),                           # (2, 1, 0)
    row(65, 16, 5, 0, 100, 1),                          # (3, 1, 0)
    row(97, 16, 3, 0, 17, 1),                           # (4, 1, 0)
    row(2, 16, 3, 1, 1, 2),                             # (1, 1, 1)
    row(50, 16, 3, 1, 100, 2),                          # (2, 1, 1)
    row(96, 10, 1, 1, 128, 2),                          # (3, 1, 1)
    row(128, 16, 2, 1, 37, 1),                          # (4, 1, 1)
    row(31, 16, 3, 2, 128, 2),                          # (1, 1, 2)
    row(64, 16, 2, 2, 16, 2),                           # (2, 1, 2)
    row(81, 10, 3, 2, 17, 1),                           # (3, 1, 2)
    row(128, 16, 5, 2, 100, 0),                         # (4, 1, 2)
    row(32, 16, 2, 3, 37, 2),                           # (1, 1, 3)
    row(33, 16, 3, 3, 100, 1),                          # (2, 1, 3)
    row(96, 16, 1, 3, 1, 2),                            # (3, 1, 3)
    row(128, 16, 2, 3, 128, 0),                         # (4, 1, 3)
    # native hidden 32
    row(9, 24, 5, 0, 17, 2),                            # (1, 2, 0)
    row(64, 32, 2, 0, 100, 2),                          # (2, 2, 0)
    row(9, 32, 3, 1, 100, 1),                           # (1, 2, 1)
    row(33, 24, 3, 1, 37, 0),                           # (2, 2, 1)
    row(31, 32, 2, 2, 16, 0),                           # (1, 2, 2)
    row(40, 24, 2, 2, 37, 0),                           # (2, 2, 2)
    row(32, 32, 1, 3, 128, 0),                          # (1, 2, 3)
    row(63, 32, 3, 3, 1, 0),                            # (2, 2, 3)
    # native hidden 64
    row(21, 40, 3, 0, 37, 1),                           # (1, 4, 0)
    row(32, 64, 1, 1, 100, 0),                          # (1, 4, 1)  the fast/slow hierarchy's coupling itself
    row(20, 64, 5, 2, 17, 0),                           # (1, 4, 2)  staging area sized by the rows of the launch
    row(8, 40, 2, 3, 37, 0),                            # (1, 4, 3)
    # extra rows
    row(20, 64, 5, 2, 128, 0),                          # (1, 4, 2) at 128 rows: two launches of 64
    row(8, 40, 2, 3, 128, 0),                           # (1, 4, 3) at 128 rows: two launches of 64
    row(40, 32, 2, 3, 128, 0),                          # (2, 2, 3) at 128 rows: 160 KB of staging leave no room for the kernel's statics
    row(20, 16, 3, 1, 100, 2, scale='translate'),
    row(21, 16, 3, 1, 37, 2, scale='constant'),         # scalars 0.2, -0.15, 0.1
    row(9, 32, 2, 2, 17, 0, scale='constant'),
    row(50, 16, 3, 1, 100, 2, beta=8),                  # the vjp must ignore the base distribution
]
N_INSTANTIATIONS = 28
LINEAR_ROWS = [VJP_TABLE[5], VJP_TABLE[32]]                         # test_vjp_is_linear_in_its_cotangent
LOSS_GRAD_ROWS = [VJP_TABLE[3], VJP_TABLE[28], VJP_TABLE[34]]       # test_vjp_reproduces_loss_grad
ADAM_SHAPES = [(20, 10, 3, 1), (9, 32, 3, 1), (32, 64, 1, 1)]       # test_adam_step_from_a_known_gradient: (D, H, B, L)

# test_fast_slow_gradient_vs_float64: (S, F, H, B, L, M)
FASTSLOW_CASES = [(1, 1, 16, 3, 1, 37), (1, 16, 16, 3, 1, 100), (16, 1, 16, 3, 1, 100), (16, 16, 16, 2, 1, 128), (7, 9, 32, 3, 2, 17),
                  (3, 5, 24, 1, 0, 1)]
FASTSLOW_STEP_CASES = [FASTSLOW_CASES[1], FASTSLOW_CASES[4]]         # test_fast_slow_one_adam_step
FASTSLOW_SPLINE_CASES = [(2, 2, 16, 3, 37), (5, 11, 32, 2, 100)]     # (S, F, H, B, M)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def layer_shapes(c):
    return ntc.HostFlow(c).layer_shapes()


def vjp_inputs(c, seed=0):
    """(w, X, gz, spare rows): default init x 1.7 (nonzero ScaleLayer scalars), rows uniform on [-1, 1], gz ~ N(0, 1) in float32"""
    w = ntc.start_weights(c, seed)
    rng = np.random.RandomState(7000 + 100 * c.D + 10 * c.B + c.L + c.M + seed)
    X = rng.uniform(-1, 1, size=(c.M, c.D)).astype(np.float32)
    gz = rng.randn(c.M, c.D).astype(np.float32)
    spare = rng.uniform(-1, 1, size=(MAX_REPLACED, c.D)).astype(np.float32)
    return w, X, gz, spare


def oracle_vjp(c, w, X, gz, gld, f32=False):
    import torch
    from oracle import nvp_grad
    return nvp_grad.vjp(w, X, gz, gld, c.D, c.H, c.B, c.L, c.scale, dtype=torch.float32 if f32 else torch.float64)


def kink(a, b):
    """whether a float32 result is further from its float64 one than float32 evaluation goes without a switched relu"""
    return bool(np.max(np.abs(a - b)) > ntc.KINK * (1e-3 + np.max(np.abs(b))))


def away_from_kinks(X, spare, disagree, what=''):
    """X with every row replaced whose own float32 and float64 gradients disagree (disagree(X, rows) -> bool, rows an index array),
    and how many were replaced; at most MAX_REPLACED, else AssertionError"""
    X, spare, replaced, every = X.copy(), list(spare), 0, np.arange(X.shape[0])
    for _ in range(4):
        if not disagree(X, every):
            return X, replaced
        bad = [r for r in every if disagree(X, every[r:r + 1])]
        replaced += len(bad)
        assert bad and replaced <= MAX_REPLACED and len(bad) <= len(spare), '%s: rows at a relu kink: %s (%d replaced so far)' % (
            what, bad, replaced)
        for r in bad:
            X[r] = spare.pop()
    raise AssertionError('%s: rows at a relu kink after four rounds of replacement' % what)


def screened_vjp_inputs(c, seed=0):
    """vjp_inputs with the rows at relu kinks replaced -> (w, X, gz, rows replaced)"""
    w, X, gz, spare = vjp_inputs(c, seed)

    def disagree(X, rows):
        a, b = oracle_vjp(c, w, X[rows], gz[rows], GLD, f32=True), oracle_vjp(c, w, X[rows], gz[rows], GLD)
        return kink(a[0], b[0]) or kink(a[1], b[1])

    X, replaced = away_from_kinks(X, spare, disagree, row_id(c))
    return w, X, gz, replaced


# ---- the checker -------------------------------------------------------------------------------------------------------------
def _slices(shapes):
    return ntc.tensor_slices(shapes) if len(shapes[0]) == 3 else \
        [(name, slice(off, off + int(np.prod(sh)))) for (name, sh), off in zip(shapes, np.cumsum([0] + [int(np.prod(s)) for _, s in shapes]))]


def worst_ratios(gw, gx, gw64, gx64, shapes, masked=None):
    """(worst max|gw - gw64|_t / max|gw64|_t over the tensors, worst |gx - gx64| / max|gx64[row]| over the rows); the parameters in
    `masked` do not count"""
    gw, gw64 = np.asarray(gw, np.float64).ravel(), np.asarray(gw64, np.float64).ravel()
    live = np.ones(gw.size, bool) if masked is None else ~np.asarray(masked, bool)
    dw = 0.0
    for _, s in _slices(shapes):
        scale = np.max(np.abs(gw64[s]), initial=0.0)
        if scale > 0 and live[s].any():
            dw = max(dw, float(np.max(np.abs(gw - gw64)[s][live[s]]) / scale))
    dx = 0.0
    if gx is not None:
        gx, gx64 = np.asarray(gx, np.float64), np.asarray(gx64, np.float64)
        scale = np.max(np.abs(gx64), axis=1, keepdims=True)
        ok = scale[:, 0] > 0
        if ok.any():
            dx = float(np.max((np.abs(gx - gx64) / np.where(scale > 0, scale, 1.0))[ok]))
    return dw, dx


def rtol(gw32, gx32, gw64, gx64, shapes, masked=None):
    """R of a case: 10 x the float32 restatement's worst per-tensor / per-row ratio on this input, at least 3e-5"""
    return max(ntc.BOUNDS['rtol_min'], ntc.BOUNDS['rtol_factor'] * max(worst_ratios(gw32, gx32, gw64, gx64, shapes, masked)))


def assert_vjp_close(gw, gx, gw64, gx64, shapes, R, masked=None, what=''):
    """dw tensor by tensor (shapes: [(name, shape, offset)] or [(name, shape)] in packed order), dx row by row (gx None: no dx),
    both within R of the tensor's / the row's largest float64 entry; `masked` (bool [n]): parameters whose gradient is zero by
    construction, which must be exactly 0.  Raises AssertionError naming the tensor and the element; returns the worst error / bound of
    dw and of dx."""
    gw, gw64 = np.asarray(gw, np.float64).ravel(), np.asarray(gw64, np.float64).ravel()
    assert gw.shape == gw64.shape, (gw.shape, gw64.shape)
    assert np.all(np.isfinite(gw)), '%s: dw not finite at %d' % (what, int(np.flatnonzero(~np.isfinite(gw))[0]))
    masked = np.zeros(gw.size, bool) if masked is None else np.asarray(masked, bool)
    assert masked.shape == gw.shape and np.all(gw64[masked] == 0) and np.any(gw64[~masked] != 0)
    slices = _slices(shapes)
    covered = np.zeros(gw.size, bool)
    for _, s in slices:
        covered[s] = True
    assert np.all(covered | masked), '%s: live parameters outside the named tensors' % what
    if np.any(gw[masked] != 0):
        i = int(np.flatnonzero(masked & (gw != 0))[0])
        where = [('%s[%d]' % (name, i - s.start)) for name, s in slices if s.start <= i < s.stop] or ['unused slot %d' % i]
        raise AssertionError('%s: %s is zero by construction, got %.9g' % (what, where[0], gw[i]))
    worst_w = 0.0
    for name, s in slices:
        if masked[s].all():
            continue
        err, bound = np.abs(gw - gw64)[s], R * float(np.max(np.abs(gw64[s])))
        k = int(np.argmax(err))
        assert err[k] <= bound, '%s: dw %s[%d]: %.9g vs float64 %.9g (error / bound %.3g, R %.3g)' % (
            what, name, k, gw[s][k], gw64[s][k], err[k] / bound if bound > 0 else np.inf, R)
        worst_w = max(worst_w, float(err[k] / bound) if bound > 0 else 0.0)
    worst_x = 0.0
    if gx is not None:
        gx, gx64 = np.asarray(gx, np.float64), np.asarray(gx64, np.float64)
        assert gx.shape == gx64.shape, (gx.shape, gx64.shape)
        assert np.all(np.isfinite(gx)), '%s: dx not finite' % what
        err, bound = np.abs(gx - gx64), R * np.max(np.abs(gx64), axis=1, keepdims=True) * np.ones_like(gx64)
        over = err - bound
        k = np.unravel_index(int(np.argmax(over)), over.shape)
        assert over[k] <= 0, '%s: dx[%d, %d]: %.9g vs float64 %.9g (error / bound %.3g, R %.3g)' % (
            what, k[0], k[1], gx[k], gx64[k], err[k] / bound[k] if bound[k] > 0 else np.inf, R)
        worst_x = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    return worst_w, worst_x


def assert_fastslow_spline_close(g, g64, g32, fs, masked, what=''):
    """a FastSlowSpline gradient in store_packed() order (fs: oracle.nvp_grad.FastSlow): the two spline stages tensor by tensor at
    spline_grad_check's GPU_RTOL_T and GPU_FLOOR (the floor relative to the stage's own largest gradient), the hidden-64 coupling with
    assert_vjp_close at R from the float32 composite g32.  Returns the worst error / bound of (the stages, the coupling)."""
    from tests import spline_grad_check as sgc
    g, g64, g32 = (np.asarray(a, np.float64).ravel() for a in (g, g64, g32))
    shapes = fs.layer_shapes()
    worst = 0.0
    for prefix, lo, hi in (('fast_flow.', 0, fs.n_fast), ('slow_flow.', fs.n_fast, fs.n_fast + fs.n_slow)):
        stage = [(n, s) for n, s, _ in shapes if n.startswith(prefix)]
        worst = max(worst, sgc.assert_grad_close(g[lo:hi], g64[lo:hi], stage, sgc.GPU_RTOL_T, sgc.GPU_FLOOR, '%s %s' % (what, prefix)))
    lo = fs.n_fast + fs.n_slow
    coupling = [(n, s) for n, s, _ in shapes if n.startswith('flow.')]
    R = rtol(g32[lo:], None, g64[lo:], None, coupling, masked[lo:])
    assert R <= R_CAP, (what, R)
    return worst, assert_vjp_close(g[lo:], None, g64[lo:], None, coupling, R, masked[lo:], what + ' coupling')[0]


def vjp_masked(c):
    shapes = layer_shapes(c)
    return ntc.masked_elements(shapes, ntc.HostFlow(c).num_params, c.D)


# ---- one Adam step from a known gradient --------------------------------------------------------------------------------------
def check_adam_step(pre, post, grad, lr, wd, what=''):
    """torch.optim.Adam with coupled weight decay, one step: pre / post = (w, m, v, t) as float32 arrays (t an int), grad the float32
    gradient the step was given.  With gi = grad + wd w:  m' = m + (gi - m)(1 - 0.9f) and v' = 0.999f v + (1 - 0.999f) gi^2 within
    4 eps32 of their terms (|m|, |grad| + |wd w|; v, (1 - 0.999f)(|grad| + |wd w|)^2); w' = w - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + 1e-8) from the kernel's own m', v' at step t + 1 within
    2 ulp(w) + 64 eps32 |update| (tests/nvp_train_check.py's bounds).  Returns the worst error / bound of (m', v', w')."""
    w, m, v, t = pre
    w1, m1, v1, t1 = post
    assert int(t1) == int(t) + 1, '%s: step count %d after %d' % (what, t1, t)
    w_, m_, v_, g_ = (np.asarray(a, np.float64) for a in (w, m, v, grad))
    w1_, m1_, v1_ = (np.asarray(a, np.float64) for a in (w1, m1, v1))
    for name, a in (('w', w1_), ('exp_avg', m1_), ('exp_avg_sq', v1_)):
        assert np.all(np.isfinite(a)), '%s: %s not finite' % (what, name)
    gi = g_ + float(np.float32(wd)) * w_
    # the terms: gi is a rounded sum of grad and wd w, so its rounding is relative to |grad| + |wd w|, which may be far above |gi|
    terms = np.abs(g_) + np.abs(float(np.float32(wd)) * w_)
    out = []
    for name, got, want, tol in (('exp_avg', m1_, m_ + (gi - m_) * ntc.C1, 4 * ntc.EPS32 * (np.abs(m_) + terms)),
                                 ('exp_avg_sq', v1_, ntc.B2 * v_ + ntc.C2 * gi ** 2, 4 * ntc.EPS32 * (v_ + ntc.C2 * terms ** 2))):
        d = np.abs(got - want)
        i = int(np.argmax(d - tol))
        assert d[i] <= tol[i], '%s: %s[%d] %.9g, the float64 step gives %.9g (tolerance %.3g)' % (what, name, i, got[i], want[i], tol[i])
        out.append(float(np.max(np.where(tol > 0, d / np.where(tol > 0, tol, 1.0), 0.0))))
    step = int(t) + 1
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    update = (lr / bc1) * m1_ / (np.sqrt(v1_) / np.sqrt(bc2) + ntc.ADAM_EPS)
    tol = ntc.BOUNDS['w_ulps'] * ntc.ulp32(w) + ntc.BOUNDS['w_rel'] * np.abs(update)
    d = np.abs(w1_ - (w_ - update))
    i = int(np.argmax(d / tol))
    assert d[i] <= tol[i], '%s: weight[%d] %.9g, Adam step %d from its own moments gives %.9g (from %.9g; tolerance %.3g)' % (
        what, i, w1_[i], step, (w_ - update)[i], w_[i], tol[i])
    out.append(float(d[i] / tol[i]))
    return tuple(out)


def adam_reference(w, m, v, t, grad, lr, wd):
    """the float32 step the way the kernel's adam_elem orders it (every operation rounded by itself), as a stand-in on the CPU"""
    f = np.float32
    w, m, v, g = (np.asarray(a, np.float32) for a in (w, m, v, grad))
    step = int(t) + 1
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    step_size, inv = f(lr / bc1), f(1.0 / np.sqrt(bc2))
    gi = g + f(wd) * w
    m1 = m + (gi - m) * (f(1.0) - f(0.9))
    v1 = v * f(0.999) + ((f(1.0) - f(0.999)) * gi) * gi
    return w - step_size * (m1 / (np.sqrt(v1) * inv + f(1e-8))), m1, v1, step
