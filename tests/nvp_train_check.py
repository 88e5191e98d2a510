"""One optimizer step of RealNVP training held to float64, from Adam's state alone; shared by tests/test_nvp_train_check.py (CPU:
the float32 oracle plays the kernel) and tests/test_gpu_nvp_train_oracle.py (GPU: the three kernels of nnest_nvp_train's epoch loop).

The epoch entry exposes no gradient, but it leaves (w, m, v, t) readable, and a launch can be one minibatch.  With the kernel's
constants c = 1.0f - 0.9f and 0.9f (both exact in float64) its first moment is m' = m + (gi - m) c, so

    gi_k = (m' - 0.9f m) / c        the gradient the kernel fed to Adam (weight decay included)
    g_k  = gi_k - wd w              the kernel's dloss/dw

check_step judges ONE step from the state before it (teacher forcing: no error is carried from step to step):

  gradient   g_k against g64 = the float64 oracle's gradient at w, on the float32 rows the kernel saw
               whole vector   max|g_k - g64| < 1e-4 (1e-3 + max|g64|)                       (the bound loss_grad is held to)
               per tensor     max|g_k - g64|_t <= R max|g64|_t + F max|g64|_all
                              R = max(3e-5, 10 x the float32 oracle's worst per-tensor relative error on this input)
  masked     parameters whose gradient is zero by construction (first-layer columns of the dimensions a block does not condition on,
             last-layer rows of the dimensions it passes through, the scale-net slots of the scale variants): the step with g = 0.
             torch's Adam decays them like any other weight (coupled: gi = wd w), so m' and v' are held to the zero-gradient step
             within float32 rounding of its terms -- 4 eps32 (|m| + |wd w|), 4 eps32 (v + 1e-3 (wd w)^2) -- which for w = m = v = 0 (every
             unused scale-net slot) is m' == 0, v' == 0, w' == w exactly.
  v          v' = 0.999f v + (1 - 0.999f) gi_k^2: relative 1e-5 plus the rounding of the recovery (second_moment_slack)
  w          w' = w - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + 1e-8), in float64 from the kernel's own m', v', bias corrections at step
             t + 1: |difference| <= 2 ulp(w) + 64 eps32 |update|
  t          t' == t + 1

F, measured: the float32 oracle (orc.NVP.train_step) run as the kernel over every row of the three tables below, four steps each,
needs NO floor: with R as above its recovered gradient stays inside R max|g64|_t for every tensor (worst error / bound 0.114 with
F = 0; FLOOR_MEASURED below, re-measured by test_nvp_train_check.py::test_float32_oracle_needs_no_floor).  F = 10 x that = 0: the
per-tensor bound is purely relative to the tensor's own largest gradient.

Validation loss: the kernels log it as the reference does, mean over the rows and then / len(dataset) once more (trainer.py:418),
so it is losses[0, 1] n_valid that is compared with -mean(log_probs) in float64, as losses[0, 0] n_train is with the batch loss."""
import collections
import re

import numpy as np

EPS32 = 2.0 ** -23
B1 = float(np.float32(0.9))
C1 = float(np.float32(1.0) - np.float32(0.9))       # the kernel's (1.0f - b1): exact in float32, and B1 + C1 == 1
B2 = float(np.float32(0.999))
C2 = float(np.float32(1.0) - np.float32(0.999))
ADAM_EPS = float(np.float32(1e-8))
JITTER, LR, WD, STEPS, N_VALID = 0.01, 1e-3, 1e-6, 4, 16

FLOOR_MEASURED = 0.0                 # the smallest F the float32 oracle needs over the tables (see the header)
BOUNDS = dict(whole=1e-4, rtol_min=3e-5, rtol_factor=10.0, floor=10.0 * FLOOR_MEASURED, v_rtol=1e-5, w_ulps=2.0, w_rel=64.0 * EPS32,
              loss=3e-5)

Case = collections.namedtuple('Case', 'D H B L M scale beta one_cu form batches')


def case(D, H, B, L, M, form, scale='', beta=0.0, one_cu=False, batches=None):
    return Case(D, H, B, L, M, scale, float(beta), one_cu, form, tuple(batches or (M,)))


def case_id(c):
    return 'd%d_h%d_b%d_l%d_m%d' % c[:5] + ('_' + c.scale if c.scale else '') + ('_beta%g' % c.beta if c.beta else '') + \
        ('_onecu' if c.one_cu else '')


def tiles(D):
    """NT: 16-slot tiles per parity class"""
    return -(-(-(-D // 2)) // 16)


def native_hidden(H):
    return 16 if H <= 16 else 32 if H <= 32 else 64


def both(M):
    """the minibatch as the whole grid (batch = M) and as the only, ragged minibatch of a larger one (batch = 128 > M)"""
    return (M,) if M == 128 else (M, 128)


# ---- the cases.  form = what nnest_nvp_train_form must answer: (name, detail) ------------------------------------------------------
# rows form: native hidden 16, B 3, L 1, scale '', batch <= 128; detail U = NT.  Four rows per workgroup, and never fewer workgroups
# than the 3 * 2 * (2 U + 1) weight-gradient jobs need at eight per workgroup.
ROWS_TABLE = [
    case(2, 16, 3, 1, 1, ('rows', 1), batches=both(1)),
    case(31, 16, 3, 1, 37, ('rows', 1), batches=both(37)),
    case(32, 16, 3, 1, 128, ('rows', 1)),
    case(20, 10, 3, 1, 100, ('rows', 1), batches=both(100)),        # hidden 10, zero-padded to 16
    case(33, 16, 3, 1, 37, ('rows', 2), batches=both(37)),
    case(64, 16, 3, 1, 100, ('rows', 2), batches=both(100)),
    case(50, 16, 3, 1, 100, ('rows', 2), beta=8, batches=both(100)),
    case(65, 16, 3, 1, 101, ('rows', 3), batches=both(101)),        # 26 workgroups, the last with one row
    case(96, 16, 3, 1, 4, ('rows', 3), batches=both(4)),
    case(97, 16, 3, 1, 128, ('rows', 4)),
    case(128, 16, 3, 1, 3, ('rows', 4), batches=both(3)),           # fewer row workgroups than job workgroups
]


def _grid_table():
    out, ms = [], (100, 37, 128, 1)
    for L in (0, 1, 2):
        for D in (9, 40, 70, 128):
            NT = tiles(D)
            B = 2 if L == 1 else 4 if (L == 0 and NT <= 3) else 3
            M = ms[len(out) % 4]
            out.append(case(D, 16, B, L, M, ('grid', 10 * NT + L), batches=both(M) if len(out) in (1, 11) else None))
    return out


# grid form: all twelve train_kernel_grid<NT,1,L>; B = 2 at L = 1 (B = 3 is the rows form)
GRID_TABLE = _grid_table()

# one workgroup (train_kernel); detail = IMGLDS
SINGLE_TABLE = [
    case(9, 32, 3, 1, 100, ('single', 1)),
    case(40, 24, 2, 2, 37, ('single', 0), batches=both(37)),
    case(20, 64, 5, 1, 128, ('single', 0)),
    case(8, 40, 2, 3, 1, ('single', 0)),
    case(40, 16, 3, 3, 100, ('single', 1)),
    case(100, 16, 5, 1, 37, ('single', 0)),                         # 5 * 2 * 9 = 90 jobs: too many for the grid
    case(50, 16, 3, 1, 100, ('single', 2), one_cu=True),
    case(20, 16, 3, 1, 100, ('single', 2), scale='translate'),
    case(20, 16, 3, 1, 100, ('single', 2), scale='constant'),
    case(9, 32, 3, 1, 37, ('single', 1), beta=8),
]
ALL_TABLES = ROWS_TABLE + GRID_TABLE + SINGLE_TABLE

# one launch of three minibatches against the chain of three launches: (case, batch, n_train)
EPOCH_CASES = [(case(65, 16, 3, 1, 100, ('rows', 3)), 100, 230), (case(40, 16, 3, 2, 37, ('grid', 22)), 37, 2 * 37 + 30),
               (case(9, 32, 3, 1, 37, ('single', 1)), 37, 2 * 37 + 30)]
VALID_SIZES = (1, 17, 800)
VALID_CASES = [ROWS_TABLE[1], GRID_TABLE[5], SINGLE_TABLE[0]]


def expected_form(c):
    """the form of a case from the launch's own rules, restated: checked against every table row on the CPU, and against
    nnest_nvp_train_form on the GPU"""
    NT, Hn, NH = tiles(c.D), native_hidden(c.H), native_hidden(c.H) // 16
    net_floats = 256 * NH * (2 * NT + c.L * NH) + 16 * (NH * (1 + c.L) + NT)
    image_bytes = c.B * 2 * net_floats * 4
    grid = c.scale == '' and not c.one_cu and 2 * image_bytes <= 160 * 1024 - 1024 and NH == 1 and c.L <= 2 and \
        c.B * 2 * (2 * NT + c.L) <= 64
    if grid and Hn == 16 and c.L == 1 and c.B == 3:
        return ('rows', NT)
    if grid:
        return ('grid', 10 * NT + c.L)
    stage = (2 * NT + 2 * (c.L + 1) * NH) * 128 * 16 * 4
    return ('single', 2 if stage + 2 * image_bytes <= 160 * 1024 - 256 else 1 if stage + image_bytes <= 160 * 1024 - 256 else 0)


# ---- weights and data ------------------------------------------------------------------------------------------------------
class HostFlow(object):
    """the packed layout of a HipNVP without a device: layer_shapes() and default_init() are HipNVP's own"""

    def __init__(self, c):
        from nnest_amd import flow
        self.D, self.H, self.B, self.L, self.scale = c.D, c.H, c.B, c.L, c.scale
        ns = c.H * c.D + c.H + c.L * (c.H * c.H + c.H) + c.D * c.H + c.D
        self.num_params = 2 * c.B * ns + (c.B if c.scale == 'constant' else 0)
        self._cls = flow.HipNVP

    def layer_shapes(self):
        return self._cls.layer_shapes(self)

    def default_init(self, seed):
        return self._cls.default_init(self, seed)


def start_weights(c, seed=0):
    """default init x 1.7 (tests/test_gpu_shapes.py::make); scale='constant': the scalars of tests/test_gpu_scale.py, cycled over B"""
    w = (HostFlow(c).default_init(seed) * 1.7).astype(np.float32)
    if c.scale == 'constant':
        w[-c.B:] = np.resize(np.float32([0.2, -0.15, 0.1]), c.B)
    return w


def make_oracle(c, w=None):
    from oracle import oracle as orc
    return orc.NVP(c.D, c.H, c.B, c.L, w, scale=c.scale, base_beta=c.beta)


def step_inputs(c, steps=STEPS, n_valid=N_VALID, M=None):
    """per step: xtrain [M, D] (M rows of a pool, drawn anew), a random permutation, noise in loader order and the float32 rows the
    kernel sees, data[k] = xtrain[perm[k]] + float32(jitter) noise[k]; plus the validation rows"""
    M = c.M if M is None else M
    rng = np.random.RandomState(1000 * c.D + 10 * c.B + c.L)
    pool = rng.uniform(-1, 1, size=(4 * M + 64, c.D)).astype(np.float32)
    out = []
    for _ in range(steps):
        xtrain = pool[rng.choice(pool.shape[0], M, replace=False)]
        perm = rng.permutation(M).astype(np.int32)
        if M > 2:
            assert not np.array_equal(perm, np.arange(M))
        noise = rng.randn(M, c.D).astype(np.float32)
        out.append(dict(xtrain=xtrain, perm=perm, noise=noise, data=jittered(xtrain, perm, noise),
                        spare=pool[rng.choice(pool.shape[0], 8, replace=False)]))
    return out, rng.uniform(-1, 1, size=(n_valid, c.D)).astype(np.float32)


def jittered(xtrain, perm, noise, jitter=JITTER):
    return (xtrain[perm] + np.float32(jitter) * noise).astype(np.float32)


# A translate net's relu has a kink: a row that puts a hidden unit's pre-activation within float32 rounding of 0 switches the unit on
# in one precision and off in the other, and the float64 gradient is then no limit of ANY float32 evaluation (first met at hidden 64,
# step 4: one row, one unit, 1.5e-2 of the gradient scale, the float32 oracle and the kernel agreeing with each other to 1e-7).  As
# the spline checks keep rows away from knots, a step's rows are screened BEFORE the step is taken, at the weights it starts from:
# the float32 oracle's gradient of the same rows must be within KINK of the float64 one -- 2.5 x the worst it shows anywhere on the
# tables (3.9e-6, hidden 64 / three layers) and 1000 x below a switched unit -- else the rows whose own gradients disagree are replaced.
KINK = 1e-5


def away_from_kinks(c, w, s, evaluator=None):
    """the step's inputs with every row at a relu kink (at weights w) replaced by a spare row; most often s itself.  evaluator(w):
    the oracle at weights w (default: the RealNVP of the case, make_oracle(c, w))"""
    ev = make_oracle(c, w) if evaluator is None else evaluator(w)

    def disagree(rows):
        g64, g32 = ev.loss_grad(rows, f64=True)[1], ev.loss_grad(rows)[1]
        return np.max(np.abs(g32 - g64)) > KINK * (1e-3 + np.max(np.abs(g64)))

    spare = list(s['spare'])
    for _ in range(4):
        if not disagree(s['data']):
            return s
        bad = [r for r in range(s['data'].shape[0]) if disagree(s['data'][r:r + 1])]
        assert bad and len(bad) <= len(spare), (case_id(c), bad)
        xtrain = s['xtrain'].copy()
        for r in bad:
            xtrain[s['perm'][r]] = spare.pop()
        s = dict(s, xtrain=xtrain, data=jittered(xtrain, s['perm'], s['noise']))
    raise AssertionError('%s: rows at a relu kink after four replacements' % case_id(c))


# ---- the checker -----------------------------------------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def tensor_slices(layer_shapes):
    return [(name, slice(off, off + max(1, int(np.prod(shape))))) for name, shape, off in layer_shapes]


def masked_elements(layer_shapes, n, D):
    """bool [n]: parameters whose gradient is zero by construction.  Block b conditions on the dimensions with (d + b) odd
    (networks.py:333-334): the first layer's columns of the others see zeros, and the last layer's rows of the conditioning dimensions
    pass through (log_s = t = 0 there).  Everything outside layer_shapes (the scale variants' scale-net slots) is unused."""
    masked = np.ones(n, bool)
    last = max(int(re.match(r'flow\.flows\.\d+\.\w+\.(\d+)\.', name).group(1)) for name, shape, _ in layer_shapes if len(shape))
    blocks = sorted(set(int(name.split('.')[2]) for name, shape, _ in layer_shapes if len(shape)))
    for name, shape, off in layer_shapes:
        if len(shape) == 0:
            masked[off] = False
            continue
        parts = name.split('.')
        b, layer = blocks.index(int(parts[2])), int(parts[4])
        cond = (np.arange(D) + b) % 2 == 1
        live = np.ones(shape, bool)
        if layer == 0 and parts[5] == 'weight':
            live[:, ~cond] = False
        if layer == last:
            live[cond] = False
        masked[off:off + live.size] = ~live.ravel()
    return masked


def recover_gradient(pre, post, wd):
    """(g_k, gi_k) in float64 from the first moments before and after the step"""
    w, m = np.asarray(pre[0], np.float64), np.asarray(pre[1], np.float64)
    gi = (np.asarray(post[1], np.float64) - B1 * m) / C1
    return gi - float(np.float32(wd)) * w, gi


def second_moment_slack(pre, post, gi):
    """What the recovery's rounding does to v'.  The kernel forms m' = fl(m + fl(fl(gi - m) c)): three roundings, at most half an ulp
    of gi - m, of (gi - m) c ~ m' - m and of m' each.  Undone by (m' - 0.9f m) / c they leave
        |gi_k - gi| <= delta = ulp(gi_k - m) / 2 + (ulp(m' - m) + ulp(m')) / (2 c),
    and v' = .. + (1 - 0.999f) gi^2 moves by (1 - 0.999f) (2 |gi_k| delta + delta^2)."""
    m, m1 = np.asarray(pre[1], np.float64), np.asarray(post[1], np.float64)
    delta = 0.5 * ulp32(gi - m) + (ulp32(m1 - m) + ulp32(m1)) / (2 * C1)
    return C2 * (2 * np.abs(gi) * delta + delta ** 2)


def gradient_rtol(g32, g64, layer_shapes, bounds=BOUNDS):
    """R: the float32 oracle's worst per-tensor relative error on this input, x 10 (another summation order), at least 3e-5"""
    worst = 0.0
    for _, s in tensor_slices(layer_shapes):
        scale = np.max(np.abs(g64[s]))
        if scale > 0:
            worst = max(worst, float(np.max(np.abs(np.asarray(g32, np.float64)[s] - g64[s])) / scale))
    return max(bounds['rtol_min'], bounds['rtol_factor'] * worst)


def tensor_bounds(g64, rtol, layer_shapes, bounds=BOUNDS):
    """[(name, slice, R max|g64|_t + F max|g64|_all)]"""
    floor = bounds['floor'] * np.max(np.abs(g64))
    return [(name, s, rtol * float(np.max(np.abs(g64[s]))) + floor) for name, s in tensor_slices(layer_shapes)]


def rebuilt(oracle):
    """the default evaluator factory: w -> an oracle of `oracle`'s class, shape, scale variant and base at weights w (a RealNVP)"""
    return lambda w: type(oracle)(oracle.D, oracle.H, oracle.B, oracle.L, w, scale=oracle.scale, base_beta=oracle.base_beta)


def check_step(pre, post, data, oracle, lr, wd, layer_shapes, bounds=BOUNDS, what='', evaluator=None, masked=None):
    """One optimizer step: pre / post = (w, m, v, t) as float32 arrays (t an int), data the float32 rows of the minibatch, oracle an
    orc.NVP of the flow's shape (its own weights are not touched).  Raises AssertionError naming the tensor and the element; returns
    the worst error / bound per check and the float64 batch loss.
    Another flow with the same packed layout supplies evaluator(w) -> its oracle at weights w (default rebuilt(oracle)) and masked,
    the parameters whose gradient is zero by construction: a bool [n] array or a callable (layer_shapes, n, D) -> one (default
    masked_elements, RealNVP's rule)."""
    w, m, v, t = pre
    w1, m1, v1, t1 = post
    n = w.size
    ev = (rebuilt(oracle) if evaluator is None else evaluator)(w)
    loss64, g64 = ev.loss_grad(data, f64=True)
    _, g32 = ev.loss_grad(data)
    assert g64.size == n and all(np.asarray(a).size == n for a in (m, v, w1, m1, v1))
    assert int(t1) == int(t) + 1, '%s: step count %d after %d' % (what, t1, t)
    masked = masked_elements if masked is None else masked
    masked = np.asarray(masked(layer_shapes, n, oracle.D) if callable(masked) else masked, bool)
    assert masked.shape == (n,)
    assert np.all(g64[masked] == 0) and np.any(g64[~masked] != 0)
    wd32 = float(np.float32(wd))
    w_, m_, v_ = (np.asarray(a, np.float64) for a in (w, m, v))
    w1_, m1_, v1_ = (np.asarray(a, np.float64) for a in (w1, m1, v1))
    for name, a in (('w', w1_), ('exp_avg', m1_), ('exp_avg_sq', v1_)):
        assert np.all(np.isfinite(a)), '%s: %s not finite at %d' % (what, name, int(np.flatnonzero(~np.isfinite(a))[0]))
    out = {}

    def locate(i):
        for name, s in tensor_slices(layer_shapes):
            if s.start <= i < s.stop:
                return '%s[%d]' % (name, i - s.start)
        return 'unused slot %d' % i

    # masked parameters: the zero-gradient step
    gi0 = wd32 * w_
    for name, got, want, tol in (('exp_avg', m1_, m_ + (gi0 - m_) * C1, 4 * EPS32 * (np.abs(m_) + np.abs(gi0))),
                                 ('exp_avg_sq', v1_, B2 * v_ + C2 * gi0 ** 2, 4 * EPS32 * (v_ + C2 * gi0 ** 2))):
        bad = masked & (np.abs(got - want) > tol)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError('%s: masked %s: %s %.9g, the zero-gradient step gives %.9g' % (what, locate(i), name, got[i], want[i]))
    still = masked & (m1_ == 0)
    assert np.array_equal(np.asarray(w1)[still], np.asarray(w)[still]), '%s: a masked parameter with zero moment moved' % what

    # gradient
    g, gi = recover_gradient(pre, post, wd)
    err = np.abs(g - g64)
    gmax = float(np.max(np.abs(g64)))
    i = int(np.argmax(err))
    whole = bounds['whole'] * (1e-3 + gmax)
    assert err[i] < whole, '%s: gradient %s: %.9g vs float64 %.9g (whole-vector bound %.3g)' % (what, locate(i), g[i], g64[i], whole)
    out['grad_whole'] = float(err[i] / whole)
    rtol = gradient_rtol(g32, g64, layer_shapes, bounds)
    out['grad_tensor'] = 0.0
    for name, s, bound in tensor_bounds(g64, rtol, layer_shapes, bounds):
        k = int(np.argmax(err[s]))
        assert err[s][k] <= bound, '%s: gradient %s[%d]: %.9g vs float64 %.9g (error / per-tensor bound %.3g; R %.3g, F %.3g)' % (
            what, name, k, g[s][k], g64[s][k], err[s][k] / bound, rtol, bounds['floor'])
        out['grad_tensor'] = max(out['grad_tensor'], float(err[s][k] / bound))
    out['rtol'] = rtol

    # second moment, from the recovered gradient
    want = B2 * v_ + C2 * gi ** 2
    tol = bounds['v_rtol'] * want + second_moment_slack(pre, post, gi)
    d = np.abs(v1_ - want)
    live = ~masked
    i = int(np.flatnonzero(live)[np.argmax((d / np.maximum(tol, 1e-300))[live])])
    assert d[i] <= tol[i], '%s: exp_avg_sq %s: %.9g vs %.9g from the recovered gradient (tolerance %.3g)' % (what, locate(i), v1_[i], want[i], tol[i])
    out['v'] = float(d[i] / max(tol[i], 1e-300))

    # weights, from the kernel's own moments
    step = int(t) + 1
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    update = (lr / bc1) * m1_ / (np.sqrt(v1_) / np.sqrt(bc2) + ADAM_EPS)
    tol = bounds['w_ulps'] * ulp32(w) + bounds['w_rel'] * np.abs(update)
    d = np.abs(w1_ - (w_ - update))
    i = int(np.argmax(d / tol))
    assert d[i] <= tol[i], '%s: weight %s: %.9g, Adam step %d from its own moments gives %.9g (from %.9g; tolerance %.3g)' % (
        what, locate(i), w1_[i], step, (w_ - update)[i], w_[i], tol[i])
    out['w'] = float(d[i] / tol[i])
    out['loss64'] = float(loss64)
    return out


def check_train_loss(logged, n_train, loss64, bounds=BOUNDS, what=''):
    """losses[0, 0] n_train (the epoch's sum of batch means / len(dataset), one minibatch) against the float64 batch-mean loss"""
    got = float(logged) * n_train
    assert abs(got - loss64) < bounds['loss'] * (1 + abs(loss64)), '%s: train loss %.9g vs float64 %.9g' % (what, got, loss64)
    return abs(got - loss64) / (bounds['loss'] * (1 + abs(loss64)))


def check_valid_loss(logged, xvalid, w_post, oracle, bounds=BOUNDS, what='', evaluator=None):
    """losses[0, 1] n_valid against -mean(log_probs(xvalid)) in float64 at the weights after the step (evaluator: as check_step)"""
    ev = (rebuilt(oracle) if evaluator is None else evaluator)(w_post)
    want = -float(np.mean(ev.log_probs(xvalid, f64=True)))
    got = float(logged) * xvalid.shape[0]
    assert abs(got - want) < bounds['loss'] * (1 + abs(want)), '%s: validation loss %.9g vs float64 %.9g' % (what, got, want)
    return abs(got - want) / (bounds['loss'] * (1 + abs(want)))
