"""What the CPU and GPU tests of the slice kernels with EVERY fused likelihood share (tests/test_slice_like_check.py,
tests/test_gpu_slice_likes.py): the case tables, the start, and the checks.  numpy only: no GPU, no torch device.

The slice proposal runs in three kernel families -- slice_kernel_solo<U, LK> (nnest_solo.hip), the wave, team and pair forms of
nnest_spline_slice.hip <NT, NH>, and nnest_slice_rounds.hip with the device likelihood -- and each is held to
oracle.slice_sample(..., like_params=...) on the kernel's own directions and the shared Philox uniforms.

Names, ids and parameters are tests/fused_like_check.LIKES'; the slice entries take a scalar like_scale and the unit box, so the
scales are this file's (SCALES).  Tolerances (none is new): counters and states as tests/test_gpu_slice.py holds them -- 2e-4 (1 + |v|)
on every state of a walker whose counters agree, an oracle margin below 2e-4 where a walker leaves, at least 80 % of walkers in
agreement; the logL a kernel returns against the float64 likelihood of like_scale times the kernel's own x in float32, within
fused_like_check.logl_bound.  The chain's logL is NOT compared with the oracle chain's logL: at shell width 0.1 that comparison
inherits the flow's conditioning (about 40 times the error in x) and says nothing about the evaluator."""
import collections

import numpy as np

from tests import fused_like_check as fl

TOL = 2e-4          # tests/test_gpu_slice.py: states of agreeing walkers, relative to 1 + |v|; the oracle margin of a leaving walker
LEAVES = 1e-3       # tests/test_gpu_slice.py: a state further than this from the oracle's is where a walker has left
AGREE = 0.8         # tests/test_gpu_slice.py: the share of walkers whose counters must agree
DRAWS, QUANTILE, UPDATES = 64, 0.2, 4

# like_scale by likelihood; the shells: 2.5 where the box is narrow against the shell (x_dim 5, and 6 in the rounds table), 1.0 at
# x_dim 40 and 97, where |x| ~ 0.35 sqrt(x_dim) reaches the shell's radius by itself
SCALES = {'rosenbrock': 5.0, 'gaussmix': 10.0, 'himmelblau': 5.0, 'gaussian': 5.0, 'eggbox': 15.0}


def like_scale(name, D):
    if name in ('shell', 'double_shell'):
        return 2.5 if D <= 6 else 1.0
    return SCALES[name]


Case = collections.namedtuple('Case', 'name params scale D S')


def case(name, D, S=UPDATES):
    e = fl.LIKES[name]
    assert e['dims'](D), (name, D)
    return Case(name, tuple(e['params']), like_scale(name, D), D, S)


def lk(name):
    """LK of slice_kernel_solo<U, LK>: 0 for Rosenbrock, -1 (the id read at run time) for every other likelihood"""
    return 0 if name == 'rosenbrock' else -1


# the solo kernel: Rosenbrock at U = 3 (x_dim 65 .. 96: both edges and the middle) and U = 4 (x_dim 128, the full-tile wrap); the other
# six at one or two widths each, together U = 1 .. 4 of the generic instantiation.  S = 4 updates, but S = 3 for double_shell at
# x_dim 97, which sits at the edge of the cap condition: with S = 4 its near_share over three direction seeds on a random flow
# (tests/test_slice_like_check.py) was 0.14, 0.16, 0.16 against the cap's 0.2 (with S = 3: 0.10, 0.10, 0.16); every other row stayed at
# or below 0.14, typically 0.02 to 0.06
SOLO_TABLE = ([case('rosenbrock', D) for D in (65, 80, 96, 128)] + [case('gaussmix', D) for D in (20, 81)]
              + [case('himmelblau', D) for D in (2, 66)] + [case('gaussian', D) for D in (7, 100)] + [case('eggbox', 2)]
              + [case('shell', D) for D in (5, 40)] + [case('double_shell', 5), case('double_shell', 97, S=3)])

# beside the table: Rosenbrock at U = 1 and U = 2, so that the GPU run of the table prints all eight <U, LK> in one place
SOLO_EXTRA = [case('rosenbrock', 5), case('rosenbrock', 33)]

# the safe rule: shell with a NaN width -- check_like admits it, every candidate's logL is non-finite -- at U = 1 and U = 3
NAN_PARAMS = (float('nan'), 2.0, 0.0)
SAFE_SOLO_DIMS = (5, 70)


def case_id(c):
    return '%s-d%d' % (c.name, c.D)


def oracle_loglike(c, x_unit, params=None):
    """the oracle's likelihood of unit-box rows (the start's logL; oracle.slice_sample evaluates the same function)"""
    from oracle import oracle as orc
    p = c.params if params is None else params
    return orc.loglike(c.name, x_unit, c.scale, list(p) if p else None)


def start(c, forward, seed=0, count=None):
    """the existing recipe (tests/test_gpu_slice.py setup): 64 points from uniform(-0.6, 0.6), L* the 20 % quantile of their logL, the
    rows above it through the flow's `forward` (x [n, D] float64 -> z [n, D] float32 numpy).  The kept count (51 of 64 without ties) is
    no multiple of 4: the last workgroup of the solo kernel, four walkers each, is ragged.  count: keep the first `count` of them only
    (the spline and rounds cases, whose oracle is slow; ragged against 8 and 16).  Returns z0, l0, star."""
    u0 = np.random.RandomState(seed).uniform(-0.6, 0.6, size=(DRAWS, c.D))
    l0 = np.asarray(oracle_loglike(c, u0), np.float64)
    assert np.all(np.isfinite(l0)), c
    star = float(np.quantile(l0, QUANTILE))
    keep = np.flatnonzero(l0 > star)
    assert len(keep) % 4 != 0 and len(keep) >= 0.75 * DRAWS, (c, len(keep))
    if count is not None:
        assert count <= len(keep) and count % 8 != 0, (c, count)
        keep = keep[:count]
    z0 = np.ascontiguousarray(forward(u0[keep]), np.float32)
    assert z0.shape == (len(keep), c.D)
    return z0.copy(), l0[keep].copy(), star


def near_share(margins):
    """the share of walkers whose oracle margin fell below 2e-4 at any update.  A correct kernel can only disagree with the oracle on
    those walkers, so near_share <= 1 - AGREE is the condition under which the 80 % cap cannot fail a correct kernel.  From the oracle
    alone: margins [S, C] as oracle.slice_sample fills it."""
    m = np.asarray(margins, np.float64)
    return float(np.mean(np.min(m, axis=0) < TOL))


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return np.abs(np.asarray(a, np.float64) - b) / (1.0 + np.abs(b))


def compare(kernel, oracle, margins, what=''):
    """the block tests/test_gpu_slice.py, tests/test_gpu_spline_slice.py and tests/test_gpu_slice_rounds.py each spell out.
    kernel: numpy arrays hist_x [C, S + 1, D], n_eval, n_call, n_move [C] and, where the entry returns it, the final z [C, D];
    oracle: what oracle.slice_sample returned; margins [S, C]: what it filled.
    A walker's counters agree only if its n_eval, n_call and n_move all match the oracle's.  Walkers whose counters agree must agree in
    every state of hist_x (and in final z) within 2e-4 (1 + |v|); a walker whose counters differ must have had an oracle margin below
    2e-4 at the update where it leaves; at least 80 % of walkers must agree.  Returns (same [C] bool, worst error / 2e-4)."""
    hx = np.asarray(kernel['hist_x'], np.float32)
    C, S = hx.shape[0], hx.shape[1] - 1
    assert hx.shape == oracle['x'].shape and margins.shape == (S, C), what
    same = np.ones(C, bool)
    for k in ('n_eval', 'n_call', 'n_move'):
        same &= np.asarray(kernel[k]).reshape(C).astype(np.int64) == np.asarray(oracle[k]).astype(np.int64)
    assert same.mean() >= AGREE, '%s: only %.3g of the walkers agree with the oracle on every counter' % (what, same.mean())
    err = float(np.max(_rel(hx[same], oracle['x'][same])))
    assert err < TOL, '%s: states of agreeing walkers: %.3g' % (what, err)   # (a NaN fails)
    if kernel.get('z') is not None:
        ez = float(np.max(_rel(np.asarray(kernel['z'])[same], oracle['z'][same])))
        assert ez < TOL, '%s: final z of agreeing walkers: %.3g' % (what, ez)
        err = max(err, ez)
    for c in np.flatnonzero(~same):   # a walker that took another decision: where it leaves, the oracle was within rounding of a threshold
        d = np.max(_rel(hx[c], oracle['x'][c]), axis=1) > LEAVES
        s_first = int(np.argmax(d)) if d.any() else S
        lo = max(s_first - 1, 0)
        assert np.min(margins[lo:min(s_first + 1, S), c]) < TOL, '%s: walker %d leaves at state %d with margins %r' % (
            what, c, s_first, margins[:, c])
    return same, err / TOL


def check_logl_of_own_x(c, logl_kernel, x_kernel, n_move, l0, what=''):
    """the logL a kernel returned against fused_like_check.exact_logl (float64) at like_scale times the kernel's own final x in
    float32, within fused_like_check.logl_bound.  A walker that never moved holds the caller's logl, not the kernel's: it must keep
    its bits.  Returns the worst error / bound."""
    logl, moved = np.asarray(logl_kernel, np.float64), np.asarray(n_move).reshape(-1) > 0
    assert np.all(fl.bits_equal(logl[~moved], np.asarray(l0, np.float64)[~moved])), '%s: an unmoved walker\'s logl changed' % what
    assert moved.mean() > 0.9, '%s: only %.3g of the walkers moved' % (what, moved.mean())
    return fl.check_logl_of_own_x(logl[moved], np.asarray(x_kernel, np.float32)[moved], np.float32(c.scale), np.float32(0.0), c.name,
                                  c.params, what=what)


def check_in_box_above_star(kernel, logl, star, what=''):
    """every state inside the box, every final logl above L*, n_eval >= n_call >= n_move"""
    assert np.all(np.abs(np.asarray(kernel['hist_x'])) <= 1.0), '%s: a state outside the box' % what
    assert np.all(np.asarray(logl) > star), '%s: a final logl not above L*' % what
    ne, nc, nm = (np.asarray(kernel[k]).astype(np.int64) for k in ('n_eval', 'n_call', 'n_move'))
    assert np.all(ne >= nc) and np.all(nc >= nm) and np.all(nm >= 0), '%s: counters out of order' % what


def check_nothing_moves(kernel, oracle, z0, l0, z, logl, what=''):
    """the safe rule under a likelihood that is non-finite everywhere: a non-finite logL counts as -1e100, so no candidate is above
    L*, no update moves, z, every state and logl keep their bits, n_move is 0, and n_call and n_eval are the oracle's (whose
    likelihood applies the same rule)"""
    assert np.all(np.asarray(oracle['n_move']) == 0) and np.all(np.asarray(oracle['n_eval']) > 0), what   # (the case is what it says)
    assert np.all(np.asarray(kernel['n_move']) == 0), '%s: %d walkers moved' % (what, int((np.asarray(kernel['n_move']) != 0).sum()))
    assert np.all(fl.bits_equal(np.asarray(z, np.float32), np.asarray(z0, np.float32))), '%s: z changed' % what
    assert np.all(fl.bits_equal(np.asarray(logl, np.float64), np.asarray(l0, np.float64))), '%s: logl changed' % what
    hx = np.asarray(kernel['hist_x'], np.float32)
    assert np.all(fl.bits_equal(hx, np.repeat(hx[:, :1], hx.shape[1], axis=1))), '%s: a state changed' % what
    if kernel.get('x') is not None:
        assert np.all(fl.bits_equal(np.asarray(kernel['x'], np.float32), hx[:, 0])), '%s: x is not the start' % what
    np.testing.assert_array_equal(np.asarray(kernel['n_call']).astype(np.int64), oracle['n_call'], err_msg=what)
    np.testing.assert_array_equal(np.asarray(kernel['n_eval']).astype(np.int64), oracle['n_eval'], err_msg=what)


def as_kernel(oracle_result):
    """an oracle.slice_sample result in the shape `compare` takes from a kernel (the CPU suite's stand-in kernels)"""
    r = oracle_result
    return dict(hist_x=r['x'], x=r['x'][:, -1], z=r['z'], n_eval=r['n_eval'], n_call=r['n_call'], n_move=r['n_move'])
