"""What the CPU and GPU tests of the slice kernels on a regression likelihood of user data share (tests/test_slice_glm_check.py,
tests/test_gpu_slice_glm.py, tests/test_gpu_spline_slice_glm.py): the case tables, the oracle's likelihood, the start and the checks.
numpy only: no GPU, no torch device.

slice_glm_kernel<U, FAM> (nnest_slice_glm.hip), spline_slice_glm_kernel_team<NT, NH, FAM> (nnest_spline_slice_glm.hip) and
slice_rounds(like_glm=...) run nnest_slice_steps's update with logL(x) = GLM(T(x)) (include/nnest_hip.h nnest_slice_glm_steps).  Each is
held to oracle.slice_sample -- the bracket rule, the uniforms and the margins every slice test already trusts -- with the oracle's
likelihood replaced, for the duration of the call, by tests/glm_check.exact on T(x) computed in float32 (two roundings), float64 with
the safe rule (`oracle_likelihood`).  The oracle evaluates that likelihood at every candidate; a kernel skips it where no decision
depends on it: the outputs compared here are the ones in which the skip must not show.

Tolerances (none is new): slice_like_check's TOL, LEAVES and AGREE through its `compare`, `check_in_box_above_star`,
`check_nothing_moves` and `near_share`; the logL a kernel returns against glm_check.exact at the kernel's own final x within
glm_check.bound."""
import collections
import contextlib

import numpy as np

from tests import glm_check as gk
from tests import slice_like_check as sl
from tests.fused_like_check import bits_equal, units

# family, x_dim, data rows, scale s (T(x) = s x, or with `affine` the per-dimension std and mean of `affine_of`), updates
Case = collections.namedtuple('Case', 'family D n scale S affine')

# The NVP table.  n: 257 = two groups of four passes, the second ragged (GLM_PASSES = 4 passes of 64 rows); 64 = exactly one pass;
# 65 and 300 = ragged last passes.  The near share of each row was measured from the oracle alone on orc.NVP(D, 16, 3, 1) with weights
# N(0, 0.15^2) and direction seeds 100 .. 105: <= 0.04, 0.12, 0.14 (at S = 4), 0.14 and 0.16 (at S = 3), against the cap 1 - AGREE =
# 0.2.  Large n with the logistic family at large x_dim goes over the cap ((128, 300) at S = 4 reached 0.22) and is not here.
NVP_TABLE = [Case('logistic', 2, 257, 5.0, 4, False), Case('poisson', 33, 257, 3.0, 4, False), Case('logistic', 65, 64, 5.0, 3, False),
             Case('logistic', 128, 65, 5.0, 3, False), Case('poisson', 128, 300, 3.0, 2, False)]
# beside it: a T with a std that varies by dimension and a mean that is not zero (the table's T is s x: a kernel that dropped t_mean, or
# read t_std at another dimension's index, would pass the table)
NVP_EXTRA = [Case('poisson', 7, 65, 3.0, 4, True)]

# The spline table: (case, hidden, walkers, golden file or None = the seeded default initialisation with ActNorm completed).
# x_dim 2, 33, 70, 100 at hidden 16: NT = 1 .. 4; tests/golden/spline_d8_h32.npz: NH = 2; 19 walkers: ragged against 16, two tiles.
# S = 3 at x_dim <= 33, 2 above.  The near share needs the handle's weights: the GPU test computes it from the oracle first.
SplineCase = collections.namedtuple('SplineCase', 'case H C golden')
SPLINE_TABLE = [SplineCase(Case('logistic', 2, 257, 5.0, 3, False), 16, 19, None), SplineCase(Case('poisson', 33, 65, 3.0, 3, False), 16, 19, None),
                SplineCase(Case('logistic', 70, 65, 5.0, 2, False), 16, 19, None), SplineCase(Case('poisson', 100, 257, 3.0, 2, False), 16, 19, None),
                SplineCase(Case('logistic', 8, 65, 5.0, 3, True), 32, 19, 'spline_d8_h32.npz')]

FAM = {'logistic': 0, 'poisson': 1}


def case_id(c):
    return '%s-d%d-n%d%s' % (c.family, c.D, c.n, '-affine' if c.affine else '')


def spline_key(sc):
    """(NT, NH) of spline_slice_glm_kernel_team<NT, NH, FAM>"""
    return units(sc.case.D), sc.H // 16


_DATA = {}


def data_of(c):
    """the descriptor (likelihoods.GLMData.hip_like_glm) of glm_check.make_like(D, n, family, seed=7 + D); made once, never changed"""
    key = (c.family, c.D, c.n)
    if key not in _DATA:
        _DATA[key] = gk.make_like(c.D, c.n, c.family, seed=7 + c.D).hip_like_glm
    return _DATA[key]


def affine_of(c):
    """(t_std [D], t_mean [D]) in float32: s and 0, or with `affine` a std within 10 % of s that varies by dimension and a mean of
    +-0.1"""
    d = np.arange(c.D)
    if not c.affine:
        return np.full(c.D, c.scale, np.float32), np.zeros(c.D, np.float32)
    return (c.scale * (1.0 + 0.1 * ((d % 3) - 1))).astype(np.float32), (0.2 * ((d % 2) - 0.5)).astype(np.float32)


def T32(c, x):
    """T(x) = x t_std + t_mean in float32, two roundings (ens_T; s x + 0 is s x)"""
    sd, mu = affine_of(c)
    return (np.asarray(x, np.float32) * sd).astype(np.float32) + mu


def exact_logl(c, x, data=None):
    """float64 with the safe rule, from the float32 T(x)"""
    return gk.exact(data_of(c) if data is None else data, T32(c, x))[0]


@contextlib.contextmanager
def oracle_likelihood(evaluate):
    """oracle.oracle.loglike replaced by evaluate(x [N, D] unit-box rows) -> logL [N] float64 for the duration of an
    oracle.slice_sample call (its name, scale and parameter arguments are not read)"""
    from oracle import oracle as orc
    real = orc.loglike
    orc.loglike = lambda name, x, scale=1.0, params=None: np.asarray(evaluate(np.asarray(x)), np.float64)
    try:
        yield
    finally:
        orc.loglike = real


def slice_sample(o, c, z0, l0, star, dz, seed, walker_offset, evaluate=None, margins=None):
    """oracle.slice_sample of the case on the oracle flow `o`, with the likelihood `evaluate` (None: exact_logl of the case)"""
    from oracle import oracle as orc
    ev = (lambda x: exact_logl(c, x)) if evaluate is None else evaluate
    with oracle_likelihood(ev):
        return orc.slice_sample(o, 'glm', 1.0, z0, l0, star, width_of(c.D), dz, seed, walker_offset=walker_offset, margins=margins)


def width_of(D):
    return 2.0 / np.sqrt(D)


def start(c, forward, seed=0, count=None, data=None):
    """slice_like_check.start's recipe on this likelihood: 64 points from uniform(-0.6, 0.6), L* the 20 % quantile of their logL, the
    rows above it through the flow's `forward`; the kept count (51 of 64 without ties) is no multiple of 4.  count: keep the first
    `count` of them only (ragged against 8 and 16).  Returns z0, l0, star."""
    u0 = np.random.RandomState(seed).uniform(-0.6, 0.6, size=(sl.DRAWS, c.D))
    l0 = np.asarray(exact_logl(c, u0, data), np.float64)
    assert np.all(np.isfinite(l0)) and np.all(l0 != gk.SAFE), c
    star = float(np.quantile(l0, sl.QUANTILE))
    keep = np.flatnonzero(l0 > star)
    assert len(keep) % 4 != 0 and len(keep) >= 0.75 * sl.DRAWS, (c, len(keep))
    if count is not None:
        assert count <= len(keep) and count % 8 != 0, (c, count)
        keep = keep[:count]
    z0 = np.ascontiguousarray(forward(u0[keep]), np.float32)
    assert z0.shape == (len(keep), c.D)
    return z0.copy(), l0[keep].copy(), star


def non_finite_data(c):
    """the case's descriptor with NaN offsets: a descriptor the library takes (it refuses a non-finite logl0 at the entry; the arrays'
    contents are the caller's) under which every candidate's eta, and with it its logL, is non-finite"""
    d = dict(data_of(c))
    d['o'] = np.full_like(d['o'], np.nan)
    return d


def check_logl_of_own_x(c, logl_kernel, x_kernel, n_move, l0, what='', data=None):
    """the logL a kernel returned against glm_check.exact at T of the kernel's own final x in float32, within glm_check.bound.  A
    walker that never moved holds the caller's logl: it must keep its bits.  Returns the worst error / bound."""
    logl, moved = np.asarray(logl_kernel, np.float64), np.asarray(n_move).reshape(-1) > 0
    assert np.all(bits_equal(logl[~moved], np.asarray(l0, np.float64)[~moved])), '%s: an unmoved walker\'s logl changed' % what
    assert moved.mean() > 0.9, '%s: only %.3g of the walkers moved' % (what, moved.mean())
    d = data_of(c) if data is None else data
    t = T32(c, np.asarray(x_kernel, np.float32)[moved])
    want, b = gk.exact(d, t)[0], gk.bound(d, t)
    r = np.abs(logl[moved] - want) / b
    assert np.all(r <= 1.0), '%s: logL of the kernel\'s own x: %.3g of the bound' % (what, float(np.nanmax(r)))   # (a NaN fails)
    return float(np.max(r))


def hold(c, k, logl, ref, margins, l0, star, what=''):
    """the checks of one kernel output, in order; the near share first, from the oracle alone.  k: numpy arrays hist_x, x, z, n_eval,
    n_call, n_move.  Returns (same, near, worst state error / TOL, worst logL error / bound)"""
    near = sl.near_share(margins)
    assert near <= 1.0 - sl.AGREE, ('%s: near share %.3g: a TEST-DESIGN failure, not the kernel\'s -- the 80 %% criterion could fail a '
                                    'correct kernel on this case; lower S' % (what, near))
    same, r_x = sl.compare(k, ref, margins, what=what)
    r_ll = check_logl_of_own_x(c, logl, k['x'], k['n_move'], l0, what=what)
    assert np.all(bits_equal(np.asarray(k['x'], np.float32), np.asarray(k['hist_x'], np.float32)[:, -1])), what
    sl.check_in_box_above_star(k, logl, star, what=what)
    return same, near, r_x, r_ll
