"""What the CPU and GPU tests of the Metropolis kernels on a regression likelihood of user data share (tests/test_mh_glm_check.py,
tests/test_gpu_mh_glm.py, tests/test_gpu_spline_mh_glm.py): the case tables, a Python restatement of the step, and the checks.  numpy
only: no GPU, no torch device.

mh_glm_kernel<U, FAM> (nnest_mh_glm.hip) and spline_mh_glm_kernel_team<NT, NH, FAM> (nnest_spline_mh_glm.hip) run K4's hard-constraint
step (nnest/sampler.py:229-463; mh_body.h) with logL(x) = GLM(T(x)) (include/nnest_hip.h nnest_mh_glm_steps).  `trace` restates that
step in the shape of mh_checks.spline_mcmc_trace: the flow is any oracle object, the likelihood slice_glm_check.exact_logl on the
float32 T(x), the rule fixed, batch-wide with a lag (the vote of step s applies from step s + 1 + lag on, as oracle.mcmc_sample(lag=)
defines it) or per 16-walker tile.  tests/test_mh_glm_check.py holds it to oracle.mcmc_sample decision for decision.  The restatement
evaluates the likelihood at every proposal; a kernel skips it where `pre` is false: the outputs compared are the ones in which the skip
must not show.

Tolerances (none is new): mh_checks.MARGIN_TOL for a walker that leaves the oracle's chain (`assert_borderline`), slice_like_check's
TOL and LEAVES for the others, its AGREE for the cap, glm_check.bound for the returned logL at the kernel's own x."""
import numpy as np

from tests import glm_check as gk
from tests import mh_checks as mc
from tests import slice_glm_check as sg
from tests import slice_like_check as sl
from tests.fused_like_check import bits_equal

Case, SplineCase = sg.Case, sg.SplineCase
case_id, data_of, affine_of, T32, exact_logl, start, non_finite_data, FAM = (
    sg.case_id, sg.data_of, sg.affine_of, sg.T32, sg.exact_logl, sg.start, sg.non_finite_data, sg.FAM)

# The NVP table: slice_glm_check's shapes -- x_dim 2, 33, 65, 128 (U = 1 .. 4), n = 64, 65, 257, 300 (one pass, ragged last passes, two
# pass groups), both families -- at S = 6 steps (S must exceed lag + 2 at lag 3), and one row with a T that varies by dimension.
# The start keeps 51 walkers: 13 workgroups of four, the last ragged.
S_STEPS = 6
NVP_TABLE = [c._replace(S=S_STEPS) for c in sg.NVP_TABLE]
NVP_EXTRA = [c._replace(S=S_STEPS) for c in sg.NVP_EXTRA]
# The spline table: NT = 1 .. 4 at hidden 16, spline_d8_h32.npz for NH = 2; 19 walkers: two tiles, one ragged
SPLINE_TABLE = [sc._replace(case=sc.case._replace(S=S_STEPS)) for sc in sg.SPLINE_TABLE]
LAGS = (0, 1, 3)
TILE = 16
CAP = 1.0 - sl.AGREE   # the share of a case's walkers that may be excluded from the element-wise comparison


def step_of(D):
    """the proposal scale of the tests: the Sampler's default 2 / sqrt(D) is for a trained flow; a quarter of it keeps about half of the
    proposals of these untrained flows inside the box and above L*, so that pre, !pre, acc and !acc all occur"""
    return 0.5 / np.sqrt(D)


def groups_of(C, rule, tile=TILE):
    """the walkers that vote together: none (fixed), all (batch), or tiles of 16"""
    if rule == 'fixed':
        return []
    if rule == 'batch':
        return [np.arange(C)]
    assert rule == 'tile', rule
    return [np.arange(a, min(a + tile, C)) for a in range(0, C, tile)]


class _Votes(object):
    """sampler.py:422-431 for one adaptation group"""

    def __init__(self, step):
        self.scale, self.up, self.down = float(step), 0, 0

    def vote(self, accepted, total):
        if 2 * accepted > total:
            self.up += 1
        else:
            self.down += 1
        if self.up > self.down:
            self.scale *= np.exp(1. / (1 + self.up))
        if self.up < self.down:
            self.scale /= np.exp(1. / (1 + self.down))


def trace(o, c, z0, l0, star, step, dz, u, rule='fixed', lag=0, evaluate=None, margins=None, fault=None, workgroup=4):
    """Sampler._mcmc_sample, hard-constraint branch, on the oracle flow `o` with recorded noise dz [S, C, D], u [S, C].
    evaluate(x [N, D]) -> logL [N] float64 (None: exact_logl of the case).  margins [S, C] (optional, filled): mh_checks'
    formula -- min of |u - ratio|, the distance of the nearest coordinate of x' from the box edge and, for rows with pre,
    |logL' - L*| / (1 + |L*|).
    fault: None, or one way of being wrong (the CPU suite's stand-in kernels): 'count_all' -- the likelihood evaluated and counted
    at every proposal; 'ncall_acc' -- n_call counts acc; 'box_on_T' -- the box tested on T(x) against +-1; 'early_vote' -- a
    vote applied one step early; 'total_wg' -- the vote's total taken over workgroups of `workgroup` walkers, not walkers.
    Returns x [C, S + 1, D], z [C, D], logl [C, S + 1], n_call [C], n_accept [C], pre / acc [S, C], scale [groups]."""
    from oracle import oracle as orc  # checker only
    ev = (lambda x: exact_logl(c, x)) if evaluate is None else evaluate
    S, C, D = dz.shape
    z = np.asarray(z0, np.float32).copy()
    x, ld = o.inverse(z)
    logl = np.asarray(l0, np.float64).copy()
    hx, hl = [x.copy()], [logl.copy()]
    groups = groups_of(C, rule)
    votes = [_Votes(step) for _ in groups]
    scale = np.full(C, float(step))
    counts = np.zeros((S, max(len(groups), 1)), np.int64)
    n_call, n_acc = np.zeros(C, np.int64), np.zeros(C, np.int64)
    pres, accs = np.zeros((S, C), bool), np.zeros((S, C), bool)
    sd, mu = affine_of(c)
    for it in range(S):
        zp = (z + (dz[it] * scale.astype(np.float32)[:, None]).astype(np.float32)).astype(np.float32)
        xp, ldp = o.inverse(zp)
        log_ratio = (ldp - ld).astype(np.float32)
        if fault == 'box_on_T':   # the box tested on T(x) against +-1, not on x (test_slice_glm_check.py's fault of that name)
            inbox = orc.prior_inbox(T32(c, xp)) == 0
        else:
            inbox = orc.prior_inbox(xp) == 0
        log_ratio[~inbox] = -np.inf
        with np.errstate(over='ignore', invalid='ignore'):
            ratio = np.minimum(np.exp(log_ratio), np.float32(1.0))
        ratio = np.where(np.isnan(log_ratio), np.float32(np.nan), ratio).astype(np.float32)
        pre = u[it] < ratio
        lp = np.asarray(ev(xp), np.float64)
        acc = pre & (lp > star)
        if margins is not None:
            m = np.abs(u[it].astype(np.float64) - ratio.astype(np.float64))
            m = np.minimum(m, np.min(np.abs(np.abs(xp.astype(np.float64)) - 1.0), axis=1))
            m = np.where(pre, np.minimum(m, np.abs(lp - star) / (1.0 + abs(star))), m)
            margins[it] = m
        n_call += np.ones(C, np.int64) if fault == 'count_all' else acc if fault == 'ncall_acc' else pre
        n_acc += acc
        pres[it], accs[it] = pre, acc
        z[acc] = zp[acc]; x[acc] = xp[acc]; ld[acc] = ldp[acc]; logl[acc] = lp[acc]
        for gi, g in enumerate(groups):
            counts[it, gi] = int(acc[g].sum())
            back = lag if rule == 'batch' else 0   # the vote of step s applies from step s + 1 + lag on
            if fault == 'early_vote':
                assert back > 0, 'early_vote: a lag to be early against'
                back -= 1
            if it - back >= 0:
                total = len(g) if fault != 'total_wg' else (len(g) + workgroup - 1) // workgroup
                votes[gi].vote(int(counts[it - back, gi]), total)
                scale[g] = votes[gi].scale
        hx.append(x.copy()); hl.append(logl.copy())
    return dict(x=np.stack(hx, 1), z=z, logl=np.stack(hl, 1), n_call=n_call, n_accept=n_acc, pre=pres, acc=accs,
                scale=np.array([v.scale for v in votes]) if groups else np.array([float(step)]))


def near_share(margins):
    """the share of walkers with any oracle margin below MARGIN_TOL: the walkers on which a correct kernel may differ.  From the oracle
    alone."""
    return float(np.mean(np.min(np.asarray(margins, np.float64), axis=0) < mc.MARGIN_TOL))


def assert_under_cap(margins, what=''):
    near = near_share(margins)
    assert near <= CAP, ('%s: near share %.3g: a TEST-DESIGN failure, not the kernel\'s -- the exclusion could hide a failure on this '
                         'case; lower S or n' % (what, near))
    return near


def as_kernel(r):
    """a `trace` result in the shape `hold` takes from a kernel (the CPU suite's stand-in kernels)"""
    return dict(hist_x=r['x'], hist_logl=r['logl'], x=r['x'][:, -1], z=r['z'], logl=r['logl'][:, -1], n_call=r['n_call'],
                n_accept=r['n_accept'], scale=r['scale'], moved=np.all(r['x'][:, 0] != r['x'][:, -1], axis=1))


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return np.abs(np.asarray(a, np.float64) - b) / (1.0 + np.abs(b))


def check_logl_of_own_x(c, logl_kernel, x_kernel, n_accept, l0, what='', data=None):
    """the logL a kernel returned against glm_check.exact at T of the kernel's own final x in float32, within glm_check.bound.  A
    walker that never moved holds the caller's logl: it must keep its bits.  Returns the worst error / bound."""
    logl, moved = np.asarray(logl_kernel, np.float64), np.asarray(n_accept).reshape(-1) > 0
    assert np.all(bits_equal(logl[~moved], np.asarray(l0, np.float64)[~moved])), '%s: an unmoved walker\'s logl changed' % what
    if not moved.any():
        return 0.0
    d = data_of(c) if data is None else data
    t = T32(c, np.asarray(x_kernel, np.float32)[moved])
    want, b = gk.exact(d, t)[0], gk.bound(d, t)
    r = np.abs(logl[moved] - want) / b
    assert np.all(r <= 1.0), '%s: logL of the kernel\'s own x: %.3g of the bound' % (what, float(np.nanmax(r)))   # (a NaN fails)
    return float(np.max(r))


def hold(c, k, ref, margins, l0, star, rule='fixed', lag=0, what=''):
    """the checks of one kernel output `k` (numpy arrays hist_x, hist_logl, x, z, logl, n_call, n_accept, moved, scale) against the
    restatement's `ref` on the same noise, in order.
    1. The cap, from the oracle alone.
    2. Under a rule one flipped decision may change a vote, and from the step that vote reaches every chain of the group is another
       chain.  The kernel's accepted count of a step is read off its history (a state that changed); per group the chains are
       compared up to the first state a differing vote can have reached (all of them where every vote matched).
    3. Within that horizon a walker that leaves the oracle's chain must do so at a step whose oracle margin is below MARGIN_TOL;
       every other walker agrees in every state within TOL.  A walker whose chain agrees but whose counters differ took a
       borderline decision without consequence (pre flipped, logL' below L* either way): it must have a margin below MARGIN_TOL.
       At most CAP of the walkers may be excluded in either way.
    4. Where every vote matched: counters of the agreeing walkers, final z, the logL history, the final scale.
    5. The returned logL against glm_check.exact at the kernel's own x; x = the last state; the box; L*; NNEST_MH_ALL_MOVED.
    Returns (agree [C] bool, near, worst state error / TOL, worst logL error / bound, every vote matched)."""
    near = assert_under_cap(margins, what)
    hx, rx = np.asarray(k['hist_x'], np.float32), ref['x']
    C, S = hx.shape[0], hx.shape[1] - 1
    assert hx.shape == rx.shape and margins.shape == (S, C), what
    groups = groups_of(C, rule)
    horizon = np.full(C, S + 1)
    moved_k = np.any(hx[:, 1:] != hx[:, :-1], axis=2).T   # [S, C]: the kernel's acc
    full = True
    for g in groups:
        vk, vo = 2 * moved_k[:, g].sum(1) > len(g), 2 * ref['acc'][:, g].sum(1) > len(g)
        d = np.flatnonzero(vk != vo)
        if len(d):
            full = False
            horizon[g] = min(S + 1, int(d[0]) + (lag if rule == 'batch' else 0) + 2)
    agree = np.ones(C, bool)
    worst = 0.0
    for w in range(C):
        H = int(horizon[w])
        err = np.max(_rel(hx[w, :H], rx[w, :H]), axis=1)
        if np.any(err > sl.LEAVES):
            agree[w] = False
            s = int(np.argmax(err > sl.LEAVES))
            assert s >= 1, '%s: walker %d starts away from the oracle' % (what, w)
            assert margins[s - 1, w] < mc.MARGIN_TOL, ('%s: walker %d leaves the oracle chain at step %d where the oracle\'s decision margin '
                                                       'is %.3g (not a rounding-borderline decision)' % (what, w, s, margins[s - 1, w]))
            continue
        assert np.all(err < sl.TOL), '%s: walker %d: states %.3g' % (what, w, float(np.max(err)))   # (a NaN fails)
        worst = max(worst, float(np.max(err)))
        if H == S + 1 and (int(k['n_call'][w]) != int(ref['n_call'][w]) or int(k['n_accept'][w]) != int(ref['n_accept'][w])):
            agree[w] = False
            assert np.min(margins[:, w]) < mc.MARGIN_TOL, ('%s: walker %d keeps the oracle\'s chain with other counters (n_call %d / %d, n_accept '
                                                           '%d / %d) and no borderline decision' % (what, w, k['n_call'][w], ref['n_call'][w],
                                                                                                   k['n_accept'][w], ref['n_accept'][w]))
    assert 1.0 - agree.mean() <= CAP, '%s: %.3g of the walkers excluded' % (what, 1.0 - agree.mean())
    if full:
        whole = agree & (horizon == S + 1)
        ez = float(np.max(_rel(np.asarray(k['z'])[whole], ref['z'][whole])))
        assert ez < sl.TOL, '%s: final z of agreeing walkers: %.3g' % (what, ez)
        el = float(np.max(_rel(np.asarray(k['hist_logl'])[whole], ref['logl'][whole])))
        assert el < sl.TOL, '%s: logL history of agreeing walkers: %.3g' % (what, el)
        if full:   # (every vote matched: the scale is the oracle's)
            ks = np.asarray(k['scale'], np.float64)
            want = ref['scale'] if rule == 'tile' else np.full(len(ks), ref['scale'][0])
            assert ks.shape == want.shape and np.all(np.abs(ks - want) <= 1e-5 * want), '%s: scale %r, the oracle\'s %r' % (what, ks, want)
    r_ll = check_logl_of_own_x(c, k['logl'], k['x'], k['n_accept'], l0, what=what)
    assert np.all(bits_equal(np.asarray(k['x'], np.float32), hx[:, -1])), what
    assert np.all(bits_equal(np.asarray(k['logl'], np.float64), np.asarray(k['hist_logl'], np.float64)[:, -1])), what
    assert np.all(np.abs(hx) <= 1.0), '%s: a state outside the box' % what
    assert np.all(np.asarray(k['logl'])[np.asarray(k['n_accept']) > 0] > star), '%s: an accepted logl not above L*' % what
    assert np.all(np.asarray(k['n_call']) >= np.asarray(k['n_accept'])) and np.all(np.asarray(k['n_call']) <= S), what
    assert np.array_equal(np.asarray(k['n_accept']), moved_k.sum(0)), '%s: n_accept against the states that changed' % what
    assert np.array_equal(np.asarray(k['moved'], bool), np.all(hx[:, 0] != hx[:, -1], axis=1)), '%s: NNEST_MH_ALL_MOVED' % what
    return agree, near, worst / sl.TOL, r_ll, full


def check_nothing_moves(k, ref, margins, z0, l0, what=''):
    """the safe rule under a likelihood that is non-finite everywhere: a non-finite logL counts as -1e100 and fails logL > L*.  Nothing
    is accepted; z, every state and logl keep their bits; n_call still counts pre: the oracle's on every walker it decided firmly"""
    hx = np.asarray(k['hist_x'], np.float32)
    assert int(np.sum(k['n_accept'])) == 0 and not np.any(k['moved']), what
    assert np.all(bits_equal(hx, np.repeat(hx[:, :1], hx.shape[1], axis=1))), what
    assert np.all(bits_equal(np.asarray(k['z'], np.float32), np.asarray(z0, np.float32))), what
    assert np.all(bits_equal(np.asarray(k['logl'], np.float64), np.asarray(l0, np.float64))), what
    assert np.all(bits_equal(np.asarray(k['hist_logl'], np.float64), np.repeat(np.asarray(l0, np.float64)[:, None], hx.shape[1], axis=1))), what
    assert ref['n_accept'].sum() == 0 and ref['n_call'].sum() > 0, what
    firm = np.min(margins, axis=0) >= mc.MARGIN_TOL
    assert firm.mean() >= sl.AGREE, what
    np.testing.assert_array_equal(np.asarray(k['n_call'])[firm], ref['n_call'][firm], err_msg='%s: n_call still counts pre' % what)
