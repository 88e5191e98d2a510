"""The tail of a solo K4 step -- what runs outside the three coupling blocks (nnest_amd/csrc/nnest_solo.hip, solo_loglike.h): the hand-over
of the new slots, scale * x, the neighbour fetch through the row rotation, the four masked Rosenbrock terms, the two reduction
ladders, the box test, the ratio with its clamp and NaN rule, the `u <` test, `lp > loglstar`, the accept selects, the counters and
the next proposal.  This is the stretch of the step that hipcc schedules and pairs as it sees fit and that build flags and hand-written
bodies are tried on (the terms are paired by class, -fno-slp-vectorize was measured and left out); whatever instructions it ends up as, its
results may not move by a bit.  The cases below were first run on the kernels of round 9, which pass all of them -- the edge cases too.

The yardstick is the one of tests/test_gpu_solo_step_body.py: the same launch with history=True, which runs
mh_kernel_solo<U, true, -1, 4> -- the generic likelihood code with its per-step select of x.  The production Rosenbrock kernel must
end on the same bits in z, x, logl, n_accept, n_call, moved and scale.

Shapes: H 16, B 3, L 1, C = 5 walkers (two workgroups, the second with one live wave), form 'solo'.
* x_dim 50, 51, 52, 53: the last valid term sits in slot 0, 1, 2, 3 of its lane; at 53 its neighbour comes from the next position
  through the rotation.  x_dim 64: nothing padded, the last lane's neighbour wraps to position 0 and must be masked.  x_dim 33: the
  second slot nearly empty.
* steps 1, 2, 3, 19: a lone step, both remainders of the unrolled pair, S = warm + 3 at the default warm-up of 16.
* rules: fixed, batch, batch with lag 0.
Edge cases at x_dim 50 under a fixed step: a proposal scale of 0.5 (most proposals leave the prior box: the box test and the -inf
ratio decide); loglstar above every reachable likelihood (nothing accepted, logl comes back as the input bits) and -1e300 (everything
inside the box that passes `u <` is accepted); like_scale 1e20 with loglstar -1e200 (every term overflows, logl = -1e100 exactly, accepted
and stored); loglstar=None (the unconstrained arm, out of line)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
C = 5
DIMS = (50, 51, 52, 53, 64, 33)
STEPS = (1, 2, 3, 19)
RULES = {'fixed': {}, 'batch': dict(dynamic='batch'), 'batch_lag0': dict(dynamic='batch', lag=0)}
KEYS = ('z', 'x', 'logl', 'n_accept', 'n_call', 'moved', 'scale')
SEED = 21
STEP_SIZE = 0.05
LIKE_SCALE = 5.0


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import flow
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return flow


def cpu(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


_flows = {}


def flow_of(hip, D, like_scale=LIKE_SCALE):
    """one flow, one start and one threshold per (x_dim, like_scale), shared by every case and left unchanged"""
    if (D, like_scale) not in _flows:
        nvp = hip.HipNVP(D, 16, 3, 1, seed=D)
        init = np.random.RandomState(D).uniform(-0.5, 0.5, size=(C, D))
        z0, _ = nvp.forward(init)
        l0 = hip.loglike(0, init, like_scale)
        _flows[(D, like_scale)] = (nvp, z0, l0, float(np.median(cpu(l0))) - 50.0)
    return _flows[(D, like_scale)]


def launch(nvp, z0, l0, star, step, S, history, like_scale=LIKE_SCALE, **kw):
    z, l = z0.clone(), l0.clone()
    res = nvp.mh_steps(0, like_scale, z, l, star, step, S, seed=SEED, form='solo', history=history, **kw)
    if kw.get('dynamic'):
        nvp.check_sync(res)
    out = dict(z=cpu(z), logl=cpu(l), x=cpu(res['x']), n_accept=cpu(res['n_accept']), n_call=cpu(res['n_call']),
               moved=cpu(res['moved']), scale=cpu(res['scale']))
    if history:
        out['hist_x'], out['hist_logl'] = cpu(res['hist_x']), cpu(res['hist_logl'])
    return out


def both(hip, D, S, star='default', step=STEP_SIZE, like_scale=LIKE_SCALE, **kw):
    nvp, z0, l0, star0 = flow_of(hip, D, like_scale)
    free = star is None
    assert nvp.mh_form_for(C, form='solo', free=free, **kw) == 'solo'
    star = star0 if isinstance(star, str) else star
    prod = launch(nvp, z0, l0, star, step, S, False, like_scale, **kw)
    hist = launch(nvp, z0, l0, star, step, S, True, like_scale, **kw)
    return prod, hist, cpu(l0)


def assert_same_bits(prod, hist):
    for k in KEYS:
        a, b = prod[k], hist[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(bits(a), bits(b)), (k, a, b)
    assert np.array_equal(bits(hist['hist_x'][:, -1]), bits(hist['x']))
    assert np.array_equal(bits(hist['hist_logl'][:, -1]), bits(hist['logl']))


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('S', STEPS)
@pytest.mark.parametrize('D', DIMS)
def test_tail_ends_on_the_history_kernels_bits(hip, D, S, rule):
    prod, hist, _ = both(hip, D, S, **RULES[rule])
    n = int(hist['n_accept'].sum())
    print('D %d S %d %s: history launch accepted %d of %d' % (D, S, rule, n, C * S))
    if S == 19:
        assert 0 < n < C * S   # both arms of every select ran (a condition on the yardstick's own launch)
    assert_same_bits(prod, hist)


@pytest.mark.parametrize('S', (3, 19))
def test_box_rejections(hip, S):
    """proposal scale 0.5: most proposals leave the prior box; the box test and the -inf ratio decide"""
    prod, hist, _ = both(hip, 50, S, step=0.5)
    n, calls = int(hist['n_accept'].sum()), int(hist['n_call'].sum())
    print('scale 0.5, S %d: accepted %d of %d, %d likelihood calls' % (S, n, C * S, calls))
    assert calls < C * S   # a proposal outside the box costs no call (a condition on the yardstick's own launch)
    assert_same_bits(prod, hist)


@pytest.mark.parametrize('S', (3, 19))
def test_loglstar_above_every_likelihood(hip, S):
    """Rosenbrock is <= 0 everywhere: under loglstar = 1.0 nothing is accepted and logl comes back as the input bits"""
    prod, hist, l0 = both(hip, 50, S, star=1.0)
    assert_same_bits(prod, hist)
    assert int(prod['n_accept'].sum()) == 0 and not prod['moved'].any()
    assert np.array_equal(bits(prod['logl']), bits(l0))


@pytest.mark.parametrize('S', (3, 19))
def test_loglstar_below_every_likelihood(hip, S):
    """loglstar = -1e300: everything inside the box that passes `u <` is accepted"""
    prod, hist, _ = both(hip, 50, S, star=-1e300)
    n = int(hist['n_accept'].sum())
    print('loglstar -1e300, S %d: accepted %d of %d' % (S, n, C * S))
    assert n > 0
    assert_same_bits(prod, hist)


@pytest.mark.parametrize('S', (3, 19))
def test_overflow_takes_the_substitute(hip, S):
    """like_scale 1e20: every term overflows float32, the sum is not finite and logl = -1e100 exactly; above loglstar = -1e200, so such
    a proposal is accepted and stored"""
    prod, hist, l0 = both(hip, 50, S, star=-1e200, like_scale=1e20)
    n = int(hist['n_accept'].sum())
    print('like_scale 1e20, S %d: accepted %d of %d' % (S, n, C * S))
    assert n > 0
    assert np.all(l0 == -1e100)
    assert_same_bits(prod, hist)
    assert np.array_equal(bits(prod['logl']), bits(np.full(C, -1e100)))
    assert np.array_equal(bits(hist['hist_logl']), bits(np.full((C, S + 1), -1e100)))


@pytest.mark.parametrize('S', (3, 19))
def test_unconstrained_launch(hip, S):
    """loglstar=None: the float64 ratio of likelihood and prior, the arm that stays out of line"""
    prod, hist, _ = both(hip, 50, S, star=None)
    n = int(hist['n_accept'].sum())
    print('unconstrained, S %d: accepted %d of %d' % (S, n, C * S))
    assert_same_bits(prod, hist)
