"""The solo K4 step loops (nnest_amd/csrc/nnest_solo.hip; schedule in solo_schedule.h): exact steps in a loop of their own, the steps
behind them straight through and unrolled by two, and -- in the register forms without history -- x inverted once behind the loop
instead of selected step by step.

The yardstick is the same launch with history=True: mh_kernel_solo<U, true, -1, 4>, the generic likelihood code, the per-step select
of x and a store of every step.  The production Rosenbrock kernel must end on the same bits: z, x, logl, n_accept, n_call, moved,
scale; and the history's last row must be what the history launch itself returns.

Shapes: H 16, B 3, L 1, C = 5 walkers (two workgroups; the second has one live wave and three idle ones); x_dim 50 (U = 2, padded
lanes, a masked last term), 64 (U = 2, nothing padded), 33 (second slot nearly empty), 4 (U = 1), 97 (U = 4: weights in LDS, x still
selected per step).  Steps 1, 2, 3, 17, 18, 19, 20: a lone step, the unroll's odd and even remainders, S <= warm and S = warm + 1 .. + 4
at the default warm-up of 16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
C = 5
DIMS = (50, 64, 33, 4, 97)
STEPS = (1, 2, 3, 17, 18, 19, 20)
RULES = {'fixed': {}, 'batch': dict(dynamic='batch'), 'batch_lag0': dict(dynamic='batch', lag=0), 'batch_warm0': dict(dynamic='batch', warm=0)}
SEED = 21
STEP_SIZE = 0.05


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


def flow_of(hip, D):
    if D not in _flows:
        nvp = hip.HipNVP(D, 16, 3, 1, seed=D)
        init = np.random.RandomState(D).uniform(-0.5, 0.5, size=(C, D))
        z0, _ = nvp.forward(init)
        l0 = hip.loglike(0, init, 5.0)
        _flows[D] = (nvp, z0, l0, float(np.median(cpu(l0))) - 50.0)
    return _flows[D]


def launch(nvp, z0, l0, star, step, S, history, **kw):
    z, l = z0.clone(), l0.clone()
    res = nvp.mh_steps(0, 5.0, z, l, star, step, S, seed=SEED, form='solo', history=history, **kw)
    if kw.get('dynamic'):
        nvp.check_sync(res)
    out = dict(z=cpu(z), logl=cpu(l), x=cpu(res['x']), n_accept=cpu(res['n_accept']), n_call=cpu(res['n_call']),
               moved=cpu(res['moved']), scale=cpu(res['scale']))
    if history:
        out['hist_x'], out['hist_logl'] = cpu(res['hist_x']), cpu(res['hist_logl'])
    return out


def both(hip, D, S, star=None, step=STEP_SIZE, **kw):
    nvp, z0, l0, star0 = flow_of(hip, D)
    assert nvp.mh_form_for(C, form='solo', **{k: v for k, v in kw.items() if k in ('dynamic', 'lag', 'warm')}) == 'solo'
    star = star0 if star is None else star
    prod = launch(nvp, z0, l0, star, step, S, False, **kw)
    hist = launch(nvp, z0, l0, star, step, S, True, **kw)
    return prod, hist


def assert_same_bits(prod, hist):
    for k in ('z', 'x', 'logl', 'n_accept', 'n_call', 'moved', 'scale'):
        a, b = prod[k], hist[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(bits(a), bits(b)), (k, a, b)
    assert np.array_equal(bits(hist['hist_x'][:, -1]), bits(hist['x']))
    assert np.array_equal(bits(hist['hist_logl'][:, -1]), bits(hist['logl']))


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('S', STEPS)
@pytest.mark.parametrize('D', DIMS)
def test_production_kernel_ends_on_the_history_kernels_bits(hip, D, S, rule):
    prod, hist = both(hip, D, S, **RULES[rule])
    n = int(hist['n_accept'].sum())
    print('D %d S %d %s: history launch accepted %d of %d' % (D, S, rule, n, C * S))
    if S >= 17:
        assert 0 < n < C * S   # both arms of every per-step select ran (a condition on the yardstick's own launch)
    assert_same_bits(prod, hist)


@pytest.mark.parametrize('S', (3, 19, 20))
def test_unconstrained_branch(hip, S):
    """loglstar=None: sampler.py:396-410, the float64 ratio that stays out of line"""
    nvp, z0, l0, _ = flow_of(hip, 50)
    prod = launch(nvp, z0, l0, None, STEP_SIZE, S, False)
    hist = launch(nvp, z0, l0, None, STEP_SIZE, S, True)
    n = int(hist['n_accept'].sum())
    print('unconstrained S %d: accepted %d of %d' % (S, n, C * S))
    assert_same_bits(prod, hist)


@pytest.mark.parametrize('D', (50, 4))
def test_nothing_accepted(hip, D):
    """loglstar=+inf: every select takes the old value, x is the chain's first x, nothing moved"""
    S = 19
    prod, hist = both(hip, D, S, star=float('inf'))
    assert_same_bits(prod, hist)
    assert int(prod['n_accept'].sum()) == 0 and not prod['moved'].any()
    assert np.array_equal(bits(prod['x']), bits(hist['hist_x'][:, 0]))


@pytest.mark.parametrize('D', (50, 4))
def test_small_steps_below_no_constraint(hip, D):
    """loglstar=-inf at step_size 1e-3: the likelihood never refuses, nearly every proposal is taken"""
    S = 19
    prod, hist = both(hip, D, S, star=float('-inf'), step=1e-3)
    n = int(hist['n_accept'].sum())
    print('D %d: accepted %d of %d' % (D, n, C * S))
    assert n > 0
    assert_same_bits(prod, hist)
