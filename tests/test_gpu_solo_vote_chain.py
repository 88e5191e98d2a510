"""The chain of an exact step's vote in the solo K4 kernel (nnest_amd/csrc/nnest_solo.hip): while a vote
travels the relay wave works out the scales that vote AND the next can lead to, and behind the vote only selects -- the scale, and the
two candidates of the next step.  Whatever moves around the barriers of an exact step (round 11 also tried the net waves' accept flag
in front of barrier A and earlier counter reads; neither was kept), the results may not move by a bit.

The yardstick is the one of tests/test_gpu_solo_tail.py: the same launch with history=True, which runs mh_kernel_solo<U, true, -1, 4>
(the generic likelihood code with its per-step select of x; the same relay).  The production Rosenbrock kernel must end on the same
bits in z, x, logl, n_accept, n_call, moved and scale.  Both kernels carry the reordered chain, so what holds them to the rule itself
is the step-rule oracle of tests/test_gpu_solo.py; here every shape at which the reordering can go wrong is run once.

Shapes: x_dim 50, Rosenbrock, H 16, B 3, L 1, form 'solo'.
* walkers 1, 4, 5, 33: one tile with one live wave, a full tile, a partial last tile, more tiles (9) than counter shards (8).
* steps 2, 3, 17, 18, 19 at the default warm-up of 16: warm = 1 (one vote: only the outcomes worked out in front of the loop are used),
  warm = 2 (the first looked-ahead pair), and the close of the warm-up with one / two / three steps behind 16 exact ones.
* rules: the default rule (16 exact steps, then lag 8) and lag 0 (every step exact; the last step's vote goes to scale_out, so steps = 2
  runs it directly behind the first).
* per rule one launch with loglstar above every likelihood (every vote down) and one with loglstar below every likelihood and a tiny
  step (every vote up): both precomputed outcomes are selected, at every exact step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D = 50
WALKERS = (1, 4, 5, 33)
STEPS = (2, 3, 17, 18, 19)
RULES = {'default': dict(dynamic='batch'), 'lag0': dict(dynamic='batch', lag=0)}
KEYS = ('z', 'x', 'logl', 'n_accept', 'n_call', 'moved', 'scale')
SEED = 23
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


_state = {}


def start_of(hip, C):
    """one flow for all cases; one start and one threshold per population, shared by every case and left unchanged"""
    if 'nvp' not in _state:
        _state['nvp'] = hip.HipNVP(D, 16, 3, 1, seed=D)
    if C not in _state:
        init = np.random.RandomState(100 + C).uniform(-0.5, 0.5, size=(C, D))
        z0, _ = _state['nvp'].forward(init)
        l0 = hip.loglike(0, init, LIKE_SCALE)
        _state[C] = (z0, l0, float(np.median(cpu(l0))) - 50.0)
    return (_state['nvp'],) + _state[C]


def launch(nvp, z0, l0, star, step, S, history, **kw):
    z, l = z0.clone(), l0.clone()
    res = nvp.mh_steps(0, LIKE_SCALE, z, l, star, step, S, seed=SEED, form='solo', history=history, **kw)
    nvp.check_sync(res)
    return dict(z=cpu(z), logl=cpu(l), x=cpu(res['x']), n_accept=cpu(res['n_accept']), n_call=cpu(res['n_call']),
                moved=cpu(res['moved']), scale=cpu(res['scale']))


def both(hip, C, S, star='default', step=STEP_SIZE, **kw):
    nvp, z0, l0, star0 = start_of(hip, C)
    assert nvp.mh_form_for(C, form='solo', **kw) == 'solo'
    star = star0 if isinstance(star, str) else star
    prod = launch(nvp, z0, l0, star, step, S, False, **kw)
    hist = launch(nvp, z0, l0, star, step, S, True, **kw)
    return prod, hist, cpu(l0)


def assert_same_bits(prod, hist):
    for k in KEYS:
        a, b = prod[k], hist[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(bits(a), bits(b)), (k, a, b)


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('S', STEPS)
@pytest.mark.parametrize('C', WALKERS)
def test_vote_chain_ends_on_the_history_kernels_bits(hip, C, S, rule):
    prod, hist, _ = both(hip, C, S, **RULES[rule])
    print('C %d S %d %s: history launch accepted %d of %d, scale %r' % (C, S, rule, int(hist['n_accept'].sum()), C * S, float(hist['scale'][0])))
    assert_same_bits(prod, hist)


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('C', (5, 33))
def test_every_vote_down(hip, C, rule):
    """Rosenbrock is <= 0 everywhere: under loglstar = 1.0 nothing is accepted, every vote of the rule is down and the scale only falls"""
    prod, hist, l0 = both(hip, C, 19, star=1.0, **RULES[rule])
    assert int(hist['n_accept'].sum()) == 0 and float(hist['scale'][0]) < STEP_SIZE   # (conditions on the yardstick's own launch)
    assert_same_bits(prod, hist)
    assert np.array_equal(bits(prod['logl']), bits(l0))


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('C', (5, 33))
def test_every_vote_up(hip, C, rule):
    """loglstar = -1e300 and a step of 1e-5: nearly every proposal stays in the box and passes `u <`, every vote is up and the scale
    only grows (by at most exp(sum 1 / (1 + k)) ~ 11 over 19 steps: it stays tiny)"""
    prod, hist, _ = both(hip, C, 19, star=-1e300, step=1e-5, **RULES[rule])
    n = int(hist['n_accept'].sum())
    print('C %d %s: accepted %d of %d, scale %r' % (C, rule, n, C * 19, float(hist['scale'][0])))
    assert 2 * n > C * 19 and float(hist['scale'][0]) > 1e-5   # (conditions on the yardstick's own launch)
    assert_same_bits(prod, hist)
