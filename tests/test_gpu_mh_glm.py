"""[UNPINNED] The Metropolis proposal on a regression likelihood of user data, NVP side (include/nnest_hip.h nnest_mh_glm_steps;
nnest_mh_glm.hip mh_glm_kernel<U, FAM>; HipNVP.mh_steps(like_glm=...)).  The step is the reference's hard-constraint step
(nnest/sampler.py:229-463); the likelihood, T and the Philox draws are build-defined.  The cases, the restatement of the step and the
checks are tests/mh_glm_check.py's; tests/test_mh_glm_check.py shows on the CPU that they fail a wrong kernel.

Every table row under the fixed step and the batch rule at lag 0, 1 and 3: the kernel against the restatement on the kernel's own
draws (fill_slice_noise's normals, oracle.slice_uniform's uniforms) -- the cap first, from the oracle alone, then chains, counters,
scale, the returned logL against glm_check.exact at the kernel's own x, the box, L*, NNEST_MH_ALL_MOVED, the sync error word; the
recorded-noise launch and the same launch again bit for bit, and under the fixed step the two halves of the population launched
separately.  Then the safe rule, the skipped likelihood (from L* = -1e300 and from the table's L*: the counters are the
restatement's, which skips nothing) and the refusals.  No launch is sent that the _check entry refuses.  Run with  pytest -m gpu."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc   # (checker only)
from tests import glm_check as gk
from tests import mh_checks as mc
from tests import mh_glm_check as mg
from tests import slice_like_check as sl
from tests.fused_like_check import units

pytestmark = pytest.mark.gpu

SEED, OFF = 4242, 100
E_ARG = 1   # (include/nnest_hip.h NNEST_E_ARG)
CASES = mg.NVP_TABLE + mg.NVP_EXTRA
RULES = [('fixed', 0)] + [('batch', lag) for lag in mg.LAGS]
KEYS = ('hist_x', 'hist_logl', 'x', 'n_call', 'n_accept', 'moved', 'scale')
DYNAMIC = {'fixed': False, 'batch': 'batch', 'tile': 'group'}


def cpu(t):
    return t.detach().cpu().numpy()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fused(net, c, z0, l0, star, rule='fixed', lag=0, data=None, noise=None, walker_offset=OFF, identity=False, wide=1.0):
    """one mh_steps(like_glm=...) launch from (z0, l0), asked of the _check entry first: what it returned as numpy arrays (z, logl:
    the final ones, updated in place)"""
    assert net.mh_glm_refusal(c.D, len(l0), DYNAMIC[rule], lag) is None
    z, logl = cuda(z0), cuda(l0)
    sd, mu = (None, None) if identity else mg.affine_of(c)
    res = net.mh_steps(None, 1.0, z, logl, star, wide * mg.step_of(c.D), c.S, dynamic=DYNAMIC[rule], lag=lag, seed=SEED, walker_offset=walker_offset,
                       history=True, noise=noise, like_glm=mg.data_of(c) if data is None else data, t_std=sd, t_mean=mu)
    assert (res['sync'] is not None) == (rule == 'batch')
    net.check_sync(res)
    if rule == 'batch':
        assert int(res['sync'][-1].item()) == 0, 'the sync error word'
    k = {key: cpu(res[key]) for key in KEYS}
    k['z'], k['logl'] = cpu(z), cpu(logl)
    return k


def same_bits(a, b, keys=KEYS + ('z', 'logl'), rows=slice(None)):
    keys = [k for k in keys if k != 'scale' or rows == slice(None)]   # (one scale per workgroup, not per walker)
    return all(a[k].dtype == b[k].dtype and np.array_equal(np.ascontiguousarray(a[k][rows]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in keys)


def own_draws(net, S, C):
    """the kernel's own draws of (SEED, OFF): normals on the device (fill_slice_noise: noise_normal4 of step 1 .. S), uniforms
    noise_uniform(seed, walker, step)"""
    dz = net.fill_slice_noise(S, C, seed=SEED, walker_offset=OFF)
    u = np.array([[orc.slice_uniform(SEED, OFF + w, it) for w in range(C)] for it in range(1, S + 1)], np.float32)
    return dz, u


def note(kernel, inst, c, C, rule, lag, near, agree, full, **ratios):
    print('RATIO %-26s %-12s %-26s C %2d S %d %-5s lag %d  near %.3f  agree %.3f  votes %s  %s' % (
        kernel, inst, mg.case_id(c), C, c.S, rule, lag, near, agree.mean(), 'same' if full else 'differ',
        '  '.join('%s %.3g' % kv for kv in ratios.items())))


_FLOWS, _STARTS, _RUNS = {}, {}, {}


def solo_flow(D):
    from nnest_amd import flow
    if D not in _FLOWS:
        nvp = flow.HipNVP(D, 16, 3, 1, seed=3)
        _FLOWS[D] = (nvp, orc.NVP(D, 16, 3, 1, nvp.store_packed()))
    return _FLOWS[D]


def oracle_run(c, rule='fixed', lag=0, star_kind='table', safe=False, wide=1.0):
    """(z0, l0, star, (dz on the device, u), restatement, margins) of a case on the kernel's own draws; star_kind 'free': L* = -1e300
    from the same start; safe: under the descriptor with NaN offsets; wide: times the tests' step (more proposals leave the box).
    Computed once, shared, never changed"""
    key = (c, rule, lag, star_kind, safe, wide)
    if key not in _RUNS:
        nvp, o = solo_flow(c.D)
        if c not in _STARTS:
            z0, l0, star = mg.start(c, lambda x: cpu(nvp.forward(x)[0]))
            _STARTS[c] = (z0, l0, star, own_draws(nvp, c.S, len(l0)))
        z0, l0, star, (dz, u) = _STARTS[c]
        if star_kind == 'free':
            star = -1e300
        margins = np.empty((c.S, len(l0)))
        ev = (lambda x: mg.exact_logl(c, x, mg.non_finite_data(c))) if safe else None
        ref = mg.trace(o, c, z0, l0, star, wide * mg.step_of(c.D), cpu(dz), u, rule, lag, evaluate=ev, margins=margins)
        _RUNS[key] = (z0, l0, star, (dz, u), ref, margins)
    return _RUNS[key]


def test_launch_has_the_new_argument():
    """(the parent commit fails here and in every test below: mh_steps has no like_glm, the flows no mh_glm_refusal)"""
    import inspect
    from nnest_amd import flow
    assert {'like_glm', 't_std', 't_mean'} <= set(inspect.signature(flow.HipNVP.mh_steps).parameters)
    nvp = solo_flow(2)[0]
    assert nvp.mh_glm_refusal() is None and nvp.mh_glm_refusal(2, 51, 'batch', 3) is None


PAIRS = [(c, rule, lag) for c in CASES for rule, lag in RULES]


@pytest.mark.parametrize('c,rule,lag', PAIRS, ids=['%s-%s%d' % (mg.case_id(c), rule, lag) for c, rule, lag in PAIRS])
def test_kernel_vs_restatement(c, rule, lag):
    nvp, o = solo_flow(c.D)
    z0, l0, star, (dz, u), ref, margins = oracle_run(c, rule, lag)
    C = len(l0)
    assert C == 51 and c.S > lag + 2
    inst = '<%d, %d>' % (units(c.D), mg.FAM[c.family])
    mg.assert_under_cap(margins, mg.case_id(c))   # (from the oracle alone, before any kernel output is looked at)
    k = fused(nvp, c, z0, l0, star, rule, lag)
    agree, near, r_x, r_ll, full = mg.hold(c, k, ref, margins, l0, star, rule, lag, what='mh_glm_kernel %s %s %s lag %d' % (inst, mg.case_id(c), rule, lag))
    assert k['scale'].shape == ((C + 3) // 4,) and len(set(k['scale'].tolist())) == 1   # one float per workgroup, the same number
    note('mh_glm_kernel', inst, c, C, rule, lag, near, agree, full, x=r_x, logL=r_ll, n_call=k['n_call'].mean(), n_accept=k['n_accept'].mean(),
         scale=float(k['scale'][0]))
    k2 = fused(nvp, c, z0, l0, star, rule, lag, noise=(dz, cuda(u)))   # the recorded-noise path replays the in-kernel draws
    assert same_bits(k, k2), 'recorded noise'
    k3 = fused(nvp, c, z0, l0, star, rule, lag)                        # the same launch twice
    assert same_bits(k, k3), 'the same launch twice'
    if rule == 'fixed':   # the two halves of the population launched separately, at their own offsets (a whole number of workgroups, and not)
        for h in (C // 2, 24):
            ka = fused(nvp, c, z0[:h], l0[:h], star, walker_offset=OFF)
            kb = fused(nvp, c, z0[h:], l0[h:], star, walker_offset=OFF + h)
            assert same_bits(k, ka, rows=slice(0, h)) and same_bits(k, kb, rows=slice(h, None)), 'halves at %d' % h


def test_null_t_is_the_identity():
    """t_std = t_mean = NULL against the vectors (1, 0): the same bits"""
    c = mg.Case('logistic', 2, 257, 1.0, mg.S_STEPS, False)
    nvp, o = solo_flow(c.D)
    z0, l0, star = mg.start(c, lambda x: cpu(nvp.forward(x)[0]))
    a = fused(nvp, c, z0, l0, star)
    b = fused(nvp, c, z0, l0, star, identity=True)
    assert same_bits(a, b) and a['n_accept'].sum() > 0


SAFE_CASES = [mg.NVP_TABLE[0], mg.NVP_TABLE[2]]   # U = 1 (two pass groups) and U = 3 (the weights in LDS)


@pytest.mark.parametrize('c', SAFE_CASES, ids=[mg.case_id(c) for c in SAFE_CASES])
@pytest.mark.parametrize('rule,lag', [('fixed', 0), ('batch', 0)])
def test_non_finite_logl_counts_as_minus_1e100(c, rule, lag):
    """NaN offsets (the library refuses a non-finite logl0 at the entry; the arrays' contents are the caller's) from a start with
    finite logl: every proposal's logL is non-finite, counts as -1e100 and fails logL > L*.  Nothing is accepted; z, every state and
    logl keep their bits; n_call still counts pre"""
    nvp, o = solo_flow(c.D)
    z0, l0, star, draws, ref, margins = oracle_run(c, rule, lag, safe=True)
    k = fused(nvp, c, z0, l0, star, rule, lag, data=mg.non_finite_data(c))
    mg.check_nothing_moves(k, ref, margins, z0, l0, what=mg.case_id(c))
    assert k['n_call'].sum() > 0
    print('SAFE %s %s: %d walkers, %d proposals with pre, none accepted' % (mg.case_id(c), rule, len(l0), int(k['n_call'].sum())))


SKIP_CASES = [mg.NVP_TABLE[1], mg.NVP_TABLE[4]]
WIDE = 3.0


@pytest.mark.parametrize('c', SKIP_CASES, ids=[mg.case_id(c) for c in SKIP_CASES])
def test_the_skipped_likelihood_shows_in_no_output(c):
    """the restatement evaluates the likelihood at every proposal, the kernel only where pre holds.  From a start with L* = -1e300
    (every proposal with pre is accepted: the likelihood decides nothing but is still the logL returned) and from the table's L*:
    n_call, n_accept and the chains are the restatement's on every walker it decided firmly.  At three times the tests' step, so that
    between 0.3 and 0.8 of the proposals are without pre (asserted on the restatement)"""
    nvp, o = solo_flow(c.D)
    for kind in ('free', 'table'):
        z0, l0, star, draws, ref, margins = oracle_run(c, star_kind=kind, wide=WIDE)
        assert 0.2 < ref['pre'].mean() < 0.7, ref['pre'].mean()
        k = fused(nvp, c, z0, l0, star, wide=WIDE)
        what = 'skip %s L* %s' % (mg.case_id(c), kind)
        mg.hold(c, k, ref, margins, l0, star, what=what)
        firm = np.min(margins, axis=0) >= mc.MARGIN_TOL
        assert firm.mean() >= sl.AGREE, what
        for key in ('n_call', 'n_accept'):
            np.testing.assert_array_equal(k[key][firm], ref[key][firm], err_msg='%s %s' % (what, key))
        assert np.max(np.abs(k['hist_x'][firm] - ref['x'][firm]) / (1.0 + np.abs(ref['x'][firm]))) < sl.TOL, what
        assert ref['n_call'].sum() < c.S * len(l0), what
        if kind == 'free':
            assert np.array_equal(k['n_call'], k['n_accept']), what
        print('SKIP %-26s L* %-5s: %d proposals, n_call %d (%.2f needed a likelihood), n_accept %d' % (
            mg.case_id(c), kind, c.S * len(l0), int(k['n_call'].sum()), k['n_call'].sum() / float(c.S * len(l0)), int(k['n_accept'].sum())))


def test_refusals_raise_without_a_launch():
    from nnest_amd import _lib, flow
    from nnest_amd.maf import HipMAF
    c = mg.NVP_EXTRA[0]
    nvp, _ = solo_flow(c.D)
    data = mg.data_of(c)
    z = torch.full((8, c.D), 0.25, dtype=torch.float32, device='cuda')
    logl = torch.full((8,), -3.5, dtype=torch.float64, device='cuda')
    kept = lambda: bool(torch.all(z == 0.25)) and bool(torch.all(logl == -3.5))
    args = (z, logl, -1e9, 0.5, 6)
    check = lambda net, D, C, flags: net._sym['mh_glm_check'](net._h, D, C, flags)
    # the batch rule on a grid that cannot be resident
    why = nvp.mh_glm_refusal(c.D, 10 ** 6, 'batch', 0)
    assert why is not None and 'resident' in why and check(nvp, c.D, 10 ** 6, _lib.MH_DYNAMIC_BATCH) == _lib.NNEST_E_UNSUPPORTED
    assert nvp.mh_glm_refusal(c.D, 10 ** 6, False) is None   # (the fixed step: any C)
    # the per-tile rule, the unconstrained walk, warm-up steps, form bits, the sync halves: argument errors
    assert 'flags' in nvp.mh_glm_refusal(c.D, 8, 'group')
    for flags in (_lib.MH_DYNAMIC_STEP, _lib.MH_UNCONSTRAINED, _lib.MH_DYNAMIC_BATCH | _lib.MH_UNCONSTRAINED, _lib.MH_DYNAMIC_BATCH | (1 << 20),
                  6 << 16, _lib.MH_DYNAMIC_BATCH | _lib.MH_SYNC_ZERO_NEXT, _lib.MH_DYNAMIC_BATCH | _lib.MH_SYNC_ZERO_PREV, 3 << 8):
        assert check(nvp, c.D, 8, flags) == E_ARG, hex(flags)
    with pytest.raises(_lib.NnestHipError, match='flags') as e:
        nvp.mh_steps(None, 1.0, *args, like_glm=data, dynamic='group')
    assert e.value.code == E_ARG
    with pytest.raises(ValueError, match='hard constraint'):
        nvp.mh_steps(None, 1.0, z, logl, None, 0.5, 6, like_glm=data)
    # the descriptor
    with pytest.raises(_lib.NnestHipError, match='logl0') as e:
        nvp.mh_steps(None, 1.0, *args, like_glm=dict(data, logl0=float('inf')))
    assert e.value.code == E_ARG
    with pytest.raises(_lib.NnestHipError, match="the likelihood's D=5 is not the flow's x_dim=%d" % c.D):
        nvp.mh_steps(None, 1.0, *args, like_glm=gk.make_like(5, 30, 'logistic', 1).hip_like_glm)
    assert 'D=5' in (nvp.mh_glm_refusal(5) or '')
    with pytest.raises(_lib.NnestHipError, match='glm: family=7'):
        nvp.mh_steps(None, 1.0, *args, like_glm=dict(data, family=7))
    with pytest.raises(ValueError, match='like_glm goes with like_id=None'):
        nvp.mh_steps(0, 5.0, *args, like_glm=data)
    with pytest.raises(ValueError, match='both or neither'):
        nvp.mh_steps(None, 1.0, *args, like_glm=data, t_std=np.ones(c.D))
    with pytest.raises(ValueError, match='one Metropolis kernel form'):
        nvp.mh_steps(None, 1.0, *args, like_glm=data, form='solo')
    maf = HipMAF(c.D, 16, 3, seed=1)
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        maf.mh_steps(None, 1.0, *args, like_glm=data)
    with pytest.raises(NotImplementedError):
        maf.mh_glm_refusal()
    other = flow.HipNVP(c.D, 32, 3, 1, seed=3)   # (not the default shape)
    assert 'hidden 16' in other.mh_glm_refusal()
    with pytest.raises(_lib.NnestHipError, match='hidden 16') as e:
        other.mh_steps(None, 1.0, *args, like_glm=data)
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    assert kept()
