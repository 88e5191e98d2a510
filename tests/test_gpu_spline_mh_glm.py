"""[UNPINNED] The Metropolis proposal on a regression likelihood of user data, spline side (include/nnest_hip.h
nnest_spline_mh_glm_steps; nnest_spline_mh_glm.hip spline_mh_glm_kernel_team<NT, NH, FAM>; HipSpline.mh_steps(like_glm=...)).  The cases,
the restatement of the step and the checks are tests/mh_glm_check.py's; the launches and the bit comparisons
tests/test_gpu_mh_glm.py's.

Every table row (19 walkers: two tiles, one ragged) under the fixed step, the batch rule at lag 0, 1 and 3 and the per-tile rule: the
cap from the oracle first (a trip is a test-design failure: lower S or n), then the kernel against the restatement on
oracle.Spline and the kernel's own draws; the recorded-noise launch and the same launch again bit for bit, and under the fixed
step the two halves launched separately.  The tile evaluates the likelihood for all 16 walkers or for none: the skip test holds
counters and chains to the restatement's, which skips nothing, from L* = -1e300 and from the table's L*.  Run with  pytest -m gpu."""
import os

import numpy as np
import pytest
import torch

from tests import mh_checks as mc
from tests import mh_glm_check as mg
from tests import slice_like_check as sl
from tests.fused_like_check import units
from tests.test_gpu_mh_glm import E_ARG, OFF, WIDE, cpu, cuda, fused, note, own_draws, same_bits
from tests.test_gpu_spline_slice import oracle_of

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), 'golden')
IDS = ['%s-h%d' % (mg.case_id(sc.case), sc.H) for sc in mg.SPLINE_TABLE]
RULES = [('fixed', 0)] + [('batch', lag) for lag in mg.LAGS] + [('tile', 0)]
_RUNS = {}


def spline_flow(sc):
    """the HipSpline of a case: a seeded default initialisation (ActNorm's first-batch initialisation is completed by the first
    forward batch, which `oracle_run` pushes through before it builds the oracle), or the trained weights of a golden file"""
    from nnest_amd.spline import HipSpline
    if sc.golden is None:
        return HipSpline(sc.case.D, sc.H, 3, 8, 3.0, seed=3)
    g = np.load(os.path.join(G, sc.golden))
    assert int(g['D']) == sc.case.D and int(g['H']) == sc.H
    sp = HipSpline(int(g['D']), int(g['H']), int(g['B']), int(g['K']), float(g['tail']))
    sp.load_packed(g['w_trained'], g['P'])
    sp.data_dep_init_done = True   # past ActNorm's first-batch initialisation (networks.py:696)
    return sp


def oracle_run(sc, rule='fixed', lag=0, star_kind='table', safe=False, wide=1.0, count=None):
    """(flow, z0, l0, star, (dz on the device, u), restatement, margins); computed once, shared, never changed.  The runs of a case
    share the flow, the start and the draws: the flow's ActNorm layers are set by the first forward batch"""
    c = sc.case
    C = sc.C if count is None else count
    key = (sc, rule, lag, star_kind, safe, wide, C)
    if key not in _RUNS:
        if (sc, 'flow') not in _RUNS:
            _RUNS[sc, 'flow'] = spline_flow(sc)
        if (sc, 'start', C) not in _RUNS:
            sp = _RUNS[sc, 'flow']
            z0, l0, star = mg.start(c, lambda x: cpu(sp.forward(x)[0]), count=C)
            _RUNS[sc, 'start', C] = (sp, oracle_of(sp), z0, l0, star, own_draws(sp, c.S, C))
        sp, o, z0, l0, star, (dz, u) = _RUNS[sc, 'start', C]
        if star_kind == 'free':
            star = -1e300
        margins = np.empty((c.S, C))
        ev = (lambda x: mg.exact_logl(c, x, mg.non_finite_data(c))) if safe else None
        ref = mg.trace(o, c, z0, l0, star, wide * mg.step_of(c.D), cpu(dz), u, rule, lag, evaluate=ev, margins=margins)
        _RUNS[key] = (sp, z0, l0, star, (dz, u), ref, margins)
    return _RUNS[key]


def test_launch_has_the_new_argument():
    """(the parent commit fails here and in every test below)"""
    from nnest_amd.spline import HipSpline
    assert 'mh_glm_refusal' in dir(HipSpline) and HipSpline.MH_GLM_WALKERS_PER_WORKGROUP == 16


PAIRS = [(sc, rule, lag) for sc in mg.SPLINE_TABLE for rule, lag in RULES]


@pytest.mark.parametrize('sc,rule,lag', PAIRS, ids=['%s-h%d-%s%d' % (mg.case_id(sc.case), sc.H, rule, lag) for sc, rule, lag in PAIRS])
def test_kernel_vs_restatement(sc, rule, lag):
    c, C = sc.case, sc.C
    sp, z0, l0, star, (dz, u), ref, margins = oracle_run(sc, rule, lag)
    assert C == 19 and len(l0) == C and c.S > lag + 2
    inst = '<%d, %d, %d>' % (units(c.D), sc.H // 16, mg.FAM[c.family])
    mg.assert_under_cap(margins, mg.case_id(c))   # (from the oracle alone, before any kernel output is looked at)
    k = fused(sp, c, z0, l0, star, rule, lag)
    agree, near, r_x, r_ll, full = mg.hold(c, k, ref, margins, l0, star, rule, lag,
                                           what='spline_mh_glm_kernel_team %s %s %s lag %d' % (inst, mg.case_id(c), rule, lag))
    assert k['scale'].shape == ((C + 15) // 16,) and (rule == 'tile' or len(set(k['scale'].tolist())) == 1)
    note('spline_mh_glm_kernel_team', inst, c, C, rule, lag, near, agree, full, x=r_x, logL=r_ll, n_call=k['n_call'].mean(),
         n_accept=k['n_accept'].mean(), scale=float(k['scale'][0]))
    k2 = fused(sp, c, z0, l0, star, rule, lag, noise=(dz, cuda(u)))   # the recorded-noise path replays the in-kernel draws
    assert same_bits(k, k2), 'recorded noise'
    k3 = fused(sp, c, z0, l0, star, rule, lag)                        # the same launch twice
    assert same_bits(k, k3), 'the same launch twice'
    if rule == 'fixed':   # the two halves of the population launched separately, at their own offsets
        h = C // 2
        ka = fused(sp, c, z0[:h], l0[:h], star, walker_offset=OFF)
        kb = fused(sp, c, z0[h:], l0[h:], star, walker_offset=OFF + h)
        assert same_bits(k, ka, rows=slice(0, h)) and same_bits(k, kb, rows=slice(h, None)), 'halves'


SAFE_CASES = [mg.SPLINE_TABLE[0], mg.SPLINE_TABLE[1]]


@pytest.mark.parametrize('sc', SAFE_CASES, ids=IDS[:2])
@pytest.mark.parametrize('rule,lag', [('fixed', 0), ('tile', 0)])
def test_non_finite_logl_counts_as_minus_1e100(sc, rule, lag):
    """NaN offsets from a start with finite logl (tests/test_gpu_mh_glm.py has the reason): nothing is accepted; z, every state and
    logl keep their bits; n_call still counts pre"""
    c = sc.case
    sp, z0, l0, star, draws, ref, margins = oracle_run(sc, rule, lag, safe=True)
    k = fused(sp, c, z0, l0, star, rule, lag, data=mg.non_finite_data(c))
    mg.check_nothing_moves(k, ref, margins, z0, l0, what=mg.case_id(c))
    assert k['n_call'].sum() > 0
    print('SAFE %s %s: %d walkers, %d proposals with pre, none accepted' % (mg.case_id(c), rule, len(l0), int(k['n_call'].sum())))


SKIP_CASES = [mg.SPLINE_TABLE[1], mg.SPLINE_TABLE[4]]
SKIP_C = 17


@pytest.mark.parametrize('sc', SKIP_CASES, ids=[IDS[1], IDS[4]])
def test_the_skipped_likelihood_shows_in_no_output(sc):
    """the tile skips the likelihood in a step where none of its walkers has pre (17 walkers here: the second tile holds one);
    from L* = -1e300 and from the table's L*, n_call, n_accept and the chains are the restatement's, which skips nothing.  At three
    times the tests' step, so that there are (tile, step) pairs without any pre (asserted on the restatement) and pairs with"""
    c = sc.case
    for kind in ('free', 'table'):
        sp, z0, l0, star, draws, ref, margins = oracle_run(sc, star_kind=kind, wide=WIDE, count=SKIP_C)
        k = fused(sp, c, z0, l0, star, wide=WIDE)
        what = 'skip %s L* %s' % (mg.case_id(c), kind)
        mg.hold(c, k, ref, margins, l0, star, what=what)
        firm = np.min(margins, axis=0) >= mc.MARGIN_TOL
        assert firm.mean() >= sl.AGREE, what
        for key in ('n_call', 'n_accept'):
            np.testing.assert_array_equal(k[key][firm], ref[key][firm], err_msg='%s %s' % (what, key))
        assert np.max(np.abs(k['hist_x'][firm] - ref['x'][firm]) / (1.0 + np.abs(ref['x'][firm]))) < sl.TOL, what
        skipped = sum(int(not ref['pre'][s, g].any()) for s in range(c.S) for g in mg.groups_of(SKIP_C, 'tile'))
        assert 0 < skipped < c.S * 2, (what, skipped)
        print('SKIP %-26s L* %-5s: %d proposals, n_call %d, n_accept %d; %d of %d (tile, step) pairs without any pre' % (
            mg.case_id(c), kind, c.S * SKIP_C, int(k['n_call'].sum()), int(k['n_accept'].sum()), skipped, c.S * 2))


def test_refusals_raise_without_a_launch():
    from nnest_amd import _lib
    sc = mg.SPLINE_TABLE[0]
    c = sc.case
    sp = oracle_run(sc)[0]
    data = mg.data_of(c)
    z = torch.full((8, c.D), 0.25, dtype=torch.float32, device='cuda')
    logl = torch.full((8,), -3.5, dtype=torch.float64, device='cuda')
    kept = lambda: bool(torch.all(z == 0.25)) and bool(torch.all(logl == -3.5))
    args = (z, logl, -1e9, 0.5, 6)
    check = lambda D, C, flags: sp._sym['mh_glm_check'](sp._h, D, C, flags)
    why = sp.mh_glm_refusal(c.D, 10 ** 6, 'batch', 0)
    assert why is not None and 'resident' in why and check(c.D, 10 ** 6, _lib.MH_DYNAMIC_BATCH) == _lib.NNEST_E_UNSUPPORTED
    assert sp.mh_glm_refusal(c.D, 10 ** 6, 'group') is None and sp.mh_glm_refusal(c.D, 10 ** 6, False) is None   # (no communication: any C)
    for flags in (_lib.MH_UNCONSTRAINED, _lib.MH_DYNAMIC_STEP | _lib.MH_DYNAMIC_BATCH, _lib.MH_DYNAMIC_STEP | (1 << 8), _lib.MH_DYNAMIC_BATCH | (1 << 20),
                  1 << 16, _lib.MH_DYNAMIC_BATCH | _lib.MH_SYNC_ZERO_NEXT):
        assert check(c.D, 8, flags) == E_ARG, hex(flags)
    with pytest.raises(_lib.NnestHipError, match='logl0') as e:
        sp.mh_steps(None, 1.0, *args, like_glm=dict(data, logl0=float('nan')))
    assert e.value.code == E_ARG
    with pytest.raises(_lib.NnestHipError, match='resident') as e:   # (refused at the entry too: nothing is launched)
        big = torch.zeros(10 ** 6, c.D, dtype=torch.float32, device='cuda')
        sp.mh_steps(None, 1.0, big, torch.zeros(10 ** 6, dtype=torch.float64, device='cuda'), -1e9, 0.5, 6, like_glm=data, dynamic='batch', lag=0)
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    with pytest.raises(ValueError, match='hard constraint'):
        sp.mh_steps(None, 1.0, z, logl, None, 0.5, 6, like_glm=data)
    with pytest.raises(ValueError, match='like_glm goes with like_id=None'):
        sp.mh_steps(0, 5.0, *args, like_glm=data)
    assert kept()
