"""[UNPINNED] The slice proposal on a regression likelihood of user data, spline side (include/nnest_hip.h
nnest_spline_slice_glm_steps; nnest_spline_slice_glm.hip spline_slice_glm_kernel_team<NT, NH, FAM>; HipSpline.slice_steps(like_glm=...);
slice_rounds(like_glm=...) on the spline flow).  Build-defined.  The cases, the oracle's likelihood, the start and the checks are
tests/slice_glm_check.py's; the launches and the bit comparisons tests/test_gpu_slice_glm.py's.

Every table row: the near share from the oracle first (a trip is a test-design failure: lower S), then the kernel against
oracle.slice_sample(oracle.Spline) on the kernel's own directions; the recorded-noise launch, the same launch again and a shard, bit for
bit.  The tile evaluates the likelihood for all 16 walkers or for none: the skip test holds the counters to the oracle's, which skips
nothing, from L* = -1e300 and from the table's L*.  Run with  pytest -m gpu."""
import os

import numpy as np
import pytest
import torch

from tests import slice_glm_check as sg
from tests import slice_like_check as sl
from tests.test_gpu_slice_glm import OFF, SEED, cpu, fused, note, rounds, same_bits
from tests.test_gpu_spline_slice import oracle_of

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), 'golden')
IDS = ['%s-h%d' % (sg.case_id(sc.case), sc.H) for sc in sg.SPLINE_TABLE]
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


def oracle_run(sc, star_kind='table', safe=False):
    """(flow, z0, l0, star, dz on the device, oracle result, margins); computed once per (case, L*), shared, never changed.  The
    three runs of a case share the flow: its ActNorm layers are set by the first"""
    c = sc.case
    key = (sc, star_kind, safe)
    if key not in _RUNS:
        sp = _RUNS[sc, 'flow'] if (sc, 'flow') in _RUNS else _RUNS.setdefault((sc, 'flow'), spline_flow(sc))
        z0, l0, star = sg.start(c, lambda u: cpu(sp.forward(u)[0]), count=sc.C)
        if star_kind == 'free':
            star = -1e300
        o = oracle_of(sp)
        dz = sp.fill_slice_noise(c.S, sc.C, seed=SEED, walker_offset=OFF)
        margins = np.empty((c.S, sc.C))
        ev = (lambda x: sg.exact_logl(c, x, sg.non_finite_data(c))) if safe else None
        ref = sg.slice_sample(o, c, z0, l0, star, cpu(dz), SEED, OFF, evaluate=ev, margins=margins)
        _RUNS[key] = (sp, z0, l0, star, dz, ref, margins)
    return _RUNS[key]


@pytest.mark.parametrize('sc', sg.SPLINE_TABLE, ids=IDS)
def test_kernel_vs_oracle(sc):
    c, C = sc.case, sc.C
    sp, z0, l0, star, dz, ref, margins = oracle_run(sc)
    assert sp.slice_glm_refusal() is None and C % 16 != 0 and C > 16
    inst = '<%d, %d, %d>' % (sg.spline_key(sc) + (sg.FAM[c.family],))
    k, logl = fused(sp, c, z0, l0, star)
    same, near, r_x, r_ll = sg.hold(c, k, logl, ref, margins, l0, star, what='spline_slice_glm_kernel_team %s %s' % (inst, sg.case_id(c)))
    assert np.array_equal(k['moved'], (k['hist_x'][:, 0] != k['x']).all(1))   # launch_mh_all_moved: the first x against the last
    note('spline_slice_glm_kernel_team', inst, c, C, near, same, x=r_x, logL=r_ll, n_eval=k['n_eval'].mean(), n_call=k['n_call'].mean())
    k1, logl1 = fused(sp, c, z0, l0, star, form='team')   # the one form, named
    assert same_bits(k, k1) and np.array_equal(logl, logl1), 'form team'
    k2, logl2 = fused(sp, c, z0, l0, star, noise=dz)      # the recorded-noise path replays the in-kernel draws
    assert same_bits(k, k2) and np.array_equal(logl, logl2), 'recorded noise'
    k3, logl3 = fused(sp, c, z0, l0, star)                # the same launch twice
    assert same_bits(k, k3) and np.array_equal(logl, logl3), 'the same launch twice'
    h = C // 2                                             # a shard: the second half of the walkers, at their own offset
    k4, logl4 = fused(sp, c, z0[h:], l0[h:], star, walker_offset=OFF + h)
    assert same_bits(k, k4, rows=slice(h, None)) and np.array_equal(logl[h:], logl4), 'shard'


SAFE_CASES = [sg.SPLINE_TABLE[0], sg.SPLINE_TABLE[1]]


@pytest.mark.parametrize('sc', SAFE_CASES, ids=IDS[:2])
def test_non_finite_logl_counts_as_minus_1e100(sc):
    """NaN offsets from a start with finite logl (tests/test_gpu_slice_glm.py has the reason): no update moves; z, every state and
    logl keep their bits; n_call and n_eval are the oracle's"""
    c = sc.case
    sp, z0, l0, star, dz, ref, margins = oracle_run(sc, safe=True)
    k, logl = fused(sp, c, z0, l0, star, data=sg.non_finite_data(c))
    sl.check_nothing_moves(k, ref, z0, l0, k['z'], logl, what=sg.case_id(c))
    assert not k['moved'].any() and k['n_call'].sum() > 0
    print('SAFE %s: %d walkers, %d candidates, %d with a likelihood, none moved' % (sg.case_id(c), len(l0), int(k['n_eval'].sum()), int(k['n_call'].sum())))


SKIP_CASES = [sg.SPLINE_TABLE[1], sg.SPLINE_TABLE[4]]


@pytest.mark.parametrize('sc', SKIP_CASES, ids=[IDS[1], IDS[4]])
def test_the_skipped_likelihood_shows_in_no_counter(sc):
    c = sc.case
    for kind in ('free', 'table'):
        sp, z0, l0, star, dz, ref, margins = oracle_run(sc, kind)
        near = sl.near_share(margins)
        what = 'skip %s L* %s' % (sg.case_id(c), kind)
        assert near <= 1.0 - sl.AGREE, '%s: near share %.3g: a TEST-DESIGN failure, not the kernel\'s; lower S' % (what, near)
        k, logl = fused(sp, c, z0, l0, star)
        sl.compare(k, ref, margins, what=what)
        firm = np.min(margins, axis=0) >= sl.TOL
        for key in ('n_eval', 'n_call', 'n_move'):
            np.testing.assert_array_equal(k[key][firm], ref[key][firm], err_msg='%s %s' % (what, key))
        assert ref['n_call'].sum() < ref['n_eval'].sum(), what
        sg.check_logl_of_own_x(c, logl, k['x'], k['n_move'], l0, what=what)
        print('SKIP %-26s L* %-5s: n_eval %d, n_call %d (%.2f of the candidates needed a likelihood)' % (
            sg.case_id(c), kind, int(k['n_eval'].sum()), int(k['n_call'].sum()), k['n_call'].sum() / float(k['n_eval'].sum())))


def test_rounds_with_the_device_likelihood_vs_the_same_oracle_run():
    sc = sg.SPLINE_TABLE[4]
    c = sc.case
    sp, z0, l0, star, dz, ref, margins = oracle_run(sc)
    k, logl = rounds(sp, c, z0, l0, star)
    same, near, r_x, r_ll = sg.hold(c, k, logl, ref, margins, l0, star, what='slice_rounds like_glm spline %s' % sg.case_id(c))
    note('slice_rounds like_glm', 'spline', c, sc.C, near, same, x=r_x, logL=r_ll)


def test_refusals_raise_without_a_launch():
    from nnest_amd import _lib
    from nnest_amd.spline import HipSpline
    from tests import glm_check as gk
    sc = sg.SPLINE_TABLE[4]
    c = sc.case
    sp = oracle_run(sc)[0]
    data = sg.data_of(c)
    z = torch.full((8, c.D), 0.25, dtype=torch.float32, device='cuda')
    logl = torch.full((8,), -3.5, dtype=torch.float64, device='cuda')
    args = (z, logl, -1e9, 0.5, 2)
    for form in ('wave', 'pair'):
        with pytest.raises(ValueError, match='team form only'):
            sp.slice_steps(None, 1.0, *args, like_glm=data, form=form)
    with pytest.raises(_lib.NnestHipError, match="the likelihood's D=5 is not the flow's x_dim=%d" % c.D) as e:
        sp.slice_steps(None, 1.0, *args, like_glm=gk.make_like(5, 30, 'logistic', 1).hip_like_glm)
    assert e.value.code == 1 and 'D=5' in (sp.slice_glm_refusal(5) or '')
    with pytest.raises(_lib.NnestHipError, match='glm: family=7'):
        sp.slice_steps(None, 1.0, *args, like_glm=dict(data, family=7))
    with pytest.raises(ValueError, match='like_glm goes with like_id=None'):
        sp.slice_steps(0, 5.0, *args, like_glm=data)
    with pytest.raises(_lib.NnestHipError):   # (a shape the tile has no instantiation for is no spline handle at all)
        HipSpline(70, 32, 3, 8, 3.0, seed=3)
    assert sp.slice_glm_refusal() is None
    assert bool(torch.all(z == 0.25)) and bool(torch.all(logl == -3.5))
