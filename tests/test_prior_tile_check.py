"""CPU checks of tests/prior_tile_check.py: the tables reach every instantiation of both walk kernels under the normal prior; the
float32 restatements of the prior term in the tile's and the solo layout's own order meet the a-priori bound B_pi of
tests/gauss_prior_check.py with half of it to spare on every table row's start, so the inputs are fair before a GPU sees them; every
planted fault misses criterion (b) of tests/test_gpu_prior_tile.py on every table row where it applies, and `applies` is held to a
count per fault; the recorded prior widths and seeds satisfy their conditions on the restatement of the walk alone."""
import numpy as np
import pytest

from tests import fused_like_check as fl
from tests import gauss_prior_check as pk
from tests import glm_check as gk
from tests import prior_tile_check as pt
from tests import tile_like_check as tl

KEYS = (11, 21, 31, 41, 12, 22)
case_id = lambda c: '-'.join(str(v) for v in c)


def test_tables_reach_every_instantiation():
    assert {(tl.key(D, H), fam) for _, D, H, fam, _ in pt.SPLINE_CASES} == {(k, f) for k in KEYS for f in gk.FAMILIES}
    assert set(pt.SPLINE_DIMS) == set(tl.GLM_DIMS) | {(31, 16), (64, 16)} and len(pt.SPLINE_CASES) == 9 * 2 * 2
    assert [(n + 15) // 16 for n in pt.SPLINE_NS] == [2, 13]
    # the ragged lane group and the exactly full tile
    assert (31, 16) in pt.SPLINE_DIMS and 31 % 8 == 7 and (64, 16) in pt.SPLINE_DIMS and 64 == 32 * fl.units(64)
    # U = 1 .. 4, each with its edge-full width 32 U; U = 2 .. 4 from the edge-plus-one width 32 (U - 1) + 1; x_dim 1
    for fam in gk.FAMILIES:
        dims = {D for _, D, _, f, _ in pt.NVP_CASES if f == fam}
        assert dims == {1, 2, 31, 32, 33, 64, 65, 96, 97, 128}
        assert {fl.units(D) for D in dims} == {1, 2, 3, 4}
        for U in (1, 2, 3, 4):
            assert 32 * U in dims and fl.units(32 * U) == U
        for U in (1, 2, 3):
            assert 32 * U + 1 in dims and fl.units(32 * U + 1) == U + 1
    assert len(pt.NVP_CASES) == 20 and {n for c in pt.NVP_CASES for n in c[4:]} == {40}
    assert set(pt.PRIOR_SEEDS) == set(pt.CASES)
    assert pt.BETAS == (1.0, 0.5) and tl.DATA_CONFIG == (0.5, 3, 4, True) and (pt.C, pt.S) == (40, 6)


def test_applies_is_not_vacuous():
    """`applies`, listed: the rows of each table at which each fault can show, at the two powers of criterion (b)"""
    rows = [(c, beta) for c in pt.CASES for beta in pt.BETAS]
    count = {f: sum(pt.applies(f, c[0], c[1], beta) for c, beta in rows) for f in pt.FAULTS}
    n_spl, n_nvp = len(pt.SPLINE_CASES), len(pt.NVP_CASES)
    nt1 = 4 * sum(fl.units(D) == 1 for D, _ in pt.SPLINE_DIMS)          # (2, 16), (8, 32), (31, 16): no smaller instantiation
    full = 4 * sum(D % 32 == 0 for D, _ in pt.SPLINE_DIMS) + 2 * sum(D % 32 == 0 for D in pt.NVP_DIMS)   # no padded dimension
    assert nt1 == 12 and full == 8 + 8
    assert count == {'group_shift': 2 * (n_spl + n_nvp), 'class_swap': 2 * (n_spl + n_nvp), 'box_ignored': 2 * (n_spl + n_nvp),
                     'stride': 2 * (n_spl - nt1), 'stage_short': 2 * (n_spl - nt1), 'pad': 2 * (n_spl + n_nvp) - 2 * full,
                     'beta_on_prior': n_spl + n_nvp, 'beta_late': n_spl + n_nvp}
    assert all(v > 0 for v in count.values())
    # where a fault does not apply, it says why: NT = 1 and the solo layout; x_dim a multiple of 32; beta = 1
    for f in ('stride', 'stage_short'):
        assert not pt.applies(f, 'spline', 31, 0.5) and not pt.applies(f, 'nvp', 128, 0.5) and pt.applies(f, 'spline', 33, 1.0)
    assert not pt.applies('pad', 'spline', 64, 0.5) and not pt.applies('pad', 'nvp', 96, 0.5) and pt.applies('pad', 'nvp', 1, 1.0)
    assert not pt.applies('beta_late', 'nvp', 2, 1.0) and not pt.applies('beta_on_prior', 'spline', 2, 1.0)


def parts(case):
    """the start of a table row (prior_tile_check.start_parts) and the row's prior"""
    return pt.start_parts(case) + (pk.replay_prior(case[1], pt.PRIOR_SEEDS[case][0]),)


@pytest.mark.parametrize('case', pt.CASES, ids=case_id)
def test_restatement_has_half_the_bound_to_spare(case):
    """on every table row's start, under the row's own prior: the worst of the 39 finite rows, in the layout of the row's kernel"""
    share = pt.start_share(case, parts(case)[4])
    print('%s: the restatement uses %.3g of B_pi' % (case_id(case), share))
    t = parts(case)[0]
    assert np.isnan(t[2, 0]) and pt.prior32(case[0], parts(case)[4], t)[2] == -np.inf
    assert share <= 0.5, share


@pytest.mark.parametrize('case', pt.CASES, ids=case_id)
def test_faults_miss_criterion_b(case):
    flow, D = case[:2]
    t, ld, logl, inside, prior = parts(case)
    assert not inside[1] and inside[2] and np.isnan(t[2, 0]) and logl[2] == fl.SAFE
    fin = np.isfinite(t).all(1)
    assert fin.sum() == pt.C - 1 and (fin & inside).sum() > pt.C // 4
    logpi = pt.prior32(flow, prior, t)
    zero = pt.prior32(flow, pt.flat(prior), t)
    assert np.all(zero[fin] == 0.0) and not np.any(np.signbit(zero[fin])) and zero[2] == -np.inf
    for beta in pt.BETAS:
        lp_flat = pt.lp32(beta, logl, ld, inside, zero)
        assert np.array_equal(lp_flat[fin & inside], ((beta * logl) + ld)[fin & inside])   # (adding +0.0 is exact)
        clean = pt.prior_term_share(pt.lp32(beta, logl, ld, inside, logpi), lp_flat, prior, t, inside)
        assert clean <= 1.0, (beta, clean)
        for fault in pt.FAULTS:
            if fault in pt.LP_FAULTS or fault in (pt.TILE_FAULTS if flow == 'spline' else pt.SOLO_FAULTS):
                bad = pt.lp32(beta, logl, ld, inside, pt.prior32(flow, prior, t, fault), fault)
                share = pt.prior_term_share(bad, lp_flat, prior, t, inside)
                if pt.applies(fault, flow, D, beta):
                    assert share > 1.0, (fault, beta, share)
                else:   # (and there it is the unfaulted run, to the bit)
                    assert share == clean, (fault, beta, share)
            else:
                assert not pt.applies(fault, flow, D, beta), fault


def test_criterion_b_refuses_what_is_not_minus_inf_outside():
    case = pt.SPLINE_CASES[0]
    t, ld, logl, inside, prior = parts(case)
    lp_flat = pt.lp32(0.5, logl, ld, inside, 0.0 * logl)
    lp = pt.lp32(0.5, logl, ld, inside, pt.prior32('spline', prior, t))
    assert pt.prior_term_share(lp, lp_flat, prior, t, inside) <= 1.0
    for v in (0.0, np.nan, np.inf):
        bad = lp.copy()
        bad[1] = v
        assert pt.prior_term_share(bad, lp_flat, prior, t, inside) == np.inf
    bad = lp.copy()
    bad[5] = np.nan
    assert inside[5] and pt.prior_term_share(bad, lp_flat, prior, t, inside) == np.inf


@pytest.mark.parametrize('case', pt.CASES, ids=case_id)
def test_widths_and_seeds_are_fair(case):
    width, seed = pt.PRIOR_SEEDS[case]
    st = pt.case_stats(case, width, seed)
    print('%s: %s' % (case_id(case), st))
    base = max(b for b in pt.WIDTHS if b <= width)
    assert base <= width < 2.0 * base and width == pt.fine_width(case, base)   # (the first fine width that leaves the half)
    assert (width == base) == (case[1] >= 31) and 9000 + case[1] <= seed < 9000 + case[1] + pt.SEED_MORE
    if case in pt.BORDER_EXCEPTIONS:
        assert st['border'] == pt.BORDER_EXCEPTIONS[case] and 0 < st['border'] <= pt.BORDER_CAP * st['decisions']
        assert pt.stats_are_fair(st, pt.BORDER_CAP)
    else:
        assert st['border'] == 0 and pt.stats_are_fair(st)
