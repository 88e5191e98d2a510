"""CPU checks of tests/tile_like_check.py: the float32 restatement of the two tile evaluators of user data meets the check of
tests/test_gpu_tile_data_likes.py -- float64 within the a-priori bound B -- with half the bound to spare at every table entry, so the
inputs are fair before a GPU sees them; every planted fault misses it at the entries it can show at; and the seeds of both GPU files
satisfy their condition on the restatement of the walk alone."""
import numpy as np
import pytest

from tests import fused_like_check as fl
from tests import glm_check as gk
from tests import tile_like_check as tl


def gdata_rows(D):
    sd, mu = tl.affine(D, D)
    return fl.T32(tl.data_start_x(D), sd, mu)


def test_tables_reach_every_instantiation():
    assert {tl.key(D, H) for D, H in tl.GDATA_CASES if D >= 2} == {11, 21, 31, 41, 12, 22}
    assert {(tl.key(D, H), fam) for D, H, fam, _ in tl.GLM_CASES} == {(k, f) for k in (11, 21, 31, 41, 12, 22) for f in gk.FAMILIES}
    for D, H, fam in {c[:3] for c in tl.GLM_CASES}:
        assert {n for d, h, f, n in tl.GLM_CASES if (d, h, f) == (D, H, fam)} == set(tl.GLM_NS)
    assert [(n + 15) // 16 for n in tl.GLM_NS] == [1, 2, 4, 5, 13]
    # every (row block, column block) pair the tile can skip is skipped by some case: rb = 2 .. 7 skip rb // 2 = 1 .. 3 blocks
    assert {(rb, rb // 2) for D, _ in tl.GDATA_CASES for rb in range(2 * fl.units(D)) if 16 * rb < D} >= {(rb, rb // 2) for rb in range(8)}
    assert set(tl.DATA_SEEDS) == {('gdata', D, H) for D, H in tl.GDATA_CASES if D >= 2} | {('glm',) + c for c in tl.GLM_CASES}


@pytest.mark.parametrize('D', sorted({D for D, _ in tl.GDATA_CASES}))
def test_gdata_restatement_and_faults(D):
    data = tl.data_like('gdata', D)
    t = gdata_rows(D)
    clean = tl.gdata_tile32(data, t)
    r = tl.gdata_ratio(clean, data, t)
    print('gdata x_dim %d: the restatement uses %.3g of B' % (D, r))
    assert r <= 0.5 and clean[2] == fl.SAFE
    shows = {'col_start': D >= 2, 'strict': True, 'break': D % 16 != 0, 'pad_col': D % 8 != 0, 'mu_shift': D > 8}
    for fault in tl.GDATA_FAULTS:
        got = tl.gdata_tile32(data, t, fault=fault)
        if shows[fault]:
            assert tl.gdata_ratio(got, data, t) > 1.0, (fault, D)
        elif fault in ('break', 'pad_col'):
            assert np.array_equal(got, clean), (fault, D)


@pytest.mark.parametrize('D,H', tl.GLM_DIMS)
@pytest.mark.parametrize('fam', gk.FAMILIES)
def test_glm_restatement_and_faults(D, H, fam):
    sd, mu = tl.affine(D, D)
    t = fl.T32(tl.data_start_x(D), sd, mu)
    for n in tl.GLM_NS:
        data = tl.data_like('glm', D, fam, n)
        at, y, o = (np.array(data[k], np.float32) for k in ('at', 'y', 'o'))
        assert at.shape[1] % 64 == 0 and at.shape[1] >= n
        clean = tl.glm_tile32(data, t)
        r = tl.glm_ratio(clean, data, t)
        print('glm %s x_dim %d n %d: the restatement uses %.3g of B' % (fam, D, n, r))
        assert r <= 0.5 and clean[2] == fl.SAFE
        # the padding behind n dirtied as tests/test_gpu_mcmc_glm.py dirties it: the same bits
        rng = np.random.RandomState(n)
        at[:, n:] = rng.normal(size=at[:, n:].shape) * 1e6
        y[n:], o[n:] = 7.0, np.nan
        assert np.array_equal(tl.glm_tile32(dict(data, at=at, y=y, o=o), t), clean)
        shows = {'rows': n % 16 != 0, 'wave3': n >= 49, 'acc2': fl.units(D) == 1 and n >= 65, 'last_col': D % 8 != 0, 'offset': True}
        for fault in tl.GLM_FAULTS:
            got = tl.glm_tile32(data, t, fault=fault)
            if shows[fault]:
                assert tl.glm_ratio(got, data, t) > 1.0, (fault, D, n)
            else:
                assert np.array_equal(got, clean), (fault, D, n)


@pytest.mark.parametrize('case', sorted(tl.WALK_SEEDS, key=repr), ids=lambda c: '-'.join(str(v) for v in c))
def test_walk_seeds_are_fair(case):
    target_of_beta, z0 = tl.analytic_case(*case)
    assert tl.seed_is_fair(target_of_beta, z0, tl.WALK_SEEDS[case], list(tl.CONFIGS.values()))


@pytest.mark.parametrize('case', sorted(tl.DATA_SEEDS, key=repr), ids=lambda c: '-'.join(str(v) for v in c))
def test_data_seeds_are_fair(case):
    target_of_beta, z0, _ = tl.data_case(*case)
    assert tl.seed_is_fair(target_of_beta, z0, tl.DATA_SEEDS[case], [tl.DATA_CONFIG])
