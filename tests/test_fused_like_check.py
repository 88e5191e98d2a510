"""CPU checks of tests/fused_like_check.py: the float32 restatement of the kernels' likelihood arithmetic meets the bound the GPU
tests hold the kernels to with at least half of it to spare, in both register layouts, at every (likelihood, recipe, x_dim) of the
GPU tables; each planted fault is caught by the check the GPU tests run; the restated draws give the replay seeds; the likelihood
classes hand the kernels the parameters the table holds."""
import numpy as np
import pytest

from tests import fused_like_check as fl

ROWS = 2000


def rows(D, seed=0, n=ROWS):
    return (np.random.RandomState(1000 + seed).normal(size=(n, D)) * 0.5).astype(np.float32)


def worst(name, recipe, D, layout, fault=None, x=None):
    sd, mu = fl.affine(name, recipe, D, D)
    x = rows(D, D) if x is None else x
    params = fl.LIKES[name]['params']
    logl = fl.restated32(name, fl.T32(x, sd, mu), params, layout, fault=fault)
    return fl.check_logl_of_own_x(logl, x, sd, mu, name, params, what='%s %s x_dim %d %s' % (name, recipe, D, layout))


def test_table_is_the_issues_and_the_ids_are_the_librarys():
    from nnest_amd import _lib
    assert {k: v['id'] for k, v in fl.LIKES.items()} == _lib.LIKE_IDS
    assert len(fl.TABLE) == 18 + 3 + 3 + 3 + 2 + 2 + 1
    for name, recipe, D in fl.TABLE:
        assert fl.LIKES[name]['dims'](D) and recipe in fl.LIKES[name]['recipes']
    assert [fl.units(D) for D in (1, 2, 32, 33, 64, 65, 96, 97, 128)] == [1, 1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize('layout', ['solo', 'tile'])
def test_restatement_meets_half_the_bound(layout):
    """worst error / bound per likelihood over the tables' x_dim; LIKES' `restated` figures are these, rounded up"""
    by_like = {}
    for name, recipe, D in fl.TABLE:
        r = worst(name, recipe, D, layout)
        by_like[name] = max(by_like.get(name, 0.0), r)
        assert r <= 0.5, (name, recipe, D, layout, r)
    print('%s layout, worst error / bound: %s' % (layout, ', '.join('%s %.3g' % kv for kv in sorted(by_like.items()))))
    for name, r in by_like.items():
        assert r <= fl.LIKES[name]['restated'][layout == 'tile'], (name, r)


def test_rosenbrock_sizes():
    """the issue's figures for the recipes: |logL| up to 2e4 at x_dim 128 (wide), about 4.5 x_dim (valley)"""
    for D in (33, 128):
        sd, mu = fl.affine('rosenbrock', 'valley', D, D)
        v = -fl.exact_logl('rosenbrock', fl.T32(rows(D, D), sd, mu))
        assert 3.0 * D < np.median(v) < 6.0 * D, (D, np.median(v))
    sd, mu = fl.affine('rosenbrock', 'wide', 128, 128)
    v = -fl.exact_logl('rosenbrock', fl.T32(rows(128, 128), sd, mu))
    assert 2e3 < v.max() < 4e4


FAULT_CASES = [('rosenbrock', 'wide', 33, 'boundary'), ('rosenbrock', 'valley', 33, 'boundary'), ('rosenbrock', 'valley', 128, 'boundary'),
               ('rosenbrock', 'wide', 33, 'mask'), ('rosenbrock', 'valley', 33, 'mask'),
               ('rosenbrock', 'valley', 32, 'mask'), ('rosenbrock', 'valley', 64, 'mask'), ('rosenbrock', 'valley', 128, 'mask'),
               ('rosenbrock', 'wide', 128, 'mask'),
               ('gaussmix', 'main', 20, 'base'), ('gaussmix', 'main', 81, 'base'), ('himmelblau', 'main', 66, 'last_pair'),
               ('gaussian', 'main', 7, 'corr'), ('gaussian', 'main', 100, 'corr'), ('shell', 'main', 5, 'triple'),
               ('double_shell', 'main', 5, 'triple'), ('double_shell', 'main', 97, 'triple')]


# (the tile layout has no wrap: behind the last tile the neighbour is 0, so 'mask' at x_dim 32 U is the solo layout's fault alone)
FAULT_CASES = [c + (layout,) for c in FAULT_CASES for layout in ('solo', 'tile') if not (layout == 'tile' and c[3] == 'mask' and c[2] % 32 == 0)]


@pytest.mark.parametrize('name,recipe,D,fault,layout', FAULT_CASES)
def test_planted_faults_are_caught(name, recipe, D, fault, layout):
    assert worst(name, recipe, D, layout) <= 0.5
    with pytest.raises(AssertionError, match='outside the bound|not -1e100'):
        worst(name, recipe, D, layout, fault=fault)


@pytest.mark.parametrize('name,D', [('rosenbrock', 33), ('gaussmix', 20), ('himmelblau', 32), ('gaussian', 7), ('eggbox', 2), ('shell', 5),
                                    ('double_shell', 5)])
def test_a_nan_row_must_be_mapped(name, D):
    recipe = sorted(fl.LIKES[name]['recipes'])[0]
    x = rows(D, D, 40)
    x[7, 0] = np.nan
    sd, mu = fl.affine(name, recipe, D, D)
    params = fl.LIKES[name]['params']
    for layout in ('solo', 'tile'):
        logl = fl.restated32(name, fl.T32(x, sd, mu), params, layout)
        assert logl[7] == fl.SAFE
        assert worst(name, recipe, D, layout, x=x) <= 0.5
        with pytest.raises(AssertionError, match='not -1e100'):
            worst(name, recipe, D, layout, fault='nan', x=x)


def test_lp_split_checks():
    rng = np.random.RandomState(3)
    ll, ld = rng.normal(size=50) * 100.0, rng.normal(size=50)
    inside = rng.uniform(size=50) < 0.7
    lp = np.where(inside, ll + ld, -np.inf)
    b = fl.logl_bound(ld)
    assert fl.check_lp_split(lp, ll, ld, inside, b) < 1e-6
    assert 0.4 < fl.check_lp_split(lp + 0.5 * b, ll, ld, inside, b) < 0.6
    with pytest.raises(AssertionError, match='outside the bound'):
        fl.check_lp_split(lp + 1.5 * b, ll, ld, inside, b)
    with pytest.raises(AssertionError, match='outside the bound'):   # the log-det's sign
        fl.check_lp_split(np.where(inside, ll - ld, -np.inf), ll, ld, inside, b)
    with pytest.raises(AssertionError, match='not -inf'):            # a row outside the box that kept a finite target
        fl.check_lp_split(ll + ld, ll, ld, inside, b)
    with pytest.raises(AssertionError, match='outside the bound'):   # a row inside the box reported as outside
        fl.check_lp_split(np.full(50, -np.inf), ll, ld, np.ones(50, bool), b)
    ll[0], inside[0] = fl.SAFE, True
    lp = np.where(inside, ll + ld, -np.inf)
    assert lp[0] == fl.SAFE and fl.check_lp_split(lp, ll, ld, inside, b) < 1e-6


def test_box_and_T():
    sd, mu = fl.affine('rosenbrock', 'valley', 33, 33)
    lo, hi = fl.box_for(sd, mu)
    share = fl.in_box(fl.T32(rows(33, 1), sd, mu), lo, hi).mean()
    assert 0.6 < share < 0.8, share
    x = np.zeros((3, 33), np.float32)
    x[1, 5] = np.nan      # a NaN coordinate counts as inside
    x[2, 5] = 100.0
    assert fl.in_box(fl.T32(x, sd, mu), lo, hi).tolist() == [True, True, False]
    assert fl.T32(x, sd, mu).dtype == np.float32


# ---- the replay seeds of tests/test_gpu_fused_likes.py (the x-space run, Rosenbrock in the valley) ---------------------------------
@pytest.mark.parametrize('mix', [False, True], ids=['stretch', 'mix'])
@pytest.mark.parametrize('D', [3, 33, 65, 128])
def test_replay_seeds_have_no_borderline_decision(D, mix):
    """the seeds the GPU replay uses (REPLAY_SEEDS: the first of 6000 + x_dim, ... that passes here): the restatement alone, on the
    restated draws, has no decision within three times the replay's margin, and some walkers move"""
    from tests.fused_like_check import MIX, REPLAY_C, REPLAY_S, REPLAY_SEEDS, replay_case
    x0, sd, mu, lo, hi = replay_case(D)
    rs = fl.Restated(None, sd, mu, lo, hi, 'rosenbrock', ())
    moves = MIX if mix else None
    seed = REPLAY_SEEDS[D, mix]
    draws = fl.ensemble_draws(seed, REPLAY_C, REPLAY_S, D, moves)
    if mix:
        assert {d[2] for d in draws} == {fl.STRETCH, fl.DE}, 'the seed must give a step of each kind'
    shares, moved = fl.replay_margins(x0, draws, rs.lp)
    print('x_dim %d %s seed %d: smallest margin share %.3g, %d of %d moved' % (D, 'mix' if mix else 'stretch', seed, shares.min(), moved,
                                                                              REPLAY_C * REPLAY_S))
    assert shares.min() > 3.0 and moved >= 5


def test_restated_split_is_a_split():
    for C in (5, 66, 300):
        for inds, u, move, jb, gamma in fl.ensemble_draws(77, C, 3, 4, {'stretch': 0.5, 'de': 0.5}):
            n0 = (C + 1) // 2
            assert (inds == 0).sum() == n0 and (inds == 1).sum() == C - n0
            nc = np.where(inds == 0, C - n0, n0)
            ja = (np.round(u[:, 1].astype(np.float64) * (1 << 24)).astype(np.int64) * nc) >> 24
            assert np.all(jb != ja) and np.all((jb >= 0) & (jb < nc)) and np.all((u >= 0) & (u < 1))
            assert np.all(np.abs(gamma / fl.de_gamma0(4) - 1.0) < 1e-4)


# ---- the likelihood classes against the table's parameters --------------------------------------------------------------------------
def test_classes_hand_over_the_tables_parameters():
    from nnest_amd import likelihoods as L
    made = {'rosenbrock': L.Rosenbrock(4), 'gaussmix': L.GaussianMix(4), 'himmelblau': L.Himmelblau(4), 'gaussian': L.Gaussian(4, 0.5),
            'eggbox': L.Eggbox(2), 'shell': L.GaussianShell(4, 0.1, 2.0, 0.0),
            'double_shell': L.DoubleGaussianShell(4, sigmas=(0.1, 0.2), rshells=(2.0, 1.5), centers=(-1.0, 1.0))}
    x = np.random.RandomState(0).normal(size=(30, 4))
    for name, like in made.items():
        assert like.hip_like_id == fl.LIKES[name]['id']
        assert tuple(float(v) for v in like.hip_like_params) == tuple(fl.LIKES[name]['params']), name
        xs = x[:, :like.x_dim].astype(np.float32)
        np.testing.assert_allclose(like(xs.astype(np.float64)), fl.exact_logl(name, xs, like.hip_like_params), rtol=1e-12, atol=1e-10)


def test_double_shell_with_a_vector_centre_takes_the_host_route():
    """a sub-shell whose centre has unequal entries is not the kernel's scalar-centre shell: the pair clears its id as the sub-shell
    does; equal entries stay on the device with the scalar they stand for"""
    from nnest_amd.likelihoods import DoubleGaussianShell, GaussianShell
    assert GaussianShell(3, center=[0.0, 1.0, 0.0]).hip_like_id is None
    for centers in (([-4.0, -3.0, -4.0], 4), (-4, [4.0, 4.0, 5.0])):
        assert DoubleGaussianShell(3, centers=centers).hip_like_id is None
    same = DoubleGaussianShell(3, centers=([-4.0, -4.0, -4.0], 4))
    assert same.hip_like_id == fl.LIKES['double_shell']['id']
    assert same.hip_like_params == (0.1, 2, -4.0, 0.1, 2, 4.0) and all(np.isscalar(v) for v in same.hip_like_params)
    assert DoubleGaussianShell(3).hip_like_params == (0.1, 2, -4.0, 0.1, 2, 4.0)
    x = np.random.RandomState(1).normal(size=(5, 3)) * 4.0
    np.testing.assert_allclose(same(x), DoubleGaussianShell(3)(x), rtol=1e-13)
