"""CPU checks of the checker of tests/test_gpu_slice_likes.py (tests/slice_like_check.py) and of oracle.slice_sample's like_params: the
oracle alone on a seeded random orc.NVP(D, 16, 3, 1) (weights N(0, 0.15^2)) with numpy normal directions.
- the tables reach every instantiation they claim;
- the cap condition: for every solo case and three direction seeds, near_share <= 0.2 -- the share of walkers on which a correct
  kernel may differ from the oracle stays within what the 80 % criterion allows;
- planted faults: oracle.slice_sample runs a second time as a stand-in kernel, its likelihood the float64 function of the float32
  like_scale x (what a correct kernel computes, to rounding), then wrong in one way each; `compare` with the own-x logL check passes
  the right one and fails every wrong one;
- like_params=None returns the arrays recorded before the argument existed, bit for bit (tests/golden/slice_sample_rosen_d4.npz)."""
import contextlib
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fused_like_check as fl
from tests import slice_like_check as sl

G = os.path.join(os.path.dirname(__file__), 'golden')
SEED, OFF = 4242, 100
BY_ID = {sl.case_id(c): c for c in sl.SOLO_TABLE + sl.SOLO_EXTRA}


def random_flow(D):
    n = orc.NVP(D, 16, 3, 1).n
    return orc.NVP(D, 16, 3, 1, (np.random.RandomState(D).normal(size=n) * 0.15).astype(np.float32))


_RUNS = {}


def oracle_run(c, dz_seed=0, params=None):
    """(flow, z0, l0, star, dz, oracle result, margins) of a case on directions of seed dz_seed; computed once, never changed"""
    key = (c, dz_seed, params)
    if key not in _RUNS:
        o = random_flow(c.D)
        z0, l0, star = sl.start(c, lambda u: o.forward(u.astype(np.float32))[0])
        C = len(l0)
        dz = np.random.RandomState(100 + dz_seed).standard_normal((c.S, C, c.D)).astype(np.float32)
        margins = np.empty((c.S, C))
        p = c.params if params is None else params
        ref = orc.slice_sample(o, c.name, c.scale, z0, l0, star, 2.0 / np.sqrt(c.D), dz, SEED, walker_offset=OFF, margins=margins,
                               like_params=list(p) if p else None)
        _RUNS[key] = (o, z0, l0, star, dz, ref, margins)
    return _RUNS[key]


FAULTS = ('params', 'scale', 'last_dim', 'rosen', 'finite')


@contextlib.contextmanager
def kernel_likelihood(fault=None):
    """oracle.loglike replaced, for the stand-in kernel's run, by what a kernel computes: the float64 likelihood of the float32
    like_scale x with the safe rule -- or that with one planted fault: 'params' zeroed; 'scale' off by 1e-3 relative; 'last_dim' left
    out of the sum (Himmelblau: the last pair); 'rosen': Rosenbrock's terms whatever was asked for; 'finite': a non-finite logL
    mapped to 0 and not to -1e100"""
    real = orc.loglike

    def like(name, x, scale, params=None):
        p = list(params) if params else None
        if fault == 'params':
            p = [0.0] * len(p)
        if fault == 'scale':
            scale = scale * (1.0 + 1e-3)
        if fault == 'rosen':
            name, p = 'rosenbrock', None
        tx = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)
        if fault == 'last_dim':
            tx = tx[:, :-2] if name == 'himmelblau' else tx[:, :-1]
        with np.errstate(all='ignore'):
            out = np.asarray(real(name, tx, 1.0, p), np.float64)
        mapped = ~np.isfinite(out) | (out == fl.SAFE)   # (the oracle applies the safe rule itself where its C code evaluates)
        return np.where(mapped, 0.0 if fault == 'finite' else fl.SAFE, out)

    orc.loglike = like
    try:
        yield
    finally:
        orc.loglike = real


def stand_in(c, fault, params=None):
    o, z0, l0, star, dz, ref, margins = oracle_run(c, params=params)
    p = c.params if params is None else params
    with kernel_likelihood(fault):
        r = orc.slice_sample(o, c.name, c.scale, z0, l0, star, 2.0 / np.sqrt(c.D), dz, SEED, walker_offset=OFF,
                             like_params=list(p) if p else None)
    return r


def held(c, r, what):
    """what the GPU test asserts of a kernel's output, in its order"""
    o, z0, l0, star, dz, ref, margins = oracle_run(c)
    assert sl.near_share(margins) <= 1.0 - sl.AGREE
    k = sl.as_kernel(r)
    sl.compare(k, ref, margins, what=what)
    sl.check_logl_of_own_x(c, r['logl'], k['x'], r['n_move'], l0, what=what)
    sl.check_in_box_above_star(k, r['logl'], star, what=what)


def test_tables_reach_every_instantiation():
    rosen = {fl.units(c.D) for c in sl.SOLO_TABLE if c.name == 'rosenbrock'}
    other = {fl.units(c.D) for c in sl.SOLO_TABLE if c.name != 'rosenbrock'}
    assert rosen == {3, 4} and other == {1, 2, 3, 4}   # (Rosenbrock at U = 1, 2 and 4: tests/test_gpu_slice.py)
    assert {c.name for c in sl.SOLO_TABLE} == set(fl.LIKES)
    for c in sl.SOLO_TABLE:
        assert c.params == tuple(fl.LIKES[c.name]['params']) and fl.LIKES[c.name]['dims'](c.D) and c.S in (3, 4)
    assert {sl.lk(c.name) for c in sl.SOLO_TABLE} == {0, -1}
    assert [(c.name, fl.units(c.D)) for c in sl.SOLO_EXTRA] == [('rosenbrock', 1), ('rosenbrock', 2)]
    assert [fl.units(D) for D in sl.SAFE_SOLO_DIMS] == [1, 3]
    assert [(c.scale, c.D) for c in sl.SOLO_TABLE if c.name == 'shell'] == [(2.5, 5), (1.0, 40)]
    assert [(c.scale, c.D) for c in sl.SOLO_TABLE if c.name == 'double_shell'] == [(2.5, 5), (1.0, 97)]


@pytest.mark.parametrize('cid', sorted(BY_ID))
def test_cap_condition_holds_for_the_solo_table(cid):
    c = BY_ID[cid]
    shares = [sl.near_share(oracle_run(c, s)[6]) for s in range(3)]
    print('NEAR %-18s S %d  %s' % (cid, c.S, '  '.join('%.3f' % v for v in shares)))
    assert max(shares) <= 1.0 - sl.AGREE, (cid, shares)
    o, z0, l0, star, dz, ref, margins = oracle_run(c)
    assert len(l0) % 4 != 0 and np.all(l0 > star)
    assert ref['n_move'].mean() > 0.9 * c.S   # (the walk is a walk: nearly every update moves)


def test_near_share_counts_walkers_not_updates():
    m = np.full((3, 10), 1.0)
    m[0, 2] = m[2, 2] = 1e-5
    m[1, 7] = 1.9e-4
    m[1, 8] = 2e-4   # (not below)
    assert sl.near_share(m) == 0.2


@pytest.mark.parametrize('cid', sorted(BY_ID))
def test_the_right_likelihood_passes(cid):
    c = BY_ID[cid]
    held(c, stand_in(c, None), cid)


PLANTED = ([(f, cid) for f, ids in (('params', ('gaussian-d7', 'shell-d40', 'double_shell-d5')),
                                    ('last_dim', ('rosenbrock-d65', 'gaussmix-d20', 'himmelblau-d66', 'gaussian-d100', 'shell-d5',
                                                  'double_shell-d97')),
                                    ('rosen', ('gaussmix-d81', 'himmelblau-d2', 'gaussian-d7', 'eggbox-d2', 'shell-d40')))
            for cid in ids] + [('scale', cid) for cid in sorted(BY_ID)])


@pytest.mark.parametrize('fault,cid', PLANTED, ids=['%s-%s' % p for p in PLANTED])
def test_a_planted_fault_fails(fault, cid):
    c = BY_ID[cid]
    r = stand_in(c, fault)
    with pytest.raises(AssertionError):
        held(c, r, '%s with %s wrong' % (cid, fault))


@pytest.mark.parametrize('D', sl.SAFE_SOLO_DIMS)
def test_the_safe_rule_check_passes_the_rule_and_fails_a_finite_value(D):
    """shell with a NaN width from a start with finite logl: under the safe rule nothing moves; a kernel that maps the non-finite logL
    to a finite value walks, and the check fails it"""
    c = sl.case('shell', D)
    o, z0, l0, star, dz, ref, margins = oracle_run(c, params=sl.NAN_PARAMS)
    assert np.all(np.isfinite(l0)) and np.all(ref['n_move'] == 0)
    good = stand_in(c, None, params=sl.NAN_PARAMS)
    sl.check_nothing_moves(sl.as_kernel(good), ref, z0, l0, good['z'], good['logl'], what='safe')
    bad = stand_in(c, 'finite', params=sl.NAN_PARAMS)
    assert bad['n_move'].sum() > 0
    with pytest.raises(AssertionError):
        sl.check_nothing_moves(sl.as_kernel(bad), ref, z0, l0, bad['z'], bad['logl'], what='finite')


def test_like_params_reach_the_likelihood():
    """the oracle's own use of the new argument: the Gaussian's correlation changes the chain, and None is the parameterless call"""
    c = BY_ID['gaussian-d7']
    o, z0, l0, star, dz, ref, margins = oracle_run(c)
    other = orc.slice_sample(o, c.name, c.scale, z0, l0, star, 2.0 / np.sqrt(c.D), dz, SEED, walker_offset=OFF, like_params=[0.0])
    assert not np.array_equal(other['logl'], ref['logl'])
    np.testing.assert_array_equal(ref['logl'], orc.loglike(c.name, ref['x'][:, -1], c.scale, list(c.params)))


def test_like_params_none_returns_the_recorded_arrays():
    g = np.load(os.path.join(G, 'slice_sample_rosen_d4.npz'))
    D = g['z0'].shape[1]
    nvp = orc.NVP(D, 16, 3, 1, g['w'])
    for kw in ({}, dict(like_params=None)):
        margins = np.empty_like(g['margins'])
        a = orc.slice_sample(nvp, 'rosenbrock', 5.0, g['z0'], g['l0'], float(g['star']), float(g['width']), g['dz'], int(g['seed']),
                             walker_offset=int(g['walker_offset']), margins=margins, **kw)
        assert set(a) == {k[4:] for k in g.files if k.startswith('out_')}
        for k, v in a.items():
            want = g['out_' + k]
            assert v.dtype == want.dtype and v.shape == want.shape, k
            assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), k
        assert np.array_equal(margins.view(np.uint8), g['margins'].view(np.uint8))
