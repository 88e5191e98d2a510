"""CPU checks of the ensemble sampler's move mixtures (tests/ensemble_moves_check.py restates nnest_ensemble_moves_steps): the
restated differential-evolution move and its mixture with the stretch move keep an exactly sampled target, the invariance
statistics reject two wrong DE moves (so the GPU invariance tests can fail), the new C entries exist and check their arguments
without a device, the `moves` dict is parsed as the reference's, and the front end chooses its route on stub flows."""
import ctypes
import inspect

import numpy as np
import pytest

from tests.ensemble_check import latent_target
from tests.ensemble_moves_check import moves_run, numpy_moves_draws
from tests.slice_invariance import ALPHA, assert_invariant, min_corrected_p, stationarity_pvalues
from tests.test_ensemble_check import D, FLOWS, N, S, exact, gauss_logl, in_box
from tests.test_spline_ensemble_abi import _StubSpline, _bare_sampler, declared_symbols

NEW = ('nnest_ensemble_moves_threshold', 'nnest_ensemble_moves_steps', 'nnest_ensemble_x_moves_steps', 'nnest_ensemble_moves_max_walkers',
       'nnest_ensemble_x_moves_max_walkers', 'nnest_ensemble_rounds_moves_propose', 'nnest_ensemble_rounds_moves_accept',
       'nnest_ensemble_fill_moves')
E_ARG = 1


def run_moves(flow, seed, p_stretch, wrong=None):
    inv, fwd = FLOWS[flow]
    rng = np.random.RandomState(seed)
    x0 = exact(rng, N)
    z0 = fwd(x0).astype(np.float32)
    lp_fn = latent_target(inv, gauss_logl, in_box)
    lp0 = lp_fn(z0)
    assert np.all(np.isfinite(lp0))
    z, _, moved = moves_run(z0, lp0, numpy_moves_draws(rng, N, S, D, p_stretch), lp_fn, wrong=wrong)
    assert moved.mean() >= 0.9   # (a frozen chain is trivially invariant)
    x, _ = inv(z)
    return stationarity_pvalues(x, exact(rng, N))


@pytest.mark.parametrize('p_stretch', [0.0, 0.5])
@pytest.mark.parametrize('flow', ['identity', 'affine', 'sinh'])
def test_restated_moves_keep_their_target(flow, p_stretch):
    assert_invariant(run_moves(flow, 21, p_stretch), what='DE move (p_stretch %g), %s flow' % (p_stretch, flow))


def test_statistics_reject_the_asymmetric_pull():
    p = run_moves('identity', 22, 0.0, wrong='pull')
    assert min_corrected_p(p) <= ALPHA, p


def test_statistics_reject_a_spurious_factor():
    p = run_moves('identity', 23, 0.0, wrong='factor')
    assert min_corrected_p(p) <= ALPHA, p


def test_header_declares_and_library_exports_the_entries():
    from nnest_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s), s
    for old, new in (('nnest_ensemble_steps', 'nnest_ensemble_moves_steps'), ('nnest_ensemble_x_steps', 'nnest_ensemble_x_moves_steps'),
                     ('nnest_ensemble_rounds_propose', 'nnest_ensemble_rounds_moves_propose'),
                     ('nnest_ensemble_rounds_accept', 'nnest_ensemble_rounds_moves_accept'),
                     ('nnest_ensemble_max_walkers', 'nnest_ensemble_moves_max_walkers'),
                     ('nnest_ensemble_x_max_walkers', 'nnest_ensemble_x_moves_max_walkers')):
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old] + [ctypes.c_void_p], new   # one trailing `moves`
    assert lib.nnest_hip_version() == 15
    assert ctypes.sizeof(_lib.EnsMoves) == 16


def test_threshold_from_the_weights():
    from nnest_amd import _lib
    lib = _lib.load()
    thr = lambda ws, wd: lib.nnest_ensemble_moves_threshold(ctypes.byref(_lib.EnsMoves(ws, wd, 0.0, 0.0)))
    assert thr(1, 0) == 1 << 24 and thr(0, 1) == 0 and thr(1, 3) == 1 << 22
    assert thr(2, 2) == 1 << 23 and thr(0.5, 0) == 1 << 24
    assert lib.nnest_ensemble_moves_threshold(None) == 1 << 24   # NULL: the stretch move alone
    assert thr(1, 3) == lib.nnest_ensemble_moves_threshold(ctypes.byref(_lib.ens_moves({'Stretch': 2.0, 'DE': 6.0})))


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = ctypes.byref(_lib.like_spec(3, 1.0, (0.5,)))
    nan = float('nan')
    bad = {'negative': (-1.0, 1.0, 0, 0), 'both 0': (0.0, 0.0, 0, 0), 'NaN': (nan, 1.0, 0, 0), 'NaN de': (1.0, nan, 0, 0),
           'inf': (float('inf'), 1.0, 0, 0), 'negative gamma0': (1.0, 1.0, -1.0, 0)}

    def x_steps(mv, C=8, work=p, x_out=ctypes.c_void_p(128)):
        return lib.nnest_ensemble_x_moves_steps(lk, None, None, None, None, p, None, x_out, None, p, p, p, None, work, C, 3, 2, 0, 0, 0, 0.0, None,
                                                mv)

    def propose(mv, C=8, work=p):
        return lib.nnest_ensemble_rounds_moves_propose(work, C, 2, 3, 0, 0, 0, 0, p, p, None, mv)

    def accept(mv, C=8, work=p):
        return lib.nnest_ensemble_rounds_moves_accept(work, C, 2, 3, 0, 0, 0, 0, p, p, p, p, None, None, None, None, None, p, p, p, p, p, p, None,
                                                      None, 0, 0.0, None, mv)

    def fill(mv, C=8, work=p):
        return lib.nnest_ensemble_fill_moves(work, p, p, p, C, 3, 2, 0, 0, mv, None)

    for name, w in bad.items():
        mv = ctypes.byref(_lib.EnsMoves(*w))
        for fn in (x_steps, propose, accept, fill):
            assert fn(mv) == E_ARG, (name, fn.__name__)
            assert b'ensemble moves' in lib.nnest_hip_last_error(), (name, fn.__name__)
        assert lib.nnest_ensemble_moves_threshold(mv) == -1, name
        assert lib.nnest_ensemble_x_moves_max_walkers(3, 3, mv) == -1, name
    de = ctypes.byref(_lib.EnsMoves(0.5, 0.5, 0.0, 0.0))
    for fn in (x_steps, propose, accept, fill):
        assert fn(de, C=3) == E_ARG and b'C >= 4' in lib.nnest_hip_last_error(), fn.__name__   # two partners in either set
        assert fn(de, work=None) == E_ARG and b'NULL' in lib.nnest_hip_last_error(), fn.__name__
    assert x_steps(de, x_out=p) == E_ARG and b'x_in_dev' in lib.nnest_hip_last_error()
    # the stretch move alone keeps C = 2 and 3 (refused for another reason, or not at all, but not for the moves)
    one = ctypes.byref(_lib.EnsMoves(1.0, 0.0, 0.0, 0.0))
    assert propose(one, C=3, work=None) == E_ARG and b'NULL device buffer' in lib.nnest_hip_last_error()
    assert propose(None, C=3, work=None) == E_ARG and b'NULL device buffer' in lib.nnest_hip_last_error()
    assert lib.nnest_ensemble_moves_steps(None, lk, p, p, None, None, p, None, p, p, p, p, p, p, None, p, 8, 2, 0, 0, 0, 0.0, None, de) == E_ARG
    assert b'NULL handle' in lib.nnest_hip_last_error()
    assert lib.nnest_ensemble_moves_max_walkers(None, 3, de) == -1


def test_the_moves_dict_is_parsed_as_the_reference_s():
    from nnest_amd import _lib
    mv = _lib.ens_moves({'De': 1.0})
    assert isinstance(mv, _lib.EnsMoves) and mv.w_de == 1.0 and mv.w_stretch == 0.0 and _lib.ens_moves_mix(mv)
    mv = _lib.ens_moves({'STRETCH': 0.25, 'de': 0.75})
    assert (mv.w_stretch, mv.w_de, mv.de_gamma0, mv.de_sigma) == (0.25, 0.75, 0.0, 0.0)
    assert _lib.ens_moves(None) is None and _lib.ens_moves(mv) is mv
    assert not _lib.ens_moves_mix(None) and not _lib.ens_moves_mix(_lib.ens_moves({'stretch': 1}))
    for name in ('kde', 'snooker', 'KDE', 'Snooker'):
        with pytest.raises(NotImplementedError, match=name):
            _lib.ens_moves({'stretch': 1.0, name: 1.0})
    with pytest.raises(ValueError, match='foo'):
        _lib.ens_moves({'foo': 1.0})
    for w in ({'de': -1.0}, {'de': 0.0, 'stretch': 0.0}, {}, {'de': float('nan')}, {'stretch': float('inf')}):
        with pytest.raises(ValueError):
            _lib.ens_moves(w)
    with pytest.raises(ValueError, match='at least 4 walkers'):
        _lib.ens_moves_mix(_lib.ens_moves({'de': 1}), 3)


class _StubNVP(_StubSpline):
    """a family that binds the `ensemble_moves` entry too, with a smaller population for it, and runs fused by default"""
    ensemble_fused_by_default = True

    def __init__(self, D, cap=1 << 12, cap_moves=64):
        super(_StubNVP, self).__init__(D, cap)
        self._sym.update(ensemble_moves=object(), ensemble_moves_max_walkers=object())
        self.cap_moves, self.moves = cap_moves, []

    def ensemble_max_walkers(self, like_id, moves=None):
        return self.cap if moves is None else self.cap_moves

    def ensemble_steps(self, like_id, z, steps, **kw):
        self.moves.append(kw.get('moves'))
        return super(_StubNVP, self).ensemble_steps(like_id, z, steps, **kw)


def test_route_choice_with_moves(monkeypatch):
    from nnest_amd import _lib
    D_, N_, S_ = 3, 16, 5
    mix = {'stretch': 0.5, 'DE': 0.5}
    # the spline flow (an `ensemble` entry, no `ensemble_moves`): rounds with a DE step, and 'fused' is refused
    net = _StubSpline(D_)
    s, rounds = _bare_sampler(D_, net, monkeypatch)
    out = s._ensemble_sample(S_, N_, seed=1, moves=mix)
    assert s.ensemble_route == 'rounds' and rounds == [(N_, S_)] and net.calls == [] and out[0].shape == (N_, S_, D_)
    with pytest.raises(ValueError, match='fused route'):
        s._ensemble_sample(S_, N_, seed=1, moves=mix, route='fused')
    s._ensemble_sample(S_, N_, seed=1, moves={'stretch': 1.0}, route='fused')   # the stretch move alone: as without `moves`
    assert s.ensemble_route == 'fused' and len(net.calls) == 1
    # the NVP: fused where the population fits the kernel that knows the move, rounds beyond
    nvp = _StubNVP(D_, cap_moves=N_)
    s, rounds = _bare_sampler(D_, nvp, monkeypatch)
    s._ensemble_sample(S_, N_, seed=1, moves=mix, chunk_steps=3)
    assert s.ensemble_route == 'fused' and rounds == [] and len(nvp.moves) == 2
    assert all(isinstance(m, _lib.EnsMoves) and m.w_de == 0.5 for m in nvp.moves)
    s._ensemble_sample(S_, N_, seed=1)
    assert nvp.moves[-1] is None and s.ensemble_route == 'fused'   # moves=None: the call of today
    nvp.cap_moves = N_ - 1
    s._ensemble_sample(S_, N_, seed=1, moves=mix)
    assert s.ensemble_route == 'rounds' and rounds == [(N_, S_)]
    with pytest.raises(ValueError, match='fused route'):
        s._ensemble_sample(S_, N_, seed=1, moves=mix, route='fused')
    s._ensemble_sample(S_, N_, seed=1, moves={'stretch': 2.0})   # no DE step: the stretch kernel's population
    assert s.ensemble_route == 'fused'
    # refusals come before anything runs
    for name in ('kde', 'snooker'):
        with pytest.raises(NotImplementedError, match=name):
            s._ensemble_sample(S_, N_, seed=1, moves={name: 1.0})
    with pytest.raises(ValueError, match='foo'):
        s._ensemble_sample(S_, N_, seed=1, moves={'foo': 1.0})
    s1, _ = _bare_sampler(1, _StubNVP(1), monkeypatch)
    with pytest.raises(ValueError, match='at least 4 walkers'):
        s1._ensemble_sample(S_, 3, seed=1, moves={'de': 1.0})


def test_front_end_signatures():
    from nnest_amd import ensemble_rounds, flow
    from nnest_amd.ensemble import EnsembleSampler
    from nnest_amd.sampler import Sampler
    for fn, name in ((EnsembleSampler.run, 'moves'), (EnsembleSampler.bootstrap, 'latent_moves'), (Sampler._ensemble_sample_x, 'moves'),
                     (Sampler._ensemble_sample, 'moves'), (flow._HipFlow.ensemble_steps, 'moves'), (flow.ensemble_x_steps, 'moves'),
                     (ensemble_rounds.ensemble_rounds, 'moves'), (ensemble_rounds.fill_moves, 'moves')):
        par = inspect.signature(fn).parameters
        assert name in par and par[name].default is None, fn.__name__
    assert 'moves=latent_moves' in inspect.getsource(EnsembleSampler.bootstrap)
    assert 'not in the reference' in inspect.getdoc(EnsembleSampler.run)
    s = EnsembleSampler.__new__(EnsembleSampler)
    with pytest.raises(NotImplementedError, match='snooker'):   # (refused before the x-space run)
        s.bootstrap(10, 8, latent_moves={'snooker': 1.0})
