"""CPU checks for EnsembleSampler.bootstrap: the numpy restatement of emcee's integrated autocorrelation time (direct sums against an
FFT statement of the same definition, the window quirk, the too-short-chain condition), emcee's thinning rule, the argument checks
of the new C entries (no device needed) and of `bootstrap` itself."""
import ctypes

import numpy as np
import pytest

from tests import bootstrap_check as bc


def test_direct_sums_agree_with_fft():
    x = bc.ar1(np.random.RandomState(0), 32, 4000, 1, 0.9)
    tau, win = bc.integrated_time(x)
    tau_f, win_f = bc.integrated_time_fft(x)
    print('tau %r window %r |direct - fft| %g' % (tau, win, np.max(np.abs(tau - tau_f))))
    assert np.array_equal(win, win_f)
    np.testing.assert_allclose(tau, tau_f, rtol=1e-12, atol=0)
    # AR(1) with phi = 0.9: tau = (1 + phi) / (1 - phi) = 19 for an infinite chain; the estimate at its window lies near it
    assert 12 < tau[0] < 26 and 50 * tau[0] <= x.shape[1]
    np.testing.assert_allclose(bc.acf_direct(x[:, :300]), bc.acf_fft(x[:, :300]), atol=1e-12)


def test_window_quirk():
    """an all-true arange(T) < c taus gives window 0 (argmin of an all-true array), not T - 1; an all-false one gives T - 1"""
    assert bc.auto_window(np.full(10, 100.0), 5) == 0
    assert bc.auto_window(np.full(10, -1.0), 5) == 9
    assert bc.auto_window(np.array([1.0, 1.0, 0.1, 0.1, 5.0]), 1) == 1   # (the first false entry, not the last)
    # (with every walker centred on its own mean the lag sums of a walker add up to zero, so taus[T - 1] = 0 and the full table
    # of integrated_time never is all-true: the quirk is a property of the window rule alone)
    x = bc.ar1(np.random.RandomState(1), 4, 50, 2, 0.5)
    np.testing.assert_allclose(2 * np.sum(bc.acf_direct(x), axis=0) - 1, 0, atol=1e-12)


def test_short_chain_raises():
    x = bc.ar1(np.random.RandomState(2), 16, 200, 2, 0.9)
    with pytest.raises(bc.AutocorrError) as e:
        bc.integrated_time(x)
    assert e.value.thresh == 200 / 50 and np.any(50 * e.value.tau > 200)
    tau, _ = bc.integrated_time(x, quiet=True)
    np.testing.assert_array_equal(tau, e.value.tau)


def test_emcee_thin_rule():
    S, N, D = 23, 3, 2
    chain = (np.arange(S)[:, None, None] * 100 + np.arange(N)[None, :, None] * 10 + np.arange(D)[None, None, :]).astype(float)
    out = bc.emcee_thin(chain, discard=5, thin=4)
    steps = [8, 12, 16, 20]   # discard + thin - 1, then every thin-th
    want = np.array([[s * 100 + k * 10 + d for d in range(D)] for s in steps for k in range(N)], float)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(bc.emcee_thin(chain, 0, 1), chain.reshape(-1, D))
    assert len(bc.emcee_thin(chain, 22, 1)) == N and len(bc.emcee_thin(chain, 22, 2)) == 0


def test_new_entries_refuse_bad_arguments():
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG, E_UNSUPPORTED = 1, _lib.NNEST_E_UNSUPPORTED
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)

    def x_steps(like=L, x_in=p, x_out=ctypes.c_void_p(128), lp_out=p, hist_x=p, hist_lp=p, work=p, C=8, D=4, steps=2):
        return lib.nnest_ensemble_x_steps(like, None, None, None, None, x_in, None, x_out, None, lp_out, hist_x, hist_lp, None, work,
                                          C, D, steps, 0, 0, 0, 0.0, None)

    assert x_steps(like=None) == E_ARG
    for name in ('x_in', 'x_out', 'lp_out', 'hist_x', 'hist_lp', 'work'):
        assert x_steps(**{name: None}) == E_ARG, name
        assert b'NULL' in lib.nnest_hip_last_error()
    assert x_steps(x_out=p) == E_ARG   # x_in == x_out
    assert x_steps(D=129, C=300) == E_UNSUPPORTED and b'128' in lib.nnest_hip_last_error()
    assert x_steps(D=0) == E_ARG
    assert x_steps(C=0) == E_ARG and x_steps(C=1) == E_ARG
    assert x_steps(steps=-1) == E_ARG
    bad = _lib.like_spec(99, 1.0)
    assert x_steps(like=ctypes.byref(bad)) == E_ARG and b'likelihood id' in lib.nnest_hip_last_error()
    assert lib.nnest_ensemble_x_max_walkers(129, 3) == -1 and lib.nnest_ensemble_x_max_walkers(4, 99) == -1

    def autocorr(x=p, work=p, f=p, C=4, T=100, D=3, cs=300, ss=3):
        return lib.nnest_chain_autocorr(x, C, T, D, cs, ss, work, f, None)

    for name in ('x', 'work', 'f'):
        assert autocorr(**{name: None}) == E_ARG, name
    assert autocorr(C=0) == E_ARG and autocorr(T=1) == E_ARG and autocorr(D=0) == E_ARG
    assert autocorr(cs=-1) == E_ARG and autocorr(ss=-1) == E_ARG
    assert lib.nnest_chain_autocorr_work_words(0, 100, 3) == -1 and lib.nnest_chain_autocorr_work_words(4, 100, 3) > 0


def _bare_sampler(sample_prior=None):
    from nnest_amd.ensemble import EnsembleSampler
    s = EnsembleSampler.__new__(EnsembleSampler)   # (no flow: the argument checks come first)
    s.x_dim, s.num_derived, s.sample_prior = 4, 0, sample_prior
    return s


@pytest.mark.parametrize('move', ['kde', 'DE', 'snooker'])
def test_bootstrap_refuses_other_moves(move):
    with pytest.raises(NotImplementedError, match=move):
        _bare_sampler().bootstrap(100, 16, moves={move: 1.0})


def test_bootstrap_needs_a_start():
    with pytest.raises(ValueError, match='Prior does not have sample method'):
        _bare_sampler().bootstrap(100, 16)
    with pytest.raises(ValueError, match='Prior does not have sample method'):
        _bare_sampler().bootstrap(100, 16, moves={'Stretch': 1.0})


def test_x_space_run_refuses_fewer_than_two_d_walkers():
    with pytest.raises(RuntimeError, match='fewer walkers than twice the number of dimensions'):
        _bare_sampler()._ensemble_sample_x(10, np.zeros((7, 4)))


def test_identity_flow_and_autocorr_error_exist():
    from nnest_amd.ensemble_rounds import IdentityFlow   # noqa: F401
    from nnest_amd.evaluation import AutocorrError
    e = AutocorrError(np.ones(2), 4.0, 'msg')
    assert e.thresh == 4.0 and e.tau.shape == (2,) and isinstance(e, Exception)
