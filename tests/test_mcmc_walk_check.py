"""CPU checks of the fused random-walk Metropolis run (include/nnest_hip.h nnest_mcmc_steps; tests/mcmc_walk_check.py restates it): the
restated move keeps an exactly sampled target, the invariance statistics reject the move with the log-det's sign flipped (so the GPU
invariance tests can fail), the three entry points are declared, exported and bound within ABI 15 and answer their argument checks
without a device, and the Python layers route to them: HipNVP / HipSpline bind an `mcmc` entry and the other families do not,
Sampler._mcmc_sample_device cuts a run into launches and keeps the reference's books, MCMCSampler.run takes `route` and `seed`."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import test_ensemble_check as ec
from tests.mcmc_walk_check import latent_target, numpy_draws, rw_run, rw_step
from tests.slice_invariance import ALPHA, assert_invariant, min_corrected_p, stationarity_pvalues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_mcmc_steps', 'nnest_spline_mcmc_steps', 'nnest_mcmc_fill_noise')
N, S, STEP = 6000, 40, 0.5


def run_move(flow, seed, logdet_sign=1.0):
    """exact draws of the Gaussian in the box (tests/test_ensemble_check.py), S steps of the restated move through a toy flow"""
    inv, fwd = ec.FLOWS[flow]
    rng = np.random.RandomState(seed)
    z0 = fwd(ec.exact(rng, N)).astype(np.float32)
    lp_fn = latent_target(inv, ec.gauss_logl, ec.in_box, logdet_sign=logdet_sign)
    lp0 = lp_fn(z0)
    assert np.all(np.isfinite(lp0))
    z, _, _, _, n_acc = rw_run(z0, lp0, numpy_draws(rng, N, ec.D, S), STEP, lp_fn)
    assert np.mean(n_acc > 0) >= 0.9
    x, _ = inv(z)
    return stationarity_pvalues(x, ec.exact(rng, N))


@pytest.mark.parametrize('flow', ['identity', 'affine', 'sinh'])
def test_restated_move_keeps_its_target(flow):
    assert_invariant(run_move(flow, 21), what='random-walk Metropolis, %s flow' % flow)


def test_statistics_reject_the_flipped_logdet():
    p = run_move('sinh', 23, logdet_sign=-1.0)
    assert min_corrected_p(p) <= ALPHA, p


def test_step_arithmetic():
    """float32 proposals with both operations rounded, a float64 ratio, u = 0 accepts every finite proposal and none from -inf to -inf"""
    z = np.array([[0.1, -0.2], [1.0, 1.0], [0.0, 0.0]], np.float32)
    eps = np.array([[1.5, -0.25], [0.3, 0.7], [1.0, 1.0]], np.float32)
    lp_fn = lambda q: np.where(np.all(np.abs(q) < 1.05, axis=1), -0.5 * (np.asarray(q, np.float64) ** 2).sum(1), -np.inf)
    rec = {}
    z1, lp1 = rw_step(z, [lp_fn(z[:1])[0], -np.inf, 0.0], eps, np.array([0.5, 0.0, 0.999], np.float32), 0.1, lp_fn, record=rec)
    assert rec['q'].dtype == np.float32
    assert np.array_equal(rec['q'], z + (np.float32(0.1) * eps).astype(np.float32))
    assert rec['accept'].tolist() == [True, False, False]   # downhill within log 0.5; -inf -> -inf: NaN, refused; downhill past log u
    assert np.array_equal(z1[1:], z[1:]) and np.array_equal(z1[0], rec['q'][0]) and lp1[0] == rec['lp_q'][0] and lp1[1] == -np.inf


def test_restated_draws():
    """the numpy Philox4x32-10 of the checker against the oracle's; the streams' structure: 24-bit uniforms, unit normals, a walker's
    draws depend on its global index alone"""
    from oracle import oracle as orc
    from tests.mcmc_walk_check import mcmc_draws, philox4x32_10
    rng = np.random.RandomState(3)
    for _ in range(20):
        ctr = [int(v) for v in rng.randint(0, 1 << 32, size=4, dtype=np.uint64)]
        seed = int(rng.randint(0, 1 << 62, dtype=np.uint64))
        assert philox4x32_10(np.array(ctr, np.uint64), seed).tolist() == orc.philox4x32_10(ctr, [seed & 0xffffffff, seed >> 32])
    eps, u = mcmc_draws(11, 1000, 3000, 3, 2, 7)
    assert eps.shape == (2, 3000, 7) and u.shape == (2, 3000) and eps.dtype == np.float32 and u.dtype == np.float32
    assert np.all(u * (1 << 24) == np.floor(u * (1 << 24))) and u.min() >= 0.0 and u.max() < 1.0
    assert abs(eps.mean()) < 0.03 and abs(eps.std() - 1.0) < 0.03 and abs(u.mean() - 0.5) < 0.02
    shard_eps, shard_u = mcmc_draws(11, 1024, 100, 4, 1, 7)   # walkers 1024 .. of step 4: rows 24 .. of the run above, its second step
    assert np.array_equal(shard_eps[0], eps[1, 24:124]) and np.array_equal(shard_u[0], u[1, 24:124])
    assert np.array_equal(mcmc_draws(11, 1000, 10, 3, 1, 5)[0], eps[:1, :10, :5])   # a narrower run shares the blocks


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(nnest_[a-z0-9_]+)\s*\(', text))


def test_header_declares_and_library_exports_the_entries():
    from nnest_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert _lib.SIGNATURES['nnest_spline_mcmc_steps'] == _lib.SIGNATURES['nnest_mcmc_steps']   # one argument list
    assert lib.nnest_hip_version() == 15


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)
    for fn in (lib.nnest_mcmc_steps, lib.nnest_spline_mcmc_steps):
        def steps(h=None, like=L, t_std=p, t_mean=p, lo=None, hi=None, z_in=p, lp_in=None, logl_in=None, z_out=p, x_out=p, lp_out=p,
                  logl_out=p, hist_z=p, hist_x=p, hist_logl=p, C=8, S=2, step=0.5):
            return fn(h, like, t_std, t_mean, lo, hi, z_in, lp_in, logl_in, z_out, x_out, lp_out, logl_out, hist_z, hist_x, hist_logl,
                      None, C, S, ctypes.c_float(step), 0, 0, 0, None)

        assert steps() == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()
        assert steps(hist_z=None, hist_x=None, hist_logl=None) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (optional)
        assert steps(S=0, z_out=None) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (steps = 0 writes no z_out)
        assert steps(C=1) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (any C >= 1)
        assert steps(like=None) == E_ARG and b'NULL' in lib.nnest_hip_last_error()
        for name in ('z_in', 'z_out', 'x_out', 'lp_out', 'logl_out'):
            assert steps(**{name: None}) == E_ARG, name
            assert b'NULL device buffer' in lib.nnest_hip_last_error(), name
        for name in ('t_std', 't_mean', 'lo', 'lp_in', 'logl_in'):
            assert steps(**{name: None if name.startswith('t_') else p}) == E_ARG, name
            assert b'both or neither' in lib.nnest_hip_last_error(), name
        assert steps(hist_x=None) == E_ARG and b'all or none' in lib.nnest_hip_last_error()
        assert steps(S=-1) == E_ARG and b'steps=-1' in lib.nnest_hip_last_error()
        assert steps(C=0) == E_ARG and b'C=0' in lib.nnest_hip_last_error()
        assert steps(step=float('nan')) == E_ARG and b'step_size' in lib.nnest_hip_last_error()
        bad = _lib.like_spec(99, 1.0)
        assert steps(like=ctypes.byref(bad)) == E_ARG and b'likelihood id' in lib.nnest_hip_last_error()
    assert lib.nnest_mcmc_fill_noise(p, p, 2, 8, 0, 0, 0, 0, None) == E_ARG and b'D=0' in lib.nnest_hip_last_error()
    assert lib.nnest_mcmc_fill_noise(p, p, -1, 8, 3, 0, 0, 0, None) == E_ARG


def bound(cls, family, **named):
    """an instance of the flow class with its C symbols bound as its constructor binds them, without a handle (no GPU)"""
    from nnest_amd import _lib
    o = object.__new__(cls)
    o._lib = _lib.load()
    o._h = None
    o._bind(family, **named)
    return o


def test_one_body_bound_per_family():
    from nnest_amd import _lib, flow
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.flow import _HipFlow, HipNVP
    from nnest_amd.maf import HipMAF
    from nnest_amd.spline import HipSpline
    lib = _lib.load()
    for cls in (HipNVP, HipSpline):
        assert 'mcmc_steps' not in cls.__dict__ and cls.mcmc_steps is _HipFlow.mcmc_steps   # one body
    assert "mcmc='nnest_mcmc_steps'" in inspect.getsource(HipNVP.__init__)
    assert "mcmc='nnest_spline_mcmc_steps'" in inspect.getsource(HipSpline.__init__)
    assert bound(HipSpline, 'nnest_spline', mcmc='nnest_spline_mcmc_steps')._sym['mcmc'] is lib.nnest_spline_mcmc_steps
    assert bound(HipNVP, 'nnest_nvp', mcmc='nnest_mcmc_steps')._sym['mcmc'] is lib.nnest_mcmc_steps
    assert callable(flow.mcmc_fill_noise)
    # a family that binds no `mcmc` symbol cannot reach another family's entry point
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        assert 'mcmc' not in inspect.getsource(cls.__init__)
        o = bound(cls, family)
        o.device = 'cpu'
        assert 'mcmc' not in o._sym
        with pytest.raises(NotImplementedError):
            o.mcmc_steps(3, None, 2, 0.5)


def test_run_takes_route_and_seed_and_the_transform_is_the_base_class():
    from nnest_amd.ensemble import EnsembleSampler
    from nnest_amd.mcmc import MCMCSampler
    from nnest_amd.sampler import Sampler
    par = inspect.signature(MCMCSampler.run).parameters
    for name in ('route', 'seed'):
        assert name in par and par[name].default is None, name
    assert '_install_transform' in Sampler.__dict__ and '_mcmc_sample_device' in Sampler.__dict__
    assert EnsembleSampler._install_transform is Sampler._install_transform and MCMCSampler._install_transform is Sampler._install_transform
    s = EnsembleSampler.__new__(EnsembleSampler)
    mean, std = np.array([1.0, -2.0]), np.array([0.5, 2.0])
    s._install_transform(mean, std)
    np.testing.assert_array_equal(s.transform(np.array([[2.0, 1.0]])), [[2.0, 0.0]])
    np.testing.assert_array_equal(s._ensemble_transform[0], std)
    np.testing.assert_array_equal(s._ensemble_transform[1], mean)
    assert s._linear_scale is None and s._fused_like_id is None


class _StubFlow(object):
    """what _mcmc_sample_device asks of the flow, recorded: every launch moves every walker by +1 per step; the first `bad_starts`
    base draws have one chain outside the prior"""
    device = 'cpu'

    def __init__(self, D, bad_starts=0):
        self._sym = {'mcmc': object()}
        self.D, self.calls, self.bad_starts, self.draws = D, [], bad_starts, 0

    def forward(self, x):
        import torch
        return torch.as_tensor(np.asarray(x, np.float32)), None

    def prior_sample(self, n):
        import torch
        self.draws += 1
        return torch.full((n, self.D), float(self.draws))

    def mcmc_steps(self, like_id, z, steps, step_size, lp=None, logl=None, step0=0, **kw):
        import torch
        C = z.shape[0]
        self.calls.append((like_id, C, steps, step0, lp is not None, kw['seed']))
        if steps == 0:
            lp0 = torch.zeros(C, dtype=torch.float64)
            if self.draws and self.draws <= self.bad_starts:
                lp0[0] = -np.inf
            return dict(z=z, x=z * 2, lp=lp0, logl=torch.full((C,), 7.0, dtype=torch.float64), hist_z=None, hist_x=None, hist_logl=None,
                        n_accept=torch.zeros(C, dtype=torch.int32))
        t = torch.arange(1, steps + 1, dtype=torch.float32)
        hz = z[:, None, :] + t[None, :, None]
        return dict(z=hz[:, -1].contiguous(), x=2 * hz[:, -1], lp=lp - steps, logl=logl + steps, hist_z=hz, hist_x=2 * hz,
                    hist_logl=logl[:, None] + t[None, :].double(), n_accept=torch.full((C,), steps, dtype=torch.int32))


class _StubTrainer(object):
    def __init__(self, net):
        self.netG = net


def _bare_sampler(D, net, agrees=True):
    from nnest_amd.mcmc import MCMCSampler

    class _Like(object):
        hip_like_id, hip_like_params = 3, (0.5,)

    s = MCMCSampler.__new__(MCMCSampler)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = D, 0, 0, _StubTrainer(net)
    s.total_calls = s.total_accepted = s.total_rejected = 0
    s.chain_stats, s._user_loglike = False, _Like()
    s.transform = lambda x: x
    s._ensemble_affine = lambda: (np.ones(D), np.zeros(D))
    s._user_prior, s._transform_prior = None, True
    s._probe_agrees = lambda like_id, params, **kw: agrees   # (the one step of _device_target that needs a device)
    saved = []
    s._save_samples = lambda samples, loglikes, derived_samples=None: saved.append((samples.shape, loglikes.shape, derived_samples.shape))
    return s, saved


def test_device_run_cuts_launches_and_keeps_the_books():
    D, Nc, steps = 3, 8, 7
    net = _StubFlow(D)
    s, saved = _bare_sampler(D, net)
    x0 = np.zeros((Nc, D))
    samples, latent, derived, loglikes, scale, ncall = s._mcmc_sample_device(steps, init_samples=x0, seed=5, chunk_steps=3, output_interval=2)
    # the start is a steps = 0 launch; the run is cut by chunk_steps and by output_interval, lp / logl handed from launch to launch
    assert net.calls == [(3, Nc, 0, 0, False, 5), (3, Nc, 2, 0, True, 5), (3, Nc, 2, 2, True, 5), (3, Nc, 2, 4, True, 5), (3, Nc, 1, 6, True, 5)]
    assert samples.shape == (Nc, steps + 1, D) and latent.shape == (Nc, steps + 1, D) and loglikes.shape == (Nc, steps + 1)
    assert derived.shape == (Nc, steps + 1, 0)
    np.testing.assert_array_equal(latent[0, :, 0], np.arange(steps + 1))
    np.testing.assert_array_equal(samples, 2 * latent)
    np.testing.assert_array_equal(loglikes[0], 7.0 + np.arange(steps + 1))
    assert scale == pytest.approx(2 / np.sqrt(D)) and ncall == Nc * (1 + steps) and s.total_calls == ncall
    assert s.total_accepted == Nc * steps and s.total_rejected == 0
    assert [sh[0] for sh in saved] == [(Nc * 3, D), (Nc * 5, D), (Nc * 7, D)]
    # without init_samples: base draws, the whole batch redrawn while a chain starts outside, counted as calls
    net = _StubFlow(D, bad_starts=2)
    s, _ = _bare_sampler(D, net)
    out = s._mcmc_sample_device(4, num_chains=Nc, seed=6)
    assert net.draws == 3 and out[5] == Nc * (3 + 4) and s.total_calls == Nc * 7
    np.testing.assert_array_equal(out[1][:, 0], 3.0)
    net = _StubFlow(D, bad_starts=100)
    s, _ = _bare_sampler(D, net)
    with pytest.raises(Exception, match='Could not find starting value'):
        s._mcmc_sample_device(4, num_chains=Nc, seed=6, max_start_tries=5)
    assert net.draws == 5


def test_device_run_names_what_it_does_not_take():
    D = 3
    for change, word in ((dict(num_derived=1), 'derived'), (dict(num_slow=1), 'fast/slow'), (dict(_user_loglike=lambda x: x), 'Python callable')):
        s, _ = _bare_sampler(D, _StubFlow(D))
        for k, v in change.items():
            setattr(s, k, v)
        with pytest.raises(ValueError, match=word):
            s._mcmc_sample_device(2, init_samples=np.zeros((4, D)))
    net = _StubFlow(D)
    del net._sym['mcmc']
    s, _ = _bare_sampler(D, net)
    with pytest.raises(ValueError, match='_StubFlow'):
        s._mcmc_sample_device(2, init_samples=np.zeros((4, D)))
    s, _ = _bare_sampler(D, _StubFlow(D), agrees=False)
    with pytest.raises(ValueError, match='prior'):
        s._mcmc_sample_device(2, init_samples=np.zeros((4, D)))
