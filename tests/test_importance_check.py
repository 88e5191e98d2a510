"""CPU checks of the importance-sampled evidence (include/nnest_hip.h nnest_importance_evidence; tests/importance_check.py restates it):
the restated sums, merge and result against scipy's logsumexp; the restated estimator on a target with closed forms; the six entry
points are declared, exported and bound within ABI 15 and answer their argument checks without a device; the Python layers route to
them: HipNVP / HipSpline bind an `importance` entry and the other families do not, Sampler.importance_evidence chooses its route from
what it can observe, names what the fused route does not take, cuts a run into launches by `sample_offset`, and states log Z in
either convention."""
import ctypes
import inspect
import logging
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp

from tests import importance_check as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_importance_groups', 'nnest_importance_evidence', 'nnest_spline_importance_evidence', 'nnest_importance_fill_noise',
       'nnest_importance_check', 'nnest_spline_importance_check')


def test_result_against_logsumexp():
    from nnest_amd import _lib
    rng = np.random.RandomState(0)
    for M in (1, 2, 17, 1000):
        lw = rng.normal(size=M) * 3.0 - 40.0
        if M >= 17:
            lw[3], lw[5] = -np.inf, np.nan   # dead
        live = ic.is_live(lw)
        for res in (ic.result(*ic.sums(lw), M), _lib.importance_result(*ic.sums(lw), M)):
            assert res['logz_x'] == pytest.approx(logsumexp(lw[live]) - np.log(M), rel=1e-13, abs=1e-12)
            w = np.exp(lw[live] - lw[live].max())
            assert res['ess'] == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-12)
            assert res['max_weight_share'] == pytest.approx(w.max() / w.sum(), rel=1e-12)
            if M > 1:
                # the standard error of the mean weight (dead samples weigh 0) over the mean weight
                wf = np.where(live, np.exp(np.where(live, lw, 0.0) - lw[live].max()), 0.0)
                assert res['logzerr'] == pytest.approx(np.sqrt(((wf * wf).mean() / wf.mean() ** 2 - 1.0) / (M - 1)), rel=1e-9)
        assert _lib.importance_result(*ic.sums(lw), M)['n_live'] == int(live.sum())
    # everything dead; a single live sample
    for res in (ic.result(*ic.sums([-np.inf, np.nan, -np.inf]), 3), _lib.importance_result(*ic.sums([-np.inf, np.nan, -np.inf]), 3)):
        assert res['logz_x'] == -np.inf and res['ess'] == 0.0 and res['logzerr'] == np.inf
    assert ic.sums([-np.inf, np.nan]) == (-np.inf, 0.0, 0.0, 0.0)
    for res in (ic.result(*ic.sums([-np.inf, -3.5, np.nan, -np.inf]), 4), _lib.importance_result(*ic.sums([-np.inf, -3.5, np.nan, -np.inf]), 4)):
        assert res['logz_x'] == pytest.approx(-3.5 - np.log(4.0), rel=1e-15) and res['ess'] == 1.0 and res['max_weight_share'] == 1.0
        assert res['logzerr'] == pytest.approx(1.0, rel=1e-15)   # sqrt((4 / 1 - 1) / 3)


def test_merge_of_any_split_is_the_whole():
    from nnest_amd import _lib
    rng = np.random.RandomState(1)
    lw = rng.normal(size=5000) * 5.0 + 100.0
    lw[rng.randint(0, 5000, size=200)] = -np.inf
    lw[:40] = -np.inf   # (a part with nothing live)
    whole = ic.sums(lw)
    for cuts in ([40], [40, 41], [1, 2, 3, 4999], sorted(rng.randint(0, 5000, size=9).tolist()), []):
        parts = [ic.sums(p) for p in np.split(lw, cuts)]
        for merged in (ic.merge(parts), _lib.merge_importance(parts)):
            assert merged[0] == whole[0] and merged[3] == whole[3]
            assert merged[1] == pytest.approx(whole[1], rel=1e-12) and merged[2] == pytest.approx(whole[2], rel=1e-12)
    assert _lib.merge_importance([]) == (-np.inf, 0.0, 0.0, 0.0)
    assert _lib.merge_importance([(-np.inf, 0.0, 0.0, 0.0)] * 2) == (-np.inf, 0.0, 0.0, 0.0)


def test_restated_estimator_on_closed_forms():
    """identity flow, the target the normalised N(0, A) with A < 2 I: Z = 1 and ESS / M -> prod a_i sqrt(2 / a_i - 1) over the
    eigenvalues a_i of A (E_q[w^2] = prod 1 / sqrt(a_i (2 - a_i))); the eigenvalues stay below 4/3, where w^2 has a variance, so the
    ESS has a standard error (the delta method on (mean w)^2 / mean w^2)"""
    M, D = 1 << 16, 3
    eig = np.array([0.7, 1.0, 1.2])
    rng = np.random.RandomState(2)
    R, _ = np.linalg.qr(rng.normal(size=(D, D)))
    A = (R * eig) @ R.T
    Ainv, logdetA = np.linalg.inv(A), np.log(eig).sum()
    logl = lambda x: -0.5 * np.einsum('ni,ij,nj->n', x, Ainv, x) - 0.5 * logdetA - 0.5 * D * np.log(2 * np.pi)
    lp = ic.latent_target(lambda q: (np.asarray(q, np.float64), np.zeros(len(q))), logl, lambda x: np.ones(len(x), bool))
    z = rng.standard_normal((M, D)).astype(np.float32)
    lw = ic.logw_of(z, lp)
    res = ic.result(*ic.sums(lw), M)
    assert abs(res['logz_x']) <= 4.0 * res['logzerr'] and 0.0 < res['logzerr'] < 0.01
    w = np.exp(lw)
    m1, m2 = w.mean(), (w * w).mean()
    g1, g2 = 2.0 * m1 / m2, -m1 * m1 / (m2 * m2)
    c = np.cov(np.stack([w, w * w]))
    se = np.sqrt((g1 * g1 * c[0, 0] + g2 * g2 * c[1, 1] + 2.0 * g1 * g2 * c[0, 1]) / M)
    exact = np.prod(eig * np.sqrt(2.0 / eig - 1.0))
    assert abs(res['ess'] / M - exact) <= 4.0 * se and se < 0.01
    # a box that cuts the target: Z is its mass, the dead samples weigh 0
    lp_box = ic.latent_target(lambda q: (np.asarray(q, np.float64), np.zeros(len(q))), logl, lambda x: np.all(np.abs(x) <= 1.5, axis=1))
    lwb = ic.logw_of(z, lp_box)
    rb = ic.result(*ic.sums(lwb), M)
    mass = np.mean(np.all(np.abs(rng.multivariate_normal(np.zeros(D), A, size=400000)) <= 1.5, axis=1))
    assert abs(rb['logz_x'] - np.log(mass)) <= 4.0 * np.hypot(rb['logzerr'], np.sqrt((1 - mass) / mass / 400000))
    assert ic.sums(lwb)[3] == np.sum(np.all(np.abs(z.astype(np.float64)) <= 1.5, axis=1))


def test_restated_draws():
    """stream 7, step 0: unit normals that depend on the global sample index alone; a narrower run shares the blocks; the stream is
    not the random walk's"""
    from tests.mcmc_walk_check import mcmc_draws
    z = ic.importance_draws(11, 1000, 3000, 7)
    assert z.shape == (3000, 7) and z.dtype == np.float32
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03
    assert np.array_equal(ic.importance_draws(11, 1024, 100, 7), z[24:124])
    assert np.array_equal(ic.importance_draws(11, 1000, 10, 5), z[:10, :5])
    far = ic.importance_draws(11, (3 << 32) + 1000, 10, 7)
    assert not np.array_equal(far, z[:10]) and np.all(np.isfinite(far))
    assert not np.array_equal(mcmc_draws(11, 1000, 10, 0, 1, 7)[0][0], z[:10])


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
    assert _lib.SIGNATURES['nnest_spline_importance_evidence'] == _lib.SIGNATURES['nnest_importance_evidence']   # one argument list
    assert lib.nnest_hip_version() == 15


def test_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1
    p = ctypes.c_void_p(64)   # (never dereferenced: every call below is refused before a launch)
    lk = _lib.like_spec(3, 1.0, (0.5,))
    L = ctypes.byref(lk)
    for fn in (lib.nnest_importance_evidence, lib.nnest_spline_importance_evidence):
        def ev(h=None, like=L, t_std=p, t_mean=p, lo=None, hi=None, z=p, x=p, logl=p, logw=p, partials=p, sums=p, M=8):
            return fn(h, like, t_std, t_mean, lo, hi, z, x, logl, logw, partials, sums, M, 0, 0, None)

        assert ev() == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()
        assert ev(z=None, x=None, logl=None, logw=None) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (optional)
        assert ev(M=0, partials=None) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()   # (M = 0 is valid, and has no partials)
        assert ev(like=None) == E_ARG and b'NULL' in lib.nnest_hip_last_error()
        assert ev(sums=None) == E_ARG and b'sums_dev' in lib.nnest_hip_last_error()
        assert ev(partials=None) == E_ARG and b'partials_dev' in lib.nnest_hip_last_error()
        assert ev(M=-1) == E_ARG and b'M=-1' in lib.nnest_hip_last_error()
        for name in ('z', 'x', 'logl', 'logw'):
            assert ev(**{name: None}) == E_ARG, name
            assert b'all or none' in lib.nnest_hip_last_error(), name
        for name in ('t_std', 't_mean', 'lo', 'hi'):
            assert ev(**{name: None if name.startswith('t_') else p}) == E_ARG, name
            assert b'both or neither' in lib.nnest_hip_last_error(), name
    assert lib.nnest_importance_fill_noise(p, 8, 0, 0, 0, None) == E_ARG and b'D=0' in lib.nnest_hip_last_error()
    assert lib.nnest_importance_fill_noise(p, -1, 3, 0, 0, None) == E_ARG
    assert lib.nnest_importance_fill_noise(None, 8, 3, 0, 0, None) == E_ARG
    assert lib.nnest_importance_groups(-1, 4) == -1 and lib.nnest_importance_groups(8, 5) == -1
    for fn in (lib.nnest_importance_check, lib.nnest_spline_importance_check):
        assert fn(None, 3) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()


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
        assert 'importance_evidence' not in cls.__dict__ and cls.importance_evidence is _HipFlow.importance_evidence   # one body
    assert "importance='nnest_importance_evidence'" in inspect.getsource(HipNVP.__init__)
    assert "importance='nnest_spline_importance_evidence'" in inspect.getsource(HipSpline.__init__)
    assert bound(HipSpline, 'nnest_spline', importance='nnest_spline_importance_evidence')._sym['importance'] is lib.nnest_spline_importance_evidence
    assert bound(HipNVP, 'nnest_nvp', importance='nnest_importance_evidence')._sym['importance'] is lib.nnest_importance_evidence
    assert (HipNVP._IMPORTANCE_TILE, HipSpline._IMPORTANCE_TILE) == (4, 16)
    assert "importance_check='nnest_importance_check'" in inspect.getsource(HipNVP.__init__)
    assert "importance_check='nnest_spline_importance_check'" in inspect.getsource(HipSpline.__init__)
    for cls in (HipNVP, HipSpline):
        assert cls.importance_refusal is _HipFlow.importance_refusal
    assert callable(flow.importance_fill_noise)
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        assert 'importance' not in inspect.getsource(cls.__init__)
        o = bound(cls, family)
        o.device = 'cpu'
        assert 'importance' not in o._sym
        with pytest.raises(NotImplementedError):
            o.importance_evidence(3, 8)
        with pytest.raises(NotImplementedError):
            o.importance_refusal(3)


# ---- the front end on stub flows --------------------------------------------------------------------------------------------
def stub_logw(m):
    """the stub flow's log weight of global sample m; every seventh sample is dead"""
    m = np.asarray(m, np.float64)
    return np.where(m % 7 == 3, -np.inf, 2.0 * np.sin(0.37 * m) - 5.0)


class _StubFlow(object):
    """what importance_evidence asks of the flow, recorded.  Fused: sample m has the log weight stub_logw(m) and x = m in every
    dimension.  Host: sample() hands out consecutive global indices as x, log_probs(x) = -stub_logw(x[:, 0])"""
    device = 'cpu'
    base_beta = 0.0
    base_dist = None

    def __init__(self, D):
        self._sym = {'importance': object()}
        self.D, self.calls, self.next, self.refuse, self.asked = D, [], 0, None, []

    def importance_refusal(self, like_id):
        self.asked.append(like_id)
        return self.refuse

    def importance_evidence(self, like_id, M, t_std=None, t_mean=None, lo=None, hi=None, seed=0, sample_offset=0, like_params=None,
                            want_samples=False):
        import torch
        self.calls.append((like_id, M, sample_offset, seed, want_samples, None if lo is None else (float(lo[0]), float(hi[0]))))
        m = sample_offset + np.arange(M)
        out = dict(sums=torch.as_tensor(ic.sums(stub_logw(m)), dtype=torch.float64))
        if want_samples:
            out.update(x=torch.as_tensor(np.repeat(m[:, None], self.D, 1).astype(np.float32)), logw=torch.as_tensor(stub_logw(m)))
        return out

    def sample(self, n):
        import torch
        m = self.next + np.arange(n)
        self.next += n
        return torch.as_tensor(np.repeat(m[:, None], self.D, 1).astype(np.float32))

    def log_probs(self, x):
        import torch
        return torch.as_tensor(-np.where(np.isfinite(stub_logw(x[:, 0].numpy())), stub_logw(x[:, 0].numpy()), 0.0))


class _StubTrainer(object):
    def __init__(self, net):
        self.netG = net


class _UnitBox(object):
    def is_unit_box(self):
        return True


def _bare_sampler(D, net, agrees=True, prior=None, cls=None):
    from nnest_amd.mcmc import MCMCSampler

    class _Like(object):
        hip_like_id, hip_like_params = 3, (0.5,)

    cls = cls or MCMCSampler
    s = cls.__new__(cls)
    s.x_dim, s.num_derived, s.num_slow, s.trainer = D, 0, 0, _StubTrainer(net)
    s.total_calls = 0
    s._user_loglike, s._user_prior, s._user_transform, s._transform_prior, s._linear_scale = _Like(), prior, None, True, 1.0
    s.transform = lambda x: x
    s._probe_agrees = lambda like_id, params, **kw: agrees   # (the one step of _device_target that needs a device)
    s.single_or_primary_process = True
    s.logger = logging.getLogger('test_importance_check')
    # the host route's callables: the likelihood is 0, the prior kills what the stub's weights call dead
    s.loglike = lambda x: (np.zeros(len(x)), np.empty((len(x), 0)))
    s.prior = lambda x: np.where(np.isfinite(stub_logw(x[:, 0])), 0.0, -np.inf)
    return s


def test_front_end_routes_and_chunks(caplog):
    D, M = 3, 1000
    whole = ic.result(*ic.sums(stub_logw(np.arange(M))), M)
    net = _StubFlow(D)
    s = _bare_sampler(D, net)
    with caplog.at_level(logging.INFO, logger='test_importance_check'):
        out = s.importance_evidence(M, seed=5, chunk=300)
    assert [r for r in caplog.records if 'importance' in r.getMessage()]
    # the run is cut by `chunk`, each launch addressed by its first global sample; one seed
    assert net.calls == [(3, 300, 0, 5, False, None), (3, 300, 300, 5, False, None), (3, 300, 600, 5, False, None), (3, 100, 900, 5, False, None)]
    assert out['route'] == 'fused' and s.importance_route == 'fused' and s.total_calls == M
    assert out['logz'] == pytest.approx(whole['logz_x'], rel=1e-12)   # (T = identity: no constant)
    assert out['ess'] == pytest.approx(whole['ess'], rel=1e-12) and out['logzerr'] == pytest.approx(whole['logzerr'], rel=1e-12)
    assert out['n_samples'] == M and out['n_live'] == int(np.isfinite(stub_logw(np.arange(M))).sum())
    assert out['max_weight_share'] == pytest.approx(whole['max_weight_share'], rel=1e-12)
    assert set(out) == {'logz', 'logzerr', 'ess', 'n_samples', 'n_live', 'max_weight_share', 'route'}
    # the default chunk: 2^22 without samples, by ENSEMBLE_HISTORY_BYTES with them
    net.calls.clear()
    s.ENSEMBLE_HISTORY_BYTES = 400 * (8 * D + 16)
    got = s.importance_evidence(M, seed=6, return_samples=True)
    assert [c[1:3] for c in net.calls] == [(400, 0), (400, 400), (200, 800)] and all(c[4] for c in net.calls)
    assert got['samples'].shape == (M, D) and got['logw'].shape == (M,)
    np.testing.assert_array_equal(got['samples'][:, 0], np.arange(M))
    np.testing.assert_array_equal(got['logw'], stub_logw(np.arange(M)))
    assert got['logz'] == pytest.approx(logsumexp(got['logw']) - np.log(M), rel=1e-12)
    net.calls.clear()
    s.importance_evidence(M)
    assert [c[1:3] for c in net.calls] == [(M, 0)] and net.calls[0][3] == net.calls[0][3] & 0xFFFFFFFFFFFFFFFF
    # route='host' on the same sampler: the same weights through sample / log_probs / loglike / prior
    host = s.importance_evidence(M, route='host', chunk=256, return_samples=True)
    assert host['route'] == 'host' and s.importance_route == 'host' and net.next == M
    assert host['logz'] == pytest.approx(whole['logz_x'], rel=1e-12) and host['ess'] == pytest.approx(whole['ess'], rel=1e-12)
    assert host['n_live'] == out['n_live'] and host['samples'].shape == (M, D)
    with pytest.raises(ValueError, match='route'):
        s.importance_evidence(M, route='rounds')
    with pytest.raises(ValueError, match='num_samples'):
        s.importance_evidence(0)


def test_front_end_names_what_the_fused_route_does_not_take():
    D, M = 3, 64
    changes = ((dict(num_derived=1), 'derived'), (dict(num_slow=1), 'fast/slow'), (dict(_user_loglike=lambda x: x), 'Python callable'))
    for change, word in changes:
        s = _bare_sampler(D, _StubFlow(D))
        for k, v in change.items():
            setattr(s, k, v)
        with pytest.raises(ValueError, match='the fused route does not take .*%s' % word):
            s.importance_evidence(M, route='fused')
        assert s.importance_evidence(M)['route'] == 'host'   # route=None: a selection from what the code can observe
    net = _StubFlow(D)
    del net._sym['importance']
    s = _bare_sampler(D, net)
    with pytest.raises(ValueError, match='_StubFlow'):
        s.importance_evidence(M, route='fused')
    assert s.importance_evidence(M)['route'] == 'host'
    # what the library says of the flow's shape or base, asked before any launch, is the reason
    for words in ('importance: GeneralisedNormal base (beta=8): the kernel draws from N(0, I) only',
                  "importance: x_dim=3 hidden=32 blocks=3 layers=1 scale mode 0: the kernel takes hidden 16, 3 blocks, 1 layer"):
        net = _StubFlow(D)
        net.refuse = words
        s = _bare_sampler(D, net)
        with pytest.raises(ValueError, match='the fused route does not take the flow _StubFlow: importance: ' + words.split(':')[1].strip()[:12]):
            s.importance_evidence(M, route='fused')
        assert s.importance_evidence(M)['route'] == 'host' and net.calls == [] and net.asked == [3, 3]
    s = _bare_sampler(D, _StubFlow(D), agrees=False)
    with pytest.raises(ValueError, match='prior'):
        s.importance_evidence(M, route='fused')
    assert s.importance_evidence(M)['route'] == 'host'


def test_front_end_states_log_z_in_either_convention():
    from nnest_amd.priors import UniformPrior
    D, M = 3, 500
    whole = ic.result(*ic.sums(stub_logw(np.arange(M))), M)
    # an installed affine transform: Z over theta = T(x), so sum log|t_std| is added (a UniformPrior stays the indicator it is)
    for route in ('fused', 'host'):
        net = _StubFlow(D)
        s = _bare_sampler(D, net, prior=UniformPrior(D, -5.0, 5.0))
        s._install_transform(np.array([1.0, 2.0, 3.0]), np.array([0.5, -2.0, 4.0]))
        out = s.importance_evidence(M, route=route, seed=1)
        assert out['route'] == route
        assert out['logz'] == pytest.approx(whole['logz_x'] + np.log(0.5 * 2.0 * 4.0), rel=1e-12)
        if route == 'fused':
            assert net.calls[0][5] == (-5.0, 5.0)
    # the NestedSampler's prior, the unit box on x under x -> s x: the box on T(x) is +-s, and log Z is over the normalised prior
    for route in ('fused', 'host'):
        net = _StubFlow(D)
        s = _bare_sampler(D, net)
        s._user_prior, s._transform_prior, s._linear_scale, s._user_transform = _UnitBox(), False, 5.0, (lambda x: 5.0 * x)
        s.transform = lambda x: 5.0 * x
        out = s.importance_evidence(M, route=route, seed=1, return_samples=True)
        assert out['route'] == route
        assert out['logz'] == pytest.approx(whole['logz_x'] - D * np.log(2.0), rel=1e-12)
        np.testing.assert_array_equal(out['samples'][:, 0], 5.0 * np.arange(M))
        if route == 'fused':
            assert net.calls[0][5] == (-5.0, 5.0)
    # the unit box on x under a transform that is not linear: the host route, and still the normalised prior
    s = _bare_sampler(D, _StubFlow(D), agrees=False)
    s._user_prior, s._transform_prior, s._linear_scale, s._user_transform = _UnitBox(), False, None, (lambda x: x ** 3)
    out = s.importance_evidence(M)
    assert out['route'] == 'host' and out['logz'] == pytest.approx(whole['logz_x'] - D * np.log(2.0), rel=1e-12)
    # another prior evaluated on x (transform_prior=False) under an affine transform: Z over x is the evidence, nothing is added
    s = _bare_sampler(D, _StubFlow(D), agrees=False)
    s._install_transform(np.array([1.0, 2.0, 3.0]), np.array([0.5, -2.0, 4.0]))
    s._user_prior, s._transform_prior = object(), False
    out = s.importance_evidence(M)
    assert out['route'] == 'host' and out['logz'] == pytest.approx(whole['logz_x'], rel=1e-12)
    # a transform that is not affine and no prior: Z stays over x
    s = _bare_sampler(D, _StubFlow(D), agrees=False)
    s._linear_scale, s._user_transform = None, (lambda x: x ** 3)
    out = s.importance_evidence(M)
    assert out['route'] == 'host' and out['logz'] == pytest.approx(whole['logz_x'], rel=1e-12)
    # everything dead
    s = _bare_sampler(D, _StubFlow(D))
    import torch
    s.trainer.netG.importance_evidence = lambda like_id, M, **kw: dict(sums=torch.tensor([-np.inf, 0.0, 0.0, 0.0], dtype=torch.float64))
    out = s.importance_evidence(M, seed=1)
    assert out['logz'] == -np.inf and out['ess'] == 0.0 and out['logzerr'] == np.inf and out['n_live'] == 0
