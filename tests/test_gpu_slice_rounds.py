"""[UNPINNED] The slice proposal in rounds (include/nnest_hip.h nnest_slice_rounds_*; nnest_amd/slice_rounds.py) for every flow and
both likelihood routes -- a host callable on the packed rows, or the device likelihood kernel.  ABSENT FROM THE REFERENCE
(nnest/sampler.py:310-316 proposes random-walk Metropolis moves only), so the step is build-defined (nnest_slice_steps's definition)
and these tests hold it to the CPU restatement oracle.slice_sample on the same directions (nnest_slice_fill_noise) and the shared
Philox uniforms, to the invariants of a slice-sampling update, and to the closed-form evidence of the reference's own test problem.
Run with  pytest -m gpu."""
import ctypes
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import oracle as orc  # noqa: E402  (checker only)

G = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def hip():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    from nnest_amd import slice_rounds
    return slice_rounds


def cpu(t):
    return t.detach().cpu().numpy()


def make(kind, D):
    """(the HIP flow, a function that returns its CPU twin once the flow's state is final)"""
    from nnest_amd.flow import HipNVP
    if kind == 'nvp':
        f = HipNVP(D, 16, 3, 1, seed=3)
        return f, lambda: orc.NVP(D, 16, 3, 1, f.store_packed())
    if kind == 'nvp_h32_translate':   # a shape nnest_slice_steps refuses
        f = HipNVP(D, 32, 3, 1, seed=3, scale='translate')
        return f, lambda: orc.NVP(D, 32, 3, 1, f.store_packed(), scale='translate')
    if kind == 'maf':
        from nnest_amd.maf import HipMAF
        f = HipMAF(D, 16, 3, 1, seed=3)
        return f, lambda: orc.NVP(D, 16, 3, 1, f.store_packed(), kind='maf')
    if kind == 'spline':
        from nnest_amd.spline import HipSpline
        f = HipSpline(D, 16, 3, 8, 3.0, seed=3)   # (ActNorm's first-batch initialisation happens on the first forward)
        return f, lambda: orc.Spline(D, 16, 3, 8, 3.0, f.store_packed(), f.P)
    if kind == 'cholesky':
        from nnest_amd.cholesky import HipCholesky
        g = np.load(os.path.join(G, 'cholesky_d5.npz'))
        assert int(g['D']) == D
        f = HipCholesky(D)
        f.load_packed(g['w0'])
        return f, lambda: orc.Cholesky(D, g['w0'])
    if kind == 'fastslow':
        from nnest_amd.fastslow import HipFastSlowNVP
        g = np.load(os.path.join(G, 'fastslow_s2_f3.npz'))
        S, F = int(g['S']), int(g['F'])
        assert S + F == D
        f = HipFastSlowNVP(F, S, 16, 3, 1)
        f.load_packed(g['w_trained'])
        return f, lambda: orc.FastSlowNVP(S, F, weights=g['w_trained'])
    raise ValueError(kind)


def fill_noise(D, S, C, seed, off):
    """the directions nnest_slice_fill_noise exports (flow-independent)"""
    from nnest_amd import _lib
    dz = torch.empty(S, C, D, dtype=torch.float32, device='cuda')
    _lib.check(_lib.load().nnest_slice_fill_noise(_lib.ptr(dz), S, C, D, seed, off, _lib.current_stream(dz.device)))
    return dz


def start(f, D, C, seed=0):
    rng = np.random.RandomState(seed)
    u = rng.uniform(-0.6, 0.6, size=(C, D))
    l0 = orc.loglike('rosenbrock', u, 5.0)
    star = float(np.quantile(l0, 0.2))
    keep = l0 > star
    u, l0 = u[keep], l0[keep]
    z, _ = f.forward(u)
    return cpu(z).copy(), l0, star


def host_rosenbrock(counter=None):
    def like(x):
        assert x.dtype == np.float32 and x.shape[0] > 0
        if counter is not None:
            counter.append(x.shape[0])
        return orc.loglike('rosenbrock', x, 5.0)
    return like


def run(sr, f, z0, l0, star, width, S, route, seed, off, **kw):
    z = torch.from_numpy(z0).cuda()
    logl = torch.from_numpy(l0).cuda()
    if route == 'host':
        r = sr.slice_rounds(f, z, logl, star, width, S, loglike=host_rosenbrock(kw.pop('counter', None)), seed=seed, walker_offset=off,
                            **kw)
    else:
        r = sr.slice_rounds(f, z, logl, star, width, S, like_id=0, like_scale=5.0, seed=seed, walker_offset=off, **kw)
    return z, logl, r


CASES = [('nvp', 2, 40, 8), ('nvp', 20, 33, 5), ('nvp', 50, 48, 5), ('nvp_h32_translate', 6, 40, 5), ('maf', 10, 40, 5),
         ('spline', 20, 33, 5), ('cholesky', 5, 40, 6), ('fastslow', 5, 40, 6)]


@pytest.mark.parametrize('route', ['host', 'device'])
@pytest.mark.parametrize('kind,D,C,S', CASES, ids=['%s-d%d' % (c[0], c[1]) for c in CASES])
def test_rounds_vs_oracle_restatement(hip, kind, D, C, S, route):
    """the driver's chains against oracle.slice_sample on the exported directions and the shared Philox uniforms: at least 80 % of
    the walkers agree on every counter and state; one that does not had a candidate within rounding of a decision threshold (box edge,
    slice level, L*) where it leaves"""
    f, twin = make(kind, D)
    z0, l0, star = start(f, D, C)
    o = twin()
    C = z0.shape[0]
    width = 2.0 / np.sqrt(D)
    seed, off = 4242, 100
    dz = cpu(fill_noise(D, S, C, seed, off))
    z, logl, res = run(hip, f, z0, l0, star, width, S, route, seed, off, history=True)
    margins = np.empty((S, C))
    ref = orc.slice_sample(o, 'rosenbrock', 5.0, z0, l0, star, width, dz, seed, walker_offset=off, margins=margins)
    hx = cpu(res['hist_x'])
    same = (cpu(res['n_eval']) == ref['n_eval']) & (cpu(res['n_call']) == ref['n_call']) & (cpu(res['n_move']) == ref['n_move'])
    assert same.mean() >= 0.8, same.mean()
    assert np.max(np.abs(hx[same] - ref['x'][same]) / (1.0 + np.abs(ref['x'][same]))) < 2e-4
    assert np.max(np.abs(cpu(z)[same] - ref['z'][same]) / (1.0 + np.abs(ref['z'][same]))) < 2e-4
    assert np.max(np.abs(cpu(logl)[same] - ref['logl'][same]) / (1.0 + np.abs(ref['logl'][same]))) < 2e-4
    for c in np.flatnonzero(~same):
        d = np.max(np.abs(hx[c] - ref['x'][c]) / (1.0 + np.abs(ref['x'][c])), axis=1) > 1e-3
        s_first = int(np.argmax(d)) if d.any() else S
        lo = max(s_first - 1, 0)
        assert np.min(margins[lo:min(s_first + 1, S), c]) < 2e-4, (c, s_first, margins[:, c])
    assert res['rounds'] == int(cpu(res['n_eval']).max())   # a batch costs its busiest walker's evaluations
    # the recorded-direction path replays the same run
    z2, logl2, res2 = run(hip, f, z0, l0, star, width, S, route, seed, off, noise=torch.from_numpy(dz).cuda())
    assert torch.equal(z2, z) and torch.equal(logl2, logl) and torch.equal(res2['n_eval'], res['n_eval'])


@pytest.mark.parametrize('kind,D', [('maf', 20), ('nvp', 20)])
def test_host_and_device_likelihood_routes_take_the_same_decisions(hip, kind, D):
    f, _ = make(kind, D)
    z0, l0, star = start(f, D, 200, seed=2)
    a = run(hip, f, z0, l0, star, 2.0 / np.sqrt(D), 6, 'host', 77, 0)
    b = run(hip, f, z0, l0, star, 2.0 / np.sqrt(D), 6, 'device', 77, 0)
    same = cpu(a[2]['n_eval']) == cpu(b[2]['n_eval'])
    assert same.mean() > 0.95, same.mean()
    np.testing.assert_allclose(cpu(a[0])[same], cpu(b[0])[same], rtol=0, atol=1e-4)
    assert np.array_equal(cpu(a[2]['n_call'])[same], cpu(b[2]['n_call'])[same])


def test_round_updates_keep_the_constraint_and_move(hip):
    """every chain ends inside the box above L*, the counters are consistent, nearly every update moves, the host callable sees
    exactly sum(n_call) rows, a repeated launch repeats its bits and a shard reproduces its slice of the full launch"""
    D, S = 50, 20
    f, _ = make('nvp_h32_translate', D)
    z0, l0, star = start(f, D, 1000, seed=1)
    C = z0.shape[0]
    seen = []
    z, logl, r = run(hip, f, z0, l0, star, 2.0 / np.sqrt(D), S, 'host', 9, 0, counter=seen)
    r = {k: cpu(v) for k, v in r.items() if torch.is_tensor(v)}
    assert np.all(np.abs(r['x']) <= 1.0) and np.all(cpu(logl) > star)
    assert np.all(r['n_eval'] >= r['n_call']) and np.all(r['n_call'] >= r['n_move']) and np.all(r['n_move'] <= S)
    assert r['n_move'].mean() > 0.95 * S
    assert r['moved'].mean() > 0.99
    assert sum(seen) == int(r['n_call'].sum()) and min(seen) > 0
    np.testing.assert_allclose(cpu(logl), orc.loglike('rosenbrock', r['x'], 5.0), rtol=0, atol=0)
    x_chk, _ = f.inverse(z)
    assert torch.equal(x_chk, torch.from_numpy(r['x']).cuda())
    z2, logl2, r2 = run(hip, f, z0, l0, star, 2.0 / np.sqrt(D), S, 'host', 9, 0)
    assert torch.equal(z, z2) and torch.equal(logl, logl2) and np.array_equal(r['n_eval'], cpu(r2['n_eval']))
    zs, ls, _ = run(hip, f, z0[256:512], l0[256:512], star, 2.0 / np.sqrt(D), S, 'host', 9, 256)
    assert torch.equal(zs, z[256:512]) and torch.equal(ls, logl[256:512])


def test_derived_parameters_follow_the_accepted_rows(hip):
    D, S = 6, 8
    f, _ = make('maf', D)
    z0, l0, star = start(f, D, 300, seed=3)
    C = z0.shape[0]

    def like(x):
        return orc.loglike('rosenbrock', x, 5.0), np.stack([x.sum(axis=1), x[:, 0] * x[:, 1]], axis=1).astype(np.float64)

    init_d = like(orc.NVP(D, 16, 3, 1, f.store_packed(), kind='maf').inverse(z0)[0])[1]
    z, logl = torch.from_numpy(z0).cuda(), torch.from_numpy(l0).cuda()
    r = hip.slice_rounds(f, z, logl, star, 2.0 / np.sqrt(D), S, loglike=like, num_derived=2, init_derived=init_d, seed=5, history=True)
    x = cpu(r['x'])
    ll, dd = like(x)
    assert np.array_equal(r['derived'], dd) and np.array_equal(cpu(logl), ll)
    hx = cpu(r['hist_x'])
    for it in range(1, S + 1):
        assert np.array_equal(r['hist_derived'][:, it], like(hx[:, it])[1]), it
    assert np.array_equal(r['hist_derived'][:, 0], init_d)


def _rosenbrock_py(x):
    """Rosenbrock 2-D as a plain Python callable (no hip_like_id: the host protocol)"""
    from nnest_amd.likelihoods import Rosenbrock
    return Rosenbrock(2)(x)


@pytest.mark.parametrize('flow,known', [('nvp', False), ('spline', False), ('maf', True)])
def test_nested_sampling_with_slice_rounds_rosenbrock_2d(hip, tmp_path, flow, known):
    """NestedSampler(mcmc_proposal='slice') on the reference's own integration problem (tests/test_nested.py:10-19: Rosenbrock 2-D,
    closed form log Z = -5.804) through the round driver: a plain Python likelihood with the NVP and the spline flow, the known
    likelihood with the MAF (no fused slice kernel).  Acceptance above 0.95 is the slice signature: every update moves."""
    from nnest_amd.likelihoods import Rosenbrock
    from nnest_amd.nested import NestedSampler
    closed = math.log(math.pi / 10 * (1 - 0.5 * math.erfc(math.sqrt(5) - 1)) / 100)
    logz = []
    for seed in range(4):
        np.random.seed(seed)
        torch.manual_seed(seed)
        s = NestedSampler(2, Rosenbrock(2) if known else _rosenbrock_py, transform=lambda x: 5.0 * x, log_dir=str(tmp_path / str(seed)),
                          num_live_points=1000, log_level=30, flow=flow, mcmc_proposal='slice')
        assert (s._fused_like_id is not None) == known
        s.run(mcmc_num_chains=100, mcmc_steps=5, train_iters=500)
        assert abs(s.logz - closed) < 4 * s.logzerr + 0.05, (seed, s.logz, s.logzerr)
        assert s.total_accepted / (s.total_accepted + s.total_rejected) > 0.95
        logz.append(s.logz)
    assert abs(np.mean(logz) - closed) < 0.15, logz
