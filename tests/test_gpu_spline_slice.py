"""[UNPINNED] The slice proposal in latent space with the neural-spline flow (include/nnest_hip.h nnest_spline_slice_steps).  ABSENT
FROM THE REFERENCE (nnest/sampler.py:310-316 proposes random-walk Metropolis moves only): the step is build-defined, the definition
of the NVP's slice kernel with the spline's inverse.  These tests hold the kernel, in each of its forms, to the CPU restatement of
that definition (oracle/oracle.py::slice_sample with an oracle.Spline) on the kernel's own directions and the shared Philox
uniforms, to the invariants a slice-sampling update must keep, and to the closed-form evidence of the reference's own test
problem.  Run with  pytest -m gpu."""
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
    from nnest_amd import _lib
    from nnest_amd.spline import HipSpline
    # the spline flow has a slice method of its own and the library exports its entry point: without them the inherited NVP method
    # would hand the spline handle to nnest_slice_steps
    assert 'slice_steps' in HipSpline.__dict__
    assert hasattr(_lib.load(), 'nnest_spline_slice_steps') and hasattr(_lib.load(), 'nnest_spline_slice_form_for')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return HipSpline


def cpu(t):
    return t.detach().cpu().numpy()


def make_flow(HipSpline, case):
    """the HipSpline of a test case (a seeded default initialisation is completed by ActNorm's first-batch initialisation on the
    first forward batch, networks.py:698-705, as in a run: `start` pushes one through)"""
    if case in ('d50', 'd5'):   # flows trained by the reference on Rosenbrock (weights and permutations)
        g = np.load(os.path.join(G, 'mcmc_spline_rosen_%s.npz' % case))
        D, H, B, K, tail, w, P = int(g['D']), int(g['H']), int(g['B']), int(g['K']), float(g['tail']), g['w'], g['P']
    elif case in ('h32', 'h10'):   # hidden 32; hidden 10 (zero-padded to 16 in the handle)
        g = np.load(os.path.join(G, 'spline_d8_h32.npz' if case == 'h32' else 'spline_d6_h10.npz'))
        D, H, B, K, tail, w, P = int(g['D']), int(g['H']), int(g['B']), int(g['K']), float(g['tail']), g['w_trained'], g['P']
    else:   # seeded default initialisation
        D = int(case[1:])
        return HipSpline(D, 16, 3, 8, 3.0, seed=3)
    sp = HipSpline(D, H, B, K, tail)
    sp.load_packed(w, P)
    sp.data_dep_init_done = True   # past ActNorm's first-batch initialisation (networks.py:696)
    return sp


def oracle_of(sp):
    return orc.Spline(sp.D, sp.H, sp.B, sp.K, sp.tail_bound, sp.store_packed(), sp.P)


def start(sp, C, seed=0):
    """C points above L* (the 20 % quantile of the draws) and their latent images"""
    D = sp.D
    rng = np.random.RandomState(seed)
    u = rng.uniform(-0.6, 0.6, size=(3 * C, D))
    l = orc.loglike('rosenbrock', u, 5.0)
    star = float(np.quantile(l, 0.2))
    keep = np.flatnonzero(l > star)[:C]
    u, l = u[keep], l[keep]
    z, _ = sp.forward(u)
    return cpu(z).copy(), l, star


CASES = [('d50', 45, 4, 'wave'), ('d50', 45, 4, 'team'), ('d50', 45, 4, 'pair'), ('d5', 37, 6, None), ('d2', 29, 8, None),
         ('d20', 33, 5, None), ('h32', 27, 5, None), ('h10', 27, 5, None)]


@pytest.mark.parametrize('case,C,S,form', CASES, ids=['%s-%s' % (c[0], c[3] or 'auto') for c in CASES])
def test_spline_slice_kernel_vs_oracle_restatement(hip, case, C, S, form):
    """the kernel's chains against oracle.slice_sample(oracle.Spline) on the kernel's own directions (fill_slice_noise) and the shared
    Philox uniforms: every walker whose counters agree must agree in every state; one that does not must have had a candidate within
    rounding of a decision threshold (box edge, slice level, L*) at the update where it leaves"""
    sp = make_flow(hip, case)
    D = sp.D
    z0, l0, star = start(sp, C)
    o = oracle_of(sp)
    assert C % 8 != 0 and z0.shape[0] == C   # ragged: the last tile is partly empty in every form
    assert sp.slice_form_for(C, form) == (form or sp.slice_form_for(C))
    width = 2.0 / np.sqrt(D)
    seed, off = 4242, 100
    dz = sp.fill_slice_noise(S, C, seed=seed, walker_offset=off)
    z = torch.from_numpy(z0).cuda()
    logl = torch.from_numpy(l0).cuda()
    res = sp.slice_steps(0, 5.0, z, logl, star, width, S, seed=seed, walker_offset=off, history=True, form=form)
    margins = np.empty((S, C))
    ref = orc.slice_sample(o, 'rosenbrock', 5.0, z0, l0, star, width, cpu(dz), seed, walker_offset=off, margins=margins)
    hx = cpu(res['hist_x'])
    same = (cpu(res['n_eval']) == ref['n_eval']) & (cpu(res['n_call']) == ref['n_call']) & (cpu(res['n_move']) == ref['n_move'])
    assert same.mean() >= 0.8, same.mean()
    err = np.max(np.abs(hx[same] - ref['x'][same]) / (1.0 + np.abs(ref['x'][same])))
    assert err < 2e-4, err
    assert np.max(np.abs(cpu(logl)[same] - ref['logl'][same]) / (1.0 + np.abs(ref['logl'][same]))) < 2e-4
    for c in np.flatnonzero(~same):   # a walker that took another decision: where it leaves, the oracle was within rounding of a threshold
        d = np.max(np.abs(hx[c] - ref['x'][c]) / (1.0 + np.abs(ref['x'][c])), axis=1) > 1e-3
        s_first = int(np.argmax(d)) if d.any() else S
        lo = max(s_first - 1, 0)
        assert np.min(margins[lo:min(s_first + 1, S), c]) < 2e-4, (c, s_first, margins[:, c])
    # the recorded-noise path replays the in-kernel launch bit for bit
    z2 = torch.from_numpy(z0).cuda()
    logl2 = torch.from_numpy(l0).cuda()
    res2 = sp.slice_steps(0, 5.0, z2, logl2, star, width, S, noise=dz, seed=seed, walker_offset=off, history=True, form=form)
    assert torch.equal(z2, z) and torch.equal(logl2, logl) and torch.equal(res2['hist_x'], res['hist_x'])
    for k in ('n_eval', 'n_call', 'n_move', 'moved'):
        assert torch.equal(res2[k], res[k]), k


def test_spline_slice_updates_keep_the_constraint_and_move(hip):
    """at x_dim 50 with the reference-trained flow, 1000 walkers x 20 updates: every chain ends inside the box and above L*, nearly
    every update moves, the counters are consistent, the end state is the state of the end point, a repeated launch repeats its bits
    and a shard reproduces its slice of the full launch"""
    sp = make_flow(hip, 'd50')
    D, S = 50, 20
    z0, l0, star = start(sp, 1000, seed=1)
    o = oracle_of(sp)
    C = z0.shape[0]
    width = 2.0 / np.sqrt(D)
    form = sp.slice_form_for(C)   # pinned on the shard too, as a sharded caller would

    def run(lo, hi, off, steps=S, f=form):
        z = torch.from_numpy(z0[lo:hi]).cuda()
        logl = torch.from_numpy(l0[lo:hi]).cuda()
        r = sp.slice_steps(0, 5.0, z, logl, star, width, steps, seed=9, walker_offset=off, form=f)
        return cpu(z), cpu(logl), {k: cpu(v) for k, v in r.items() if v is not None}

    z, logl, r = run(0, C, 0)
    assert np.all(np.abs(r['x']) <= 1.0) and np.all(logl > star)
    assert np.all(r['n_eval'] >= r['n_call']) and np.all(r['n_call'] >= r['n_move']) and np.all(r['n_move'] <= S)
    assert r['n_move'].mean() > 0.95 * S                       # shrinkage ends on a point of the slice
    assert r['moved'].mean() > 0.99                            # the reference's usable-chain test (nested.py:432)
    np.testing.assert_allclose(logl, orc.loglike('rosenbrock', r['x'], 5.0), rtol=2e-6, atol=1e-5)
    x_chk, _ = o.inverse(z)
    assert np.max(np.abs(x_chk - r['x'])) < 5e-5
    z2, logl2, r2 = run(0, C, 0)
    assert np.array_equal(z, z2) and np.array_equal(logl, logl2)
    for k in ('n_eval', 'n_call', 'n_move', 'moved', 'x'):
        assert np.array_equal(r[k], r2[k]), k
    zs, ls, rs = run(256, 512, 256)
    assert np.array_equal(zs, z[256:512]) and np.array_equal(ls, logl[256:512]) and np.array_equal(rs['n_eval'], r['n_eval'][256:512])


def test_spline_slice_forms_agree(hip):
    """the three forms run the same walkers on the same streams.  Not bit for bit: the team form sums a walker's log-det from four
    waves' partials and the pair form from two halves of the columns, the wave form in one wave -- float32 association differs in
    the last bits, and a slice decision that falls within that rounding of its threshold sends the chain elsewhere.  So the
    criterion of the oracle test: 80 % of walkers with identical counters, and those agree in every state to rounding."""
    sp = make_flow(hip, 'd50')
    S = 5
    z0, l0, star = start(sp, 1000, seed=2)
    out = {}
    for f in ('wave', 'team', 'pair'):
        z = torch.from_numpy(z0).cuda()
        logl = torch.from_numpy(l0).cuda()
        r = sp.slice_steps(0, 5.0, z, logl, star, 2.0 / np.sqrt(50), S, seed=11, walker_offset=0, form=f)
        out[f] = (cpu(z), cpu(logl), {k: cpu(v) for k, v in r.items() if v is not None})
    zw, lw, rw = out['wave']
    for f in ('team', 'pair'):
        zf, lf, rf = out[f]
        same = (rf['n_eval'] == rw['n_eval']) & (rf['n_call'] == rw['n_call']) & (rf['n_move'] == rw['n_move'])
        assert same.mean() >= 0.8, (f, same.mean())
        assert np.max(np.abs(rf['x'][same] - rw['x'][same]) / (1.0 + np.abs(rw['x'][same]))) < 2e-4, f
        assert np.max(np.abs(lf[same] - lw[same]) / (1.0 + np.abs(lw[same]))) < 2e-4, f
        assert np.all(np.abs(rf['x']) <= 1.0) and np.all(lf > star)


def test_spline_slice_refusals(hip):
    from nnest_amd import _lib
    from nnest_amd.cholesky import HipCholesky
    sp = make_flow(hip, 'd20')
    z = torch.zeros(8, 20, device='cuda')
    logl = torch.zeros(8, dtype=torch.float64, device='cuda')
    assert sp.slice_form_for(8, 'pair') is None   # two halves of 16-slot tiles: x_dim > 32 only
    with pytest.raises(_lib.NnestHipError) as ei:
        sp.slice_steps(0, 5.0, z, logl, -1e9, 0.5, 2, form='pair')
    assert ei.value.code == 3   # NNEST_E_UNSUPPORTED
    with pytest.raises(_lib.NnestHipError) as ei:
        sp.slice_steps(0, 5.0, z, logl, -1e9, 0.5, 2, max_shrink=0)
    assert ei.value.code == 1   # NNEST_E_ARG
    ch = HipCholesky(6)
    with pytest.raises(NotImplementedError):
        ch.slice_steps(0, 5.0, torch.zeros(8, 6, device='cuda'), logl, -1e9, 0.5, 2)


def test_nested_sampling_with_the_spline_slice_proposal_rosenbrock_2d(hip, tmp_path):
    """NestedSampler(flow='spline', mcmc_proposal='slice') on the reference's own integration problem (tests/test_nested.py:10-19:
    Rosenbrock 2-D, closed form log Z = -5.804): the mean over seeds within 0.15, each run within 4 of its own error"""
    from nnest_amd.likelihoods import Rosenbrock
    from nnest_amd.nested import NestedSampler
    closed = math.log(math.pi / 10 * (1 - 0.5 * math.erfc(math.sqrt(5) - 1)) / 100)
    logz = []
    for seed in range(4):
        np.random.seed(seed)
        torch.manual_seed(seed)
        s = NestedSampler(2, Rosenbrock(2), transform=lambda x: 5.0 * x, log_dir=str(tmp_path / str(seed)), num_live_points=1000,
                          log_level=30, flow='spline', mcmc_proposal='slice')
        assert s._fused_like_id is not None
        s.run(mcmc_num_chains=100, mcmc_steps=5, train_iters=500)
        assert abs(s.logz - closed) < 4 * s.logzerr + 0.05, (seed, s.logz, s.logzerr)
        logz.append(s.logz)
    assert abs(np.mean(logz) - closed) < 0.15, logz
