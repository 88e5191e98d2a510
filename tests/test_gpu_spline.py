"""GPU parity for the neural-spline flow (reference networks.py:393-715) through the C ABI:
passes against the fixtures produced by the reference (tests/golden/spline_*.npz) and against the oracle, the fused
proposal kernel against the oracle-side restatement of Sampler._mcmc_sample.  Run with  pytest -m gpu."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import oracle as orc  # noqa: E402  (checker only)
from tests.mh_checks import spline_mcmc_trace, assert_borderline, first_divergence, spline_fixture_launch, check_spline_fixture  # noqa: E402

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(G, 'spline_*.npz')))
IDS = [os.path.basename(p)[7:-4] for p in FILES]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def hip():
    from nnest_amd import spline
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return spline


@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_passes_vs_reference_fixture(hip, path):
    g = np.load(path)
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    sp = hip.HipSpline(D, H, B, K, float(g['tail']))
    assert sp.num_params == g['w_raw'].size
    assert list(sp.state_dict().keys()) == [str(k) for k in g['keys']]
    # raw state (randn ActNorm): inverse, with rows outside the spline interval
    sp.load_packed(g['w_raw'], g['P'])
    o = orc.Spline(D, H, B, K, float(g['tail']), g['w_raw'], g['P'])
    xi, ldi = sp.inverse(g['z0'])
    xo, ldo = o.inverse(g['z0'])
    xo64, _ = o.inverse(g['z0'], f64=True)
    tol = max(3e-5, 4 * rel(xo, xo64))
    assert rel(cpu(xi), g['x_inv_raw']) < tol and rel(cpu(ldi), g['ld_inv_raw']) < tol
    for tag in ('init', 'trained'):
        sp.load_packed(g['w_' + tag], g['P'])
        sp.data_dep_init_done = True   # these weights are past ActNorm's first-batch initialisation (networks.py:696)
        assert np.array_equal(sp.store_packed(), g['w_' + tag]) and np.array_equal(sp.P, g['P'])
        x = g['x']
        # measured against the float64 oracle the kernels sit at 1e-6..2e-6, the level of the reference's own float32
        # (tests/diag_spline_err.py); against the reference's float32 outputs: 1e-5 relative-to-(1+|v|)
        z, ld = sp.forward(x)
        assert rel(cpu(z), g['z_' + tag]) < 1e-5
        assert rel(cpu(ld), g['ldf_' + tag]) < 1e-5
        xb, ldb = sp.inverse(g['z_' + tag])
        assert rel(cpu(xb)[2:], g['xb_' + tag][2:]) < 1e-5 and rel(cpu(xb), g['xb_' + tag]) < 1e-4   # rows 0-1: see below
        assert rel(cpu(ldb)[2:], g['ldi_' + tag][2:]) < 1e-5 and rel(cpu(ldb), g['ldi_' + tag]) < 1e-4
        xs, lds = sp.inverse(g['zs'])
        assert rel(cpu(xs), g['xs_' + tag]) < 1e-5
        assert rel(cpu(lds), g['lds_' + tag]) < 1e-5
        assert rel(cpu(sp.log_probs(x)), g['lp_' + tag]) < 1e-5
        # round trip (tests/test_flows.py:27-30 asks 1e-5 of in-distribution rows; rows 0-1 of x are pushed far outside
        # the training box, where the spline's end bins are steep and the inverse is ill-conditioned)
        xr, ldr = sp.inverse(z)
        assert rel(cpu(xr)[2:], x[2:]) <= 1e-5 and rel(cpu(xr), x) <= 1e-4
        assert rel(cpu(ldr)[2:], -cpu(ld)[2:]) <= 2e-5


def test_ragged_sizes_and_fused_eval(hip):
    g = np.load(os.path.join(G, 'spline_d5.npz'))
    D, H, B, K = 5, 16, 3, 8
    sp = hip.HipSpline(D, H, B, K, 3.0)
    sp.load_packed(g['w_trained'], g['P'])
    sp.data_dep_init_done = True
    o = orc.Spline(D, H, B, K, 3.0, g['w_trained'], g['P'])
    rng = np.random.RandomState(0)
    for N in (0, 1, 15, 16, 17, 1000, 70001):
        z = (0.7 * rng.randn(N, D)).astype(np.float32)
        x, ld = sp.inverse(z)
        assert x.shape == (N, D)
        if 0 < N <= 1000:
            xo, ldo = o.inverse(z)
            assert rel(cpu(x), xo) < 3e-5 and rel(cpu(ld), ldo) < 3e-5
            x2, ld2, logl, inbox = sp.inverse_loglike(0, 5.0, z)
            assert torch.equal(x2, x) and torch.equal(ld2, ld)
            lo = orc.loglike('rosenbrock', cpu(x), 5.0)
            np.testing.assert_allclose(cpu(logl), lo, rtol=2e-6, atol=1e-5)
            assert np.array_equal(cpu(inbox) == 1, orc.prior_inbox(cpu(x)) == 0)
    xl, _ = sp.inverse((0.7 * rng.randn(70001, D)).astype(np.float32)[-5:])
    assert np.all(np.isfinite(cpu(xl)))


def _assert_first_leaver_borderline(h_gpu, h_orc, margins):
    first = first_divergence(h_gpu, h_orc)
    assert np.any(first >= 1), 'the counters differ but no chain leaves the oracle\'s'
    w = min((int(s_), int(k)) for k, s_ in enumerate(first) if s_ >= 1)[1]
    assert_borderline(h_gpu, h_orc, margins, [w])


@pytest.mark.parametrize('name,C', [('d5', 40), ('d50', 40), ('d8_h32', 100), ('d50', 3000), ('d5', 9000)])
def test_fused_proposal_kernel_vs_oracle(hip, name, C):
    """K4 with the spline inverse: the kernel's own noise draws (nnest_mh_fill_noise) replayed through the oracle-side
    restatement of Sampler._mcmc_sample's hard-constraint branch (sampler.py:291-444)."""
    g = np.load(os.path.join(G, 'spline_%s.npz' % name))
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    sp = hip.HipSpline(D, H, B, K, 3.0)
    sp.load_packed(g['w_trained'], g['P'])
    sp.data_dep_init_done = True
    o = orc.Spline(D, H, B, K, 3.0, g['w_trained'], g['P'])
    rng = np.random.RandomState(C)
    S = 8
    init = rng.uniform(-0.5, 0.5, size=(C, D))
    init_logl = orc.loglike('rosenbrock', init, 5.0)
    dz, u = sp.fill_noise(S, C, seed=5)
    z, _ = sp.forward(init)
    z0 = cpu(z).copy()
    logl = torch.from_numpy(init_logl).cuda()
    step = 0.1 / np.sqrt(D)
    res = sp.mh_steps(0, 5.0, z, logl, -1e12, step, S, seed=5, history=True, dynamic='group')
    ngood = 0
    for g0 in list(range(0, min(C, 96), 16)):
        sl = slice(g0, min(g0 + 16, C))
        margins = np.empty((S, sl.stop - sl.start))
        tr = spline_mcmc_trace(o, z0[sl], init_logl[sl], -1e12, step, cpu(dz)[:, sl], cpu(u)[:, sl], margins=margins)
        if tr['ncall'] == int(res['n_call'][sl].sum()) and tr['nacc'] == int(res['n_accept'][sl].sum()):
            assert rel(cpu(res['hist_x'])[sl], tr['x']) < 3e-4
            hl = cpu(res['hist_logl'])[sl]
            assert np.max(np.abs(hl - tr['logl'])) < 2e-3 * (1.0 + np.max(np.abs(tr['logl'])))
            assert abs(float(res['scale'][g0 // 16]) - tr['scale']) < 1e-5 * tr['scale']
            ngood += 1
        else:   # a decision fell the other way: it must have been a rounding-borderline one (round-5 verdict: no silent skip)
            _assert_first_leaver_borderline(cpu(res['hist_x'])[sl], tr['x'], margins)
    assert ngood >= max(1, len(range(0, min(C, 96), 16)) - 1)
    assert int(res['n_accept'].sum()) > 0
    # production instantiation lands on the same state
    z2 = torch.from_numpy(z0).cuda()
    logl2 = torch.from_numpy(init_logl).cuda()
    res2 = sp.mh_steps(0, 5.0, z2, logl2, -1e12, step, S, seed=5, dynamic='group')
    assert torch.equal(z2, z) and torch.equal(logl2, logl) and torch.equal(res2['x'], res['x'])


@pytest.mark.parametrize('C,rule', [(40, False), (1000, False), (333, 'batch'), (1000, 'batch')])
def test_pair_form_of_the_proposal_kernel_vs_oracle(hip, C, rule):
    """round 5: at x_dim > 32, a fixed step or the batch-wide rule and up to 8 walkers per CU the proposal kernel runs its PAIR form
    (nnest_spline_mh.hip: 8 walkers per workgroup held in both halves of the matrix-core columns, one spline evaluation per lane
    serving two super-tiles).  Held to the oracle's restatement of sampler.py:291-444 on the kernel's own noise -- fixed step per
    16 walkers, the batch rule (lag 0: the reference's own) over the whole batch -- and to the team form it replaces."""
    g = np.load(os.path.join(G, 'spline_d50.npz'))
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    sp = hip.HipSpline(D, H, B, K, 3.0)
    sp.load_packed(g['w_trained'], g['P'])
    sp.data_dep_init_done = True
    o = orc.Spline(D, H, B, K, 3.0, g['w_trained'], g['P'])
    rng = np.random.RandomState(C)
    S = 8
    init = rng.uniform(-0.5, 0.5, size=(C, D))
    init_logl = orc.loglike('rosenbrock', init, 5.0)
    dz, u = sp.fill_noise(S, C, seed=5)
    z, _ = sp.forward(init)
    z0 = cpu(z).copy()
    logl = torch.from_numpy(init_logl).cuda()
    step = 0.1 / np.sqrt(D)
    kw = dict(dynamic='batch', lag=0) if rule == 'batch' else dict(dynamic=False)
    res = sp.mh_steps(0, 5.0, z, logl, -1e12, step, S, seed=5, history=True, **kw)
    groups = [slice(0, C)] if rule == 'batch' else [slice(g0, min(g0 + 16, C)) for g0 in range(0, min(C, 96), 16)]
    ngood = 0
    for sl in groups:
        margins = np.empty((S, sl.stop - sl.start))
        tr = spline_mcmc_trace(o, z0[sl], init_logl[sl], -1e12, step, cpu(dz)[:, sl], cpu(u)[:, sl], adapt=rule == 'batch', margins=margins)
        if tr['ncall'] == int(res['n_call'][sl].sum()) and tr['nacc'] == int(res['n_accept'][sl].sum()):
            assert rel(cpu(res['hist_x'])[sl], tr['x']) < 3e-4
            hl = cpu(res['hist_logl'])[sl]
            assert np.max(np.abs(hl - tr['logl'])) < 2e-3 * (1.0 + np.max(np.abs(tr['logl'])))
            if rule == 'batch':
                assert abs(float(res['scale'][0]) - tr['scale']) < 1e-5 * tr['scale']
                assert float(res['scale'].min()) == float(res['scale'].max())
            ngood += 1
        else:   # a decision fell the other way: the walker that leaves the oracle's chain FIRST did so at a step the oracle decided
            #         at rounding level (round-5 verdict: asserted, not skipped)
            _assert_first_leaver_borderline(cpu(res['hist_x'])[sl], tr['x'], margins)
            if rule == 'batch':   # one borderline decision among C x S: the counts differ by that one, the rule's votes rarely
                assert abs(tr['nacc'] - int(res['n_accept'][sl].sum())) <= 2 and abs(tr['ncall'] - int(res['n_call'][sl].sum())) <= 2
                ngood += 1
    assert ngood >= max(1, len(groups) - 1)
    assert int(res['n_accept'].sum()) > 0
    if rule is False:
        assert np.all(cpu(res['scale']) == np.float32(step))
    # the production instantiation lands on the same state
    z2 = torch.from_numpy(z0).cuda()
    logl2 = torch.from_numpy(init_logl).cuda()
    res2 = sp.mh_steps(0, 5.0, z2, logl2, -1e12, step, S, seed=5, **kw)
    assert torch.equal(z2, z) and torch.equal(logl2, logl) and torch.equal(res2['x'], res['x'])
    assert torch.equal(res2['n_accept'], res['n_accept']) and torch.equal(res2['moved'], res['moved'])


MCMC_SPLINE = sorted(glob.glob(os.path.join(G, 'mcmc_spline_*.npz')))


def _spline_oracle(g):
    return orc.Spline(int(g['D']), int(g['H']), int(g['B']), int(g['K']), float(g['tail']), g['w'], g['P'])


@pytest.mark.parametrize('path', MCMC_SPLINE, ids=[os.path.basename(p)[12:-4] for p in MCMC_SPLINE])
def test_proposal_kernels_vs_the_references_recorded_spline_trace(hip, path):
    """Round-5 verdict item 2: Sampler._mcmc_sample (nnest/sampler.py:291-444) on the reference's DEFAULT flow (NSF_CL,
    nnest/networks.py:458-556) with torch's draws recorded (oracle/gen_golden.py::gen_mcmc_spline): EVERY accept / reject decision
    of the reference, every state, the final scale, the usable-chain flag -- through every form of the proposal kernel that can take
    the trace in this process: the form the library picks for the batch (pair at x_dim 50, team at x_dim 5) under the
    reference's rule (whole batch, lag 0) or the fixed step, the team form under the per-16-walker rule where the batch IS one group
    of 16, and the one-wave-per-tile form on the trace repeated over 8 208 walkers (every group of 16 is the reference's batch again,
    and must repeat group 0 bit for bit)."""
    g = np.load(path)
    D, C, dyn = int(g['D']), g['dz'].shape[1], bool(g['dynamic'])
    o = _spline_oracle(g)
    ran = []
    out = spline_fixture_launch(path, 'batch' if dyn else 'fixed')
    assert out['form'] == ('pair' if D > 32 else 'team')
    check_spline_fixture(out, g, o)
    ran.append(out['form'])
    if C == 16:
        if dyn:   # one group of 16 = the whole batch: the per-group rule is the reference's rule
            out = spline_fixture_launch(path, 'group')
            assert out['form'] == 'team'
            check_spline_fixture(out, g, o)
            ran.append('team')
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        reps = 2 * cu + 1
        out = spline_fixture_launch(path, 'group' if dyn else 'fixed', reps=reps)
        assert out['form'] == 'wave'
        check_spline_fixture(out, g, o)
        for k in range(1, reps):   # (same walkers, same noise, same rule: the same bits)
            sl = slice(16 * k, 16 * k + 16)
            assert np.array_equal(out['hist_x'][sl], out['hist_x'][:16]) and np.array_equal(out['n_accept'][sl], out['n_accept'][:16])
        ran.append('wave')
    assert len(ran) >= 1


@pytest.mark.parametrize('name', ['rosen_d50', 'rosen_d50_c40_dyn'])
def test_team_form_vs_the_references_recorded_spline_trace_at_x_dim_50(hip, name):
    """the team form at x_dim 50 under a fixed step / the batch-wide rule (where the library would pick the pair form):
    NNEST_SPLINE_MH_FORM=team is read once per process, so the launch runs in a process of its own"""
    import subprocess
    import sys
    import tempfile
    path = os.path.join(G, 'mcmc_spline_%s.npz' % name)
    g = np.load(path)
    code = ('import sys, numpy as np; sys.path.insert(0, %r); from tests.mh_checks import spline_fixture_launch; '
            'out = spline_fixture_launch(%r, %r); np.savez(sys.argv[1], **out)' % (ROOT, path, 'batch' if bool(g['dynamic']) else 'fixed'))
    with tempfile.NamedTemporaryFile(suffix='.npz') as f:
        subprocess.run([sys.executable, '-c', code, f.name], check=True, env=dict(os.environ, NNEST_SPLINE_MH_FORM='team'), timeout=600)
        out = dict(np.load(f.name))
    assert str(out['form']) == 'team'
    check_spline_fixture(out, g, _spline_oracle(g))


def test_the_library_says_which_proposal_form_runs(hip):
    """nnest_spline_mh_form_for: pair at x_dim 50 under a fixed step / the batch rule up to 8 walkers per CU, team under the
    per-16-walker rule, at small x_dim and up to 32 walkers per CU, one wave per tile beyond; the test above therefore drove the
    pair form"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    big = hip.HipSpline(50, 16, 3, 8, 3.0)
    assert big.kernel_form_for(1000) == 'pair' and big.kernel_form_for(40) == 'pair' and big.kernel_form_for(8 * cu) == 'pair'
    assert big.kernel_form_for(1000, dynamic='batch', lag=0) == 'pair' and big.kernel_form_for(333, dynamic='batch', lag=4) == 'pair'
    assert big.kernel_form_for(1000, dynamic='group') == 'team'
    assert big.kernel_form_for(8 * cu + 1) == 'team' and big.kernel_form_for(32 * cu) == 'team'
    assert big.kernel_form_for(32 * cu + 1) == 'wave'
    assert big.kernel_form_for(16 * cu + 1, dynamic='batch', lag=0) is None     # the batch rule needs a resident grid
    small = hip.HipSpline(20, 16, 3, 8, 3.0)
    assert small.kernel_form_for(1000) == 'team' and small.kernel_form_for(32 * cu + 1) == 'wave'


def test_pair_form_against_the_team_form(hip):
    """the same launch through the two small-population forms (NNEST_SPLINE_MH_FORM=team keeps the team form; read once per process,
    so each form runs in a process of its own): same walkers, same noise streams, the same arithmetic per walker -- up to the
    multiply-add contractions hipcc chooses per kernel, which can flip a borderline decision: nearly every chain ends on the same
    point up to rounding, and the accept counts agree to a fraction of a percent"""
    import subprocess
    import sys
    code = '''
import sys, numpy as np, torch
sys.path.insert(0, %r)
from nnest_amd.spline import HipSpline
import nnest_amd.flow as nflow
g = np.load(%r)
sp = HipSpline(int(g['D']), int(g['H']), int(g['B']), int(g['K']), 3.0)
sp.load_packed(g['w_trained'], g['P']); sp.data_dep_init_done = True
rng = np.random.RandomState(3)
init = rng.uniform(-0.5, 0.5, size=(1000, int(g['D'])))
logl = nflow.loglike(0, init, 5.0, device=torch.device('cuda', 0))
z, _ = sp.forward(init)
res = sp.mh_steps(0, 5.0, z, logl, float(logl.min()) - 1.0, 0.1 / np.sqrt(int(g['D'])), 50, seed=11, dynamic=False)
np.savez(sys.argv[1], x=res['x'].cpu().numpy(), n_accept=res['n_accept'].cpu().numpy(), n_call=res['n_call'].cpu().numpy(), logl=logl.cpu().numpy())
''' % (ROOT, os.path.join(G, 'spline_d50.npz'))
    import tempfile
    out = {}
    for form in ('pair', 'team'):
        with tempfile.NamedTemporaryFile(suffix='.npz') as f:
            env = dict(os.environ, NNEST_SPLINE_MH_FORM=form)
            subprocess.run([sys.executable, '-c', code, f.name], check=True, env=env, timeout=600)
            out[form] = dict(np.load(f.name))
    a, b = out['pair'], out['team']
    close = np.max(np.abs(a['x'] - b['x']), axis=1) < 1e-4      # (a chain that took the same decisions ends within rounding)
    assert close.mean() > 0.97, close.mean()
    assert np.mean(a['n_accept'] == b['n_accept']) > 0.97
    assert abs(int(a['n_accept'].sum()) - int(b['n_accept'].sum())) <= 0.01 * int(b['n_accept'].sum()) + 5
    assert int(b['n_accept'].sum()) > 1000
    np.testing.assert_allclose(a['logl'][close], b['logl'][close], rtol=1e-4, atol=1e-3)


# ---- training -----------------------------------------------------------------------------------------------------
def test_rows_form_of_the_training_step_against_the_tile_form(hip):
    """the same gradient and the same training call through the two forms of the training step (nnest_spline_train_form: 'rows' -- one
    row of the minibatch per workgroup, nnest_spline_rows.hip -- where the shape allows it; NNEST_SPL_ROWS=0 pins the tile form; read
    once per process, so each form runs in a process of its own).  Same arithmetic per row, other summation orders (the rows form
    contracts the weight gradients over the rows on the matrix cores): gradients agree to rounding, the loss trajectories of a short
    call stay together.  The tests below drive the rows form at hidden_dim 16, x_dim <= 64;
    test_tile_form_of_the_training_step_vs_the_reference_fixtures holds the tile form to the same fixtures."""
    import subprocess
    import sys
    import tempfile
    code = '''
import sys, numpy as np, torch
sys.path.insert(0, %r)
from nnest_amd.spline import HipSpline
out = {}
for D in (2, 5, 50):
    g = np.load(%r %% D)
    sp = HipSpline(D, int(g['H']), int(g['B']), int(g['K']), float(g['tail']))
    sp.load_packed(g['w_trained'], g['P']); sp.data_dep_init_done = True
    rng = np.random.RandomState(D)
    live = rng.uniform(-0.8, 0.8, size=(500, D))
    loss, grad = sp.loss_grad(live[:100])
    perms = torch.stack([torch.randperm(450, generator=torch.Generator().manual_seed(e)) for e in range(6)]).int()
    res = sp.train_epochs(live[50:], live[:50], perms, None, seed=3, jitter=0.01, batch=100, max_epochs=6, patience=50)
    out['form_%%d' %% D] = np.array(sp.train_form_for(100))
    out['loss_%%d' %% D] = loss.cpu().numpy(); out['grad_%%d' %% D] = grad.cpu().numpy()
    out['traj_%%d' %% D] = res['losses'].numpy()[:res['epochs_run']]
    out['w_%%d' %% D] = sp.store_packed()
np.savez(sys.argv[1], **out)
''' % (ROOT, os.path.join(G, 'spline_d%d.npz'))
    got = {}
    for form, env in (('rows', {}), ('tiles', {'NNEST_SPL_ROWS': '0'})):
        with tempfile.NamedTemporaryFile(suffix='.npz') as f:
            subprocess.run([sys.executable, '-c', code, f.name], check=True, env=dict(os.environ, **env), timeout=600)
            got[form] = dict(np.load(f.name))
    for D in (2, 5, 50):
        a, b = got['rows'], got['tiles']
        assert str(a['form_%d' % D]) == 'rows' and str(b['form_%d' % D]) == 'tiles'
        assert rel(a['loss_%d' % D], b['loss_%d' % D]) < 1e-5
        assert rel(a['grad_%d' % D], b['grad_%d' % D]) < 2e-5, D
        assert not np.array_equal(a['grad_%d' % D], b['grad_%d' % D])     # (two kernels, not one)
        np.testing.assert_allclose(a['traj_%d' % D], b['traj_%d' % D], rtol=2e-3)
        assert rel(a['w_%d' % D], b['w_%d' % D]) < 2e-2


def test_tile_form_of_the_training_step_vs_the_reference_fixtures(hip):
    """the training tests of this file once more with NNEST_SPL_ROWS=0 (the tile form, nnest_spline_train.hip, at the shapes where the
    library would pick the rows form): autograd gradients, the reference's Adam trajectory, one step = gradient + Adam, early stopping"""
    import subprocess
    import sys
    if os.environ.get('NNEST_SPL_ROWS') == '0':
        pytest.skip('already inside the tile-form run')
    k = ('test_loss_and_gradient_vs_reference_autograd or test_adam_steps_vs_reference_trajectory or test_one_training_step_is_gradient_plus_adam '
         'or test_training_improves_and_is_reproducible or test_spline_training_stops_when_patience_runs_out')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-k', k, '-p', 'no:cacheprovider'],
                       env=dict(os.environ, NNEST_SPL_ROWS='0'), cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_actnorm_data_dependent_init_vs_reference(hip, path):
    """networks.py:698-705: the first forward batch of a fresh model sets s = -log std, t = -mean(x e^s) per block"""
    g = np.load(path)
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    sp = hip.HipSpline(D, H, B, K, float(g['tail']))
    sp.load_packed(g['w_raw'], g['P'])
    assert not sp.data_dep_init_done
    z, ld = sp.forward(g['x_first'])
    assert sp.data_dep_init_done
    w = sp.store_packed()
    bs = sp.num_params // B
    st = np.concatenate([np.arange(2 * D) + b * bs for b in range(B)])
    assert np.max(np.abs(w[st] - g['w_init'][st])) < 3e-5
    other = np.setdiff1d(np.arange(sp.num_params), st)
    assert np.array_equal(w[other], g['w_raw'][other])
    assert rel(cpu(z), g['z_first']) < 5e-5 and rel(cpu(ld), g['ld_first']) < 5e-5


@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_loss_and_gradient_vs_reference_autograd(hip, path):
    """every element of dLoss/dw against the reference's autograd gradient (tests/golden/spline_*.npz, first two steps)"""
    g = np.load(path)
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    sp = hip.HipSpline(D, H, B, K, float(g['tail']))
    sp.load_packed(g['w_init'], g['P'])
    sp.data_dep_init_done = True
    for k in range(2):
        if k == 1:
            sp.load_packed(g['ws'][0], g['P'])
        data = g['X'][g['perms'][0][100 * k:100 * (k + 1)]] + np.float32(g['jitter']) * g['noises'][0][100 * k:100 * (k + 1)]
        loss, grad = sp.loss_grad(data)
        assert abs(float(loss) - g['losses'][k]) < 2e-5 * (1 + abs(g['losses'][k]))
        gref = g['grads'][k]
        err = np.abs(cpu(grad) - gref)
        assert np.max(err) < 2e-4 * (1e-3 + np.max(np.abs(gref))), (k, int(np.argmax(err)), float(np.max(err)), float(np.max(np.abs(gref))))
    # ragged batch sizes: the loss is a mean over rows, so gradients of disjoint batches combine linearly
    # (M_A g_A + M_B g_B = (M_A + M_B) g_AB), single-row and full-tile batches included; loss against the oracle
    o = orc.Spline(D, H, B, K, float(g['tail']), g['w_init'], g['P'])
    sp.load_packed(g['w_init'], g['P'])
    X = g['X']

    def lg(rows):
        loss, grad = sp.loss_grad(X[rows])
        lo = o.log_probs(X[rows], f64=True)[1]
        assert abs(float(loss) - lo) < 3e-5 * (1 + abs(lo))
        return cpu(grad).astype(np.float64)

    g0, g1_36, g0_36, g37_99, g0_99, g100_227 = lg(slice(0, 1)), lg(slice(1, 37)), lg(slice(0, 37)), lg(slice(37, 100)), \
        lg(slice(0, 100)), lg(slice(100, 228))
    scale = np.max(np.abs(g0_99))
    assert np.max(np.abs(1 * g0 + 36 * g1_36 - 37 * g0_36)) < 2e-4 * 37 * scale
    assert np.max(np.abs(37 * g0_36 + 63 * g37_99 - 100 * g0_99)) < 2e-4 * 100 * scale
    assert np.all(np.isfinite(g100_227))
    idx = np.random.RandomState(1).choice(np.argsort(-np.abs(g0_99))[:300], 10, replace=False)
    fd = o.fd_grad(X[:100], idx)
    assert np.median(np.abs(fd - g0_99[idx])) < 5e-3 * scale     # piecewise-smooth loss: FD is only a coarse yardstick


@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_adam_steps_vs_reference_trajectory(hip, path):
    """two epochs of Trainer._train (trainer.py:384-403) with the recorded shuffles and jitter noise"""
    g = np.load(path)
    D, H, B, K = int(g['D']), int(g['H']), int(g['B']), int(g['K'])
    sp = hip.HipSpline(D, H, B, K, float(g['tail']))
    sp.load_packed(g['w_init'], g['P'])
    sp.data_dep_init_done = True
    X = g['X']
    n = X.shape[0]
    res = sp.train_epochs(X, X[:23], torch.from_numpy(g['perms'].astype(np.int32)), torch.from_numpy(g['noises']),
                          jitter=float(g['jitter']), batch=100, max_epochs=2, patience=50)
    losses = res['losses'].numpy()[:2, 0] * n
    ref = g['losses'].reshape(2, -1).sum(axis=1)
    np.testing.assert_allclose(losses, ref, rtol=5e-5)
    # the run restores the best-validation weights; with 2 epochs that is normally the last state
    if res['best_epoch'] == 2:
        dref = g['ws'][-1] - g['w_init']
        dour = sp.store_packed() - g['w_init']
        assert np.sqrt(np.mean((dour - dref) ** 2)) < 0.05 * np.sqrt(np.mean(dref ** 2))
        # element by element against the float64 chain: the six Adam steps (3 minibatches x 2 epochs) with the oracle's gradients
        # at the chain's own weights.  Each step is within 2e-5 of its float64 prediction (tests/test_gpu_spline_grad.py); the
        # weights of the two chains differ by at most the sum of those, and so their later gradients by a second-order amount
        from oracle import spline_grad as sg
        ws, grads = [g['w_init'].astype(np.float64)], []
        for e in range(2):
            for lo in range(0, n, 100):
                sl = slice(lo, min(lo + 100, n))
                data = X[g['perms'][e][sl]] + np.float32(g['jitter']) * g['noises'][e][sl]
                grads.append(sg.loss_grad(ws[-1].astype(np.float32), g['P'], data, D, H, B, K, float(g['tail']))[1])
                ws.append(sg.adam(ws, grads, 1e-3, 1e-6))
        gmax = np.max(np.abs(grads), axis=0)
        keep = np.zeros(gmax.size, bool)
        off = 0
        for _, shape in sp.layer_shapes():
            m = int(np.prod(shape))
            keep[off:off + m] = gmax[off:off + m] >= 1e-3 * np.max(gmax[off:off + m])
            off += m
        err = np.abs(sp.store_packed().astype(np.float64) - ws[-1])[keep]
        assert np.max(err) < 6 * 2e-5, (int(np.flatnonzero(keep)[np.argmax(err)]), float(np.max(err)))


@pytest.mark.parametrize('D,H', [(8, 16), (33, 16), (50, 16), (64, 16), (70, 16), (40, 32)])
def test_one_training_step_is_gradient_plus_adam(hip, D, H):
    """one minibatch of the training loop = loss_grad + one Adam step (torch/optim/adam.py, coupled weight decay): for a shape
    whose loop keeps the training image current from inside the update kernel on 16-row tiles (x_dim 8), the shapes that run
    8-row tiles with one spline evaluation per pair of super-tiles (x_dim 33, 50, 64: the smallest, BASELINE's and the largest
    of that form; hidden_dim 32 = two hidden tiles) and one that rebuilds the image per minibatch (x_dim 70)"""
    rng = np.random.RandomState(3)
    sp = hip.HipSpline(D, H, 2, seed=5)
    X = rng.uniform(-1, 1, size=(140, D))
    sp.actnorm_init(X[:100])
    sp.data_dep_init_done = True
    w0 = sp.store_packed().astype(np.float64)
    loss, grad = sp.loss_grad(X[40:])
    g = cpu(grad).astype(np.float64)
    lr, wd, b1, b2, eps = 1e-3, 1e-6, 0.9, 0.999, 1e-8
    gi = g + wd * w0
    m, v = (1 - b1) * gi, (1 - b2) * gi * gi
    w1 = w0 - (lr / (1 - b1)) * m / (np.sqrt(v) / np.sqrt(1 - b2) + eps)
    perm = torch.arange(100, dtype=torch.int32)[None, :]
    res = sp.train_epochs(X[40:], X[:40], perm, None, seed=1, jitter=0.0, batch=100, max_epochs=1, patience=50, lr=lr, weight_decay=wd)
    assert res['epochs_run'] == 1 and res['best_epoch'] == 1
    np.testing.assert_allclose(float(res['losses'][0, 0]) * 100, float(cpu(loss).ravel()[0]), rtol=2e-5)
    dref, dour = w1 - w0, sp.store_packed().astype(np.float64) - w0
    # |step| = lr for every parameter with a gradient well above eps; compare where the reference step is not degenerate
    big = np.abs(g) > 1e-5
    assert big.sum() > 0.5 * big.size
    np.testing.assert_allclose(dour[big], dref[big], rtol=0, atol=2e-5)
    # a second epoch runs from an image that follows the new weights: the loss it reports is the loss at w1
    sp2 = hip.HipSpline(D, H, 2, seed=5)
    sp2.load_packed(sp.store_packed(), sp.P)
    sp2.data_dep_init_done = True
    loss1, _ = sp2.loss_grad(X[40:])
    sp3 = hip.HipSpline(D, H, 2, seed=5)
    sp3.load_packed(w0.astype(np.float32), sp.P)
    sp3.data_dep_init_done = True
    res2 = sp3.train_epochs(X[40:], X[:40], perm.repeat(2, 1), None, seed=1, jitter=0.0, batch=100, max_epochs=2, patience=50, lr=lr,
                            weight_decay=wd)
    np.testing.assert_allclose(float(res2['losses'][1, 0]) * 100, float(cpu(loss1).ravel()[0]), rtol=5e-5)


def test_training_improves_and_is_reproducible(hip):
    rng = np.random.RandomState(0)
    D, N, E = 6, 400, 30
    live = rng.normal(size=(N, D)) * 0.3 + 0.2 * rng.normal(size=(N, 1))
    perms = np.stack([rng.permutation(N - 40) for _ in range(E)]).astype(np.int32)
    outs = []
    for rep in range(2):
        sp = hip.HipSpline(D, 16, 3, seed=4)
        res = sp.train_epochs(live[40:], live[:40], torch.from_numpy(perms), None, seed=11, jitter=0.01, batch=100, max_epochs=E,
                              patience=50)
        outs.append((sp.store_packed(), res['losses'].numpy().copy(), res['best_epoch']))
    # the data-dependent init draws its jitter from torch's generator: compare runs from the same initialised state
    l = outs[0][1]
    assert l[-1, 1] < l[0, 1] and l[-1, 0] < l[0, 0]
    assert np.all(np.isfinite(l))


def test_trainer_spline_save_and_load_model(hip, tmp_path):
    """Trainer(flow='spline') writes models/netG.pt (reference keys) plus the permutations; load_model restores the flow"""
    from nnest_amd.trainer import Trainer
    rng = np.random.RandomState(0)
    live = rng.normal(size=(300, 4)) * 0.3
    t = Trainer(4, log_dir=str(tmp_path / 'run'), log_level=30)
    assert type(t.netG).__name__ == 'HipSpline'
    t.train(live, max_iters=5, jitter=0.01)
    x = rng.uniform(-1, 1, size=(20, 4)).astype(np.float32)
    lp = cpu(t.log_probs(x))
    z = cpu(t.get_latent_samples(x))
    t2 = Trainer(4, log_dir=str(tmp_path), load_model='run', log_level=30)
    assert np.array_equal(cpu(t2.log_probs(x)), lp) and np.array_equal(cpu(t2.get_latent_samples(x)), z)
    assert t.best_validation_epoch >= 1 and t.losses.shape == (5, 2)


@pytest.mark.parametrize('D,H', [(70, 16), (100, 16), (33, 32), (64, 32)])
def test_wider_shapes_vs_oracle(hip, D, H):
    """the other instantiated tile shapes (3 and 4 tiles per half at hidden 16, 2 at hidden 32) against the oracle: passes,
    ActNorm initialisation, loss, gradient (every element against the float64 oracle + linearity over batches)"""
    sp = hip.HipSpline(D, H, 2, seed=D)
    w, P = sp.store_packed(), sp.P
    rng = np.random.RandomState(D)
    x0 = rng.uniform(-1, 1, size=(90, D)).astype(np.float32)
    o = orc.Spline(D, H, 2, 8, 3.0, w, P)
    z, ld = sp.forward(x0)                       # data-dependent init on both sides
    zo, ldo = o.forward(x0, data_init=True)
    assert rel(cpu(z), zo) < 5e-5 and rel(cpu(ld), ldo) < 5e-5
    assert np.max(np.abs(sp.store_packed() - o.w)) < 5e-5
    o.w[:] = sp.store_packed()
    x = rng.uniform(-1, 1, size=(50, D)).astype(np.float32)
    z, ld = sp.forward(x)
    z64, ld64 = o.forward(x, f64=True)
    assert rel(cpu(z), z64) < 1e-5 and rel(cpu(ld), ld64) < 1e-5
    zs = (0.8 * rng.randn(40, D)).astype(np.float32)
    xi, ldi = sp.inverse(zs)
    xi64, ldi64 = o.inverse(zs, f64=True)
    assert rel(cpu(xi), xi64) < 2e-5 and rel(cpu(ldi), ldi64) < 2e-5
    loss, grad = sp.loss_grad(x)
    lo = o.log_probs(x, f64=True)[1]
    assert abs(float(loss) - lo) < 3e-5 * (1 + abs(lo))
    gr = cpu(grad).astype(np.float64)
    # every gradient element against the float64 oracle, tensor by tensor, on the rows whose spline inputs stay clear of the knots
    from oracle import spline_grad as sg
    from tests import spline_grad_check as sgc
    away = sg.log_probs(o.w, P, x, D, H, 2, 8, 3.0, margins=True)[2] > 1e-5
    assert away.sum() >= 45
    g64 = sg.loss_grad(o.w, P, x[away], D, H, 2, 8, 3.0)[1]
    sgc.assert_grad_close(cpu(sp.loss_grad(x[away])[1]), g64, sg.layer_shapes(D, H, 2, 8), sgc.GPU_RTOL_T, sgc.GPU_FLOOR,
                          'd%d h%d' % (D, H))
    ga, gb = cpu(sp.loss_grad(x[:20])[1]).astype(np.float64), cpu(sp.loss_grad(x[20:])[1]).astype(np.float64)
    assert np.max(np.abs(20 * ga + 30 * gb - 50 * gr)) < 2e-4 * 50 * np.max(np.abs(gr))
    # a short training run moves the loss down
    perms = torch.stack([torch.randperm(80) for _ in range(4)]).int()
    res = sp.train_epochs(x0[:80], x0[80:], perms, None, seed=1, jitter=0.01, batch=100, max_epochs=4, patience=50)
    l = res['losses'].numpy()
    assert np.all(np.isfinite(l)) and l[-1, 0] < l[0, 0]


@pytest.mark.parametrize('D', [6, 50])
def test_spline_training_stops_when_patience_runs_out_and_queued_launches_do_nothing(hip, D):
    """Trainer.train's early stopping (nnest/trainer.py:205-209, :223-232) on the spline flow: the epoch books live on the device
    and the host queues launches ahead of them, so the launches queued past the stop must leave weights, Adam state and step count
    alone (every training kernel looks at the stop flag in front of its first store -- round 6: behind its first loads).  A run with
    a validation set that gets worse: it ends `patience` epochs after its best epoch, restores that epoch's weights, and is -- bit
    for bit -- the run that was only ever asked for that many epochs."""
    rng = np.random.RandomState(1)
    X = rng.uniform(-1, 1, size=(240, D)).astype(np.float32)
    Xv = (rng.uniform(-1, 1, size=(30, D)) * 2.5).astype(np.float32)   # off-distribution: the validation loss turns around early
    E = 120
    perm = torch.stack([torch.randperm(240, generator=torch.Generator().manual_seed(e)) for e in range(E)]).int()
    kw = dict(seed=1, jitter=0.0, batch=100, patience=4, lr=5e-3)

    def run(max_epochs):
        sp = hip.HipSpline(D, 16, 3, seed=5)
        res = sp.train_epochs(X, Xv, perm[:max_epochs], None, max_epochs=max_epochs, **kw)
        return sp, res

    sp, res = run(E)
    assert res['stopped'] and res['epochs_run'] < E - 16          # (the host runs up to two chunks of eight epochs ahead)
    assert res['epochs_run'] == res['best_epoch'] + 4
    losses = res['losses'].numpy()[:res['epochs_run']]
    assert abs(losses[res['best_epoch'] - 1, 1] - res['best_validation_loss']) < 1e-7
    assert np.all(losses[res['best_epoch']:, 1] >= res['best_validation_loss'])
    sp2, res2 = run(res['epochs_run'])                             # nothing queued past the stop
    assert res2['epochs_run'] == res['epochs_run'] and res2['best_epoch'] == res['best_epoch']
    assert np.array_equal(res2['losses'].numpy()[:res['epochs_run']], losses)
    assert np.array_equal(sp2.store_packed(), sp.store_packed())   # the best epoch's weights, the same bits
    # the optimiser's state too: one more epoch from either lands on the same weights
    for s_ in (sp, sp2):
        s_.train_epochs(X, Xv, perm[:1], None, max_epochs=1, **kw)
    assert np.array_equal(sp2.store_packed(), sp.store_packed())
