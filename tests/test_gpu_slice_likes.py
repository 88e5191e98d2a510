"""[UNPINNED] The slice kernels with EVERY fused likelihood at every instantiation (the slice proposal is build-defined: the reference
proposes random-walk Metropolis moves only, nnest/sampler.py:310-316).  slice_kernel_solo<U, LK> (nnest_slice_steps), the wave, team
and pair forms of nnest_spline_slice_steps <NT, NH> and the round driver's device route, each against oracle.slice_sample with the
likelihood's parameters, on the kernel's own directions (fill_slice_noise) and the shared Philox uniforms.  The cases, the start and
the checks are tests/slice_like_check.py's; tests/test_slice_like_check.py shows on the CPU that they fail a wrong likelihood.

Every case asserts its near share (the share of walkers the oracle itself had within 2e-4 of a threshold) before it compares, then:
counters and states (`compare`), the returned logL against the float64 likelihood of the kernel's own x, the box, L*, the counters'
order and the bit-for-bit replay on recorded directions.  One RATIO line per case: worst error / bound and the instantiation.
Run with  pytest -m gpu."""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import oracle as orc   # (checker only)
from tests import fused_like_check as fl
from tests import slice_like_check as sl
from tests.test_gpu_fused_likes import SPLINE_KEYS, spline_flow, spline_tols
from tests.test_gpu_slice_rounds import make as make_flow

pytestmark = pytest.mark.gpu

SEED, OFF = 4242, 100


def cpu(t):
    return t.detach().cpu().numpy()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def note(kernel, inst, c, C, near, same, **ratios):
    print('RATIO %-22s %-14s %-12s x_dim %3d  C %2d S %d  near %.3f  agree %.3f  %s' % (
        kernel, inst, c.name, c.D, C, c.S, near, same.mean(), '  '.join('%s %.3g' % kv for kv in ratios.items())))


def width_of(D):
    return 2.0 / np.sqrt(D)


def fused(net, c, params, z0, l0, star, form=None, noise=None):
    """one slice_steps launch from (z0, l0): what it returned as numpy arrays (z: the walker's final z, updated in place), and logl"""
    z, logl = cuda(z0), cuda(l0)
    res = net.slice_steps(fl.LIKES[c.name]['id'], c.scale, z, logl, star, width_of(c.D), c.S, seed=SEED, walker_offset=OFF, history=True,
                          like_params=params, form=form, noise=noise)
    k = {key: cpu(res[key]) for key in ('hist_x', 'x', 'n_eval', 'n_call', 'n_move', 'moved')}
    k['z'] = cpu(z)
    return k, cpu(logl)


def oracle_of_case(o, c, params, z0, l0, star, dz):
    margins = np.empty((c.S, len(l0)))
    t = time.time()
    ref = orc.slice_sample(o, c.name, c.scale, z0, l0, star, width_of(c.D), dz, SEED, walker_offset=OFF, margins=margins,
                           like_params=list(params) if params else None)
    return ref, margins, time.time() - t


def hold(kernel, inst, c, k, logl, ref, margins, l0, star, extra=None):
    """the checks of one kernel output, in order; the near share first, from the oracle alone"""
    what = '%s %s %s' % (kernel, inst, sl.case_id(c))
    near = sl.near_share(margins)
    assert near <= 1.0 - sl.AGREE, '%s: near share %.3g: the 80 %% criterion could fail a correct kernel' % (what, near)
    same, r_x = sl.compare(k, ref, margins, what=what)
    r_ll = sl.check_logl_of_own_x(c, logl, k['x'], k['n_move'], l0, what=what)
    assert np.all(fl.bits_equal(k['x'], k['hist_x'][:, -1])), what
    sl.check_in_box_above_star(k, logl, star, what=what)
    note(kernel, inst, c, len(l0), near, same, x=r_x, logL=r_ll, **(extra or {}))
    return same


def same_bits(a, b, keys=('hist_x', 'x', 'z', 'n_eval', 'n_call', 'n_move', 'moved')):
    return all(a[k].dtype == b[k].dtype and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in keys)


# ---- the solo kernel ---------------------------------------------------------------------------------------------------------------------
def solo_flow(D):
    from nnest_amd import flow
    nvp = flow.HipNVP(D, 16, 3, 1, seed=3)
    return nvp, orc.NVP(D, 16, 3, 1, nvp.store_packed())


SOLO_CASES = sl.SOLO_TABLE + sl.SOLO_EXTRA


@pytest.mark.parametrize('c', SOLO_CASES, ids=[sl.case_id(c) for c in SOLO_CASES])
def test_solo_kernel_vs_oracle(c):
    nvp, o = solo_flow(c.D)
    z0, l0, star = sl.start(c, lambda u: cpu(nvp.forward(u)[0]))
    C = len(l0)
    dz = nvp.fill_slice_noise(c.S, C, seed=SEED, walker_offset=OFF)
    k, logl = fused(nvp, c, c.params, z0, l0, star)
    ref, margins, _ = oracle_of_case(o, c, c.params, z0, l0, star, cpu(dz))
    hold('slice_kernel_solo', '<%d, %d>' % (fl.units(c.D), sl.lk(c.name)), c, k, logl, ref, margins, l0, star)
    k2, logl2 = fused(nvp, c, c.params, z0, l0, star, noise=dz)   # the recorded-noise path replays the same launch
    assert same_bits(k, k2) and np.array_equal(logl, logl2)


# ---- the safe rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['solo-d%d' % D for D in sl.SAFE_SOLO_DIMS] + ['spline-d5', 'rounds-d5'])
def test_non_finite_logl_counts_as_minus_1e100(route):
    """shell with a NaN width (check_like admits it) from a start with finite logl: every candidate's logL is non-finite, so no
    update moves; z, x and logl keep their bits, n_move is 0, n_call and n_eval are the oracle's"""
    kind, D = route.split('-d')
    c = sl.case('shell', int(D))
    C = 27 if kind != 'solo' else None
    if kind == 'solo':
        net, o = solo_flow(c.D)
    elif kind == 'spline':
        net, o = spline_flow(c.D, 16, 27)
    else:
        net, twin = make_flow('cholesky', c.D)
        o = twin()
    z0, l0, star = sl.start(c, lambda u: cpu(net.forward(u)[0]), count=C)
    dz = solo_flow(c.D)[0].fill_slice_noise(c.S, len(l0), seed=SEED, walker_offset=OFF)   # (the directions are flow-independent)
    if kind == 'rounds':
        k, logl = rounds(net, c, sl.NAN_PARAMS, z0, l0, star, 'device')
    else:
        k, logl = fused(net, c, sl.NAN_PARAMS, z0, l0, star)
    ref, margins, _ = oracle_of_case(o, c, sl.NAN_PARAMS, z0, l0, star, cpu(dz))
    sl.check_nothing_moves(k, ref, z0, l0, k['z'], logl, what=route)
    assert not k['moved'].any()
    print('SAFE %s: %d walkers, %d candidates, none moved' % (route, len(l0), int(k['n_eval'].sum())))


# ---- the spline kernels ----------------------------------------------------------------------------------------------------------------------
# (likelihood, x_dim, hidden, walkers, updates, forms).  Rosenbrock at the keys no other test launches (31, 41, 22); the other six
# spread over all six keys; wave and team at every key, pair at NT >= 2.  Walkers are ragged against 8 and 16; C and S shrink with
# the oracle's cost.  Measured on the CPUs of an MI355X host, the oracle's part of a case: 2.7 to 2.9 s at key 41 (21 walkers, 3
# updates, about 330 evaluations at 9 ms), 0.7 s at key 31 (27 walkers, 4 updates), 0.2 s at keys 21 and 22, below 0.1 s at 11 and 12
SPLINE_CASES = [('rosenbrock', 70, 16, 27, 4, ('wave', 'pair')), ('rosenbrock', 128, 16, 21, 3, ('team', 'pair')),
                ('rosenbrock', 40, 32, 37, 4, ('wave', 'team')), ('eggbox', 2, 16, 45, 4, ('wave',)), ('double_shell', 5, 16, 45, 4, ('team',)),
                ('gaussmix', 8, 32, 45, 4, ('wave', 'team')), ('shell', 40, 16, 37, 4, ('wave', 'team', 'pair')),
                ('gaussian', 40, 32, 37, 4, ('pair',)), ('himmelblau', 70, 16, 27, 4, ('team',)), ('gaussian', 128, 16, 21, 3, ('wave',))]


def test_spline_cases_reach_every_key_and_form():
    keys = lambda pick: {SPLINE_KEYS[D, H] for n, D, H, _, _, _ in SPLINE_CASES if pick(n)}
    assert keys(lambda n: n == 'rosenbrock') == {31, 41, 22}
    assert keys(lambda n: n != 'rosenbrock') == {11, 21, 31, 41, 12, 22}
    assert {n for n, *_ in SPLINE_CASES} == set(fl.LIKES)
    reached = {(SPLINE_KEYS[D, H], f) for _, D, H, _, _, forms in SPLINE_CASES for f in forms}
    assert reached == {(k, f) for k in (11, 21, 31, 41, 12, 22) for f in ('wave', 'team')} | {(k, 'pair') for k in (21, 31, 41, 22)}
    for _, D, H, C, _, _ in SPLINE_CASES:
        assert 10 * fl.units(D) + H // 16 == SPLINE_KEYS[D, H] and C % 8 != 0 and C % 16 != 0


@pytest.mark.parametrize('name,D,H,C,S,forms', SPLINE_CASES, ids=['%s-d%d-h%d' % c[:3] for c in SPLINE_CASES])
def test_spline_kernels_vs_oracle(name, D, H, C, S, forms):
    """one oracle run per case, every listed form of the kernel against it.  Besides `compare`: the final x against the oracle's
    inverse of the kernel's own final z, within tests/test_gpu_fused_likes.py's spline_tols for the key"""
    c = sl.case(name, D, S)
    key = SPLINE_KEYS[D, H]
    sp, o = spline_flow(D, H, C)
    z0, l0, star = sl.start(c, lambda u: cpu(sp.forward(u)[0]), count=C)
    dz = sp.fill_slice_noise(S, C, seed=SEED, walker_offset=OFF)
    ref, margins, secs = oracle_of_case(o, c, c.params, z0, l0, star, cpu(dz))
    print('spline key %d %s: the oracle took %.1f s (%d evaluations)' % (key, sl.case_id(c), secs, int(ref['n_eval'].sum())))
    for form in forms:
        assert sp.slice_form_for(C, form) == form
        k, logl = fused(sp, c, c.params, z0, l0, star, form=form)
        _, x_tol = spline_tols(key, o, k['z'])
        xo, _ = o.inverse(k['z'])
        r_own = float(np.max(np.abs(k['x'] - xo) / x_tol(xo)))
        assert r_own <= 1.0, (form, r_own)
        hold('spline_slice_%s' % form, 'key %d' % key, c, k, logl, ref, margins, l0, star, extra=dict(x_of_own_z=r_own))
        k2, logl2 = fused(sp, c, c.params, z0, l0, star, form=form, noise=dz)
        assert same_bits(k, k2) and np.array_equal(logl, logl2), form


# ---- the round driver, device route ---------------------------------------------------------------------------------------------------------
def rounds(f, c, params, z0, l0, star, route, noise=None):
    from nnest_amd.slice_rounds import slice_rounds
    z, logl = cuda(z0), cuda(l0)
    if route == 'device':
        like = dict(like_id=fl.LIKES[c.name]['id'], like_scale=c.scale, like_params=params)
    else:   # the float64 likelihood of the same parameters on the float32 like_scale x, as a host callable
        like = dict(loglike=lambda x: fl.exact_logl(c.name, fl.T32(x, np.float32(c.scale), np.float32(0.0)), params))
    res = slice_rounds(f, z, logl, star, width_of(c.D), c.S, seed=SEED, walker_offset=OFF, history=True, noise=noise, **like)
    k = {key: cpu(res[key]) for key in ('hist_x', 'x', 'n_eval', 'n_call', 'n_move', 'moved')}
    k['z'] = cpu(z)
    return k, cpu(logl)


ROUNDS_CASES = [('gaussian', 'maf', 10), ('double_shell', 'nvp_h32_translate', 6), ('shell', 'cholesky', 5)]


@pytest.mark.parametrize('name,kind,D', ROUNDS_CASES, ids=['%s-%s-d%d' % c for c in ROUNDS_CASES])
def test_rounds_device_route_vs_oracle_and_host_route(name, kind, D):
    c = sl.case(name, D)
    f, twin = make_flow(kind, D)
    z0, l0, star = sl.start(c, lambda u: cpu(f.forward(u)[0]), count=45)
    o = twin()
    C = len(l0)
    dz = solo_flow(D)[0].fill_slice_noise(c.S, C, seed=SEED, walker_offset=OFF)   # (nnest_slice_fill_noise: flow-independent)
    k, logl = rounds(f, c, c.params, z0, l0, star, 'device')
    ref, margins, _ = oracle_of_case(o, c, c.params, z0, l0, star, cpu(dz))
    same = hold('slice_rounds device', kind, c, k, logl, ref, margins, l0, star)
    k2, logl2 = rounds(f, c, c.params, z0, l0, star, 'device', noise=dz)
    assert same_bits(k, k2) and np.array_equal(logl, logl2)
    # the host route with the float64 likelihood: the same decisions for the walkers `compare` holds (one the oracle had within
    # 2e-4 of a threshold may be turned by the two likelihoods' rounding alone)
    h, logl_h = rounds(f, c, c.params, z0, l0, star, 'host')
    firm = same & (np.min(margins, axis=0) >= sl.TOL)
    assert firm.mean() >= sl.AGREE
    for key in ('n_eval', 'n_call', 'n_move'):
        np.testing.assert_array_equal(h[key][firm], k[key][firm], err_msg=key)
    assert np.max(np.abs(h['z'][firm] - k['z'][firm]) / (1.0 + np.abs(k['z'][firm]))) < sl.TOL
    sl.check_logl_of_own_x(c, logl_h, h['x'], h['n_move'], l0, what='host route')


# ---- the sampler's wiring ------------------------------------------------------------------------------------------------------------------
def like_classes(D):
    from nnest_amd import likelihoods as L
    return {'gaussian': L.Gaussian(D, 0.5), 'shell': L.GaussianShell(D, sigma=0.1, rshell=2.0, center=0.0),
            'double_shell': L.DoubleGaussianShell(D, sigmas=(0.1, 0.2), rshells=(2.0, 1.5), centers=(-1.0, 1.0))}


@pytest.mark.parametrize('flow', ['nvp', 'spline', 'maf'])
@pytest.mark.parametrize('name', ['gaussian', 'shell', 'double_shell'])
def test_sampler_hands_the_parameters_to_the_slice_kernels(tmp_path, name, flow):
    """NestedSampler(mcmc_proposal='slice') with a likelihood class that has parameters, from prior points above a quantile L*, no
    training and no run: one _mcmc_sample call (the round driver's device route, for every flow: it returns the whole history) and
    one _mcmc_endpoints_fused call, the batch of a run (the solo kernel with 'nvp', the spline kernel with 'spline', the round driver
    with 'maf').  The loglikes they return are the class's own loglike_rows at the samples they return, within logl_bound, and above
    L*: parameters that arrive zeroed, reordered or with another scale are off by O(1)."""
    from nnest_amd.nested import NestedSampler
    D, S = 5, 4
    c = sl.case(name, D)
    like = like_classes(D)[name]
    assert like.hip_like_id == fl.LIKES[name]['id'] and tuple(like.hip_like_params) == pytest.approx(c.params)
    np.random.seed(2)
    torch.manual_seed(2)
    s = NestedSampler(D, like, transform=lambda x: c.scale * x, log_dir=str(tmp_path), num_live_points=64, log_level=30, flow=flow,
                      mcmc_proposal='slice')
    assert s._fused_like_id == like.hip_like_id and tuple(s._fused_like_params) == tuple(like.hip_like_params)
    assert s._linear_scale == c.scale
    u = np.random.RandomState(1).uniform(-0.6, 0.6, size=(sl.DRAWS, D))
    l = np.asarray(like.loglike_rows(c.scale * u), np.float64)
    star = float(np.quantile(l, sl.QUANTILE))
    u, l = u[l > star], l[l > star]
    netG = s.trainer.netG
    launched = []
    if hasattr(netG, 'slice_steps'):
        inner = netG.slice_steps
        netG.slice_steps = lambda *a, **kw: (launched.append(kw.get('like_params')), inner(*a, **kw))[1]

    def class_logl(x32):
        tx = fl.T32(np.asarray(x32, np.float32), np.float32(c.scale), np.float32(0.0)).astype(np.float64)
        return np.asarray(like.loglike_rows(tx), np.float64)

    samples, latent, derived, loglikes, scale, ncall = s._mcmc_sample(S, init_samples=u, init_loglikes=l, loglstar=star, seed=5)
    assert samples.shape == (len(l), S + 1, D) and loglikes.shape == (len(l), S + 1) and ncall > 0 and not launched
    moved = ~np.all(fl.bits_equal(samples[:, 1:], samples[:, :1]), axis=2)   # (a state that is the start holds the caller's logl)
    assert moved.mean() > 0.9
    want = class_logl(samples[:, 1:][moved])
    r_hist = float(np.max(np.abs(loglikes[:, 1:][moved] - want) / fl.logl_bound(want)))
    assert r_hist <= 1.0, r_hist
    assert np.all(loglikes > star) and np.all(np.abs(samples) <= 1.0)
    ends, _, ncall = s._mcmc_endpoints_fused(S, 1.0 / np.sqrt(D), False, u, l, star, 0, 6)
    ends = cpu(ends)
    x, ll, mv = ends[:, :D].astype(np.float32), ends[:, D], ends[:, D + 1] > 0
    assert len(launched) == (0 if flow == 'maf' else 1) and ncall > 0
    if launched:
        assert tuple(launched[0]) == tuple(like.hip_like_params)
    assert mv.mean() > 0.9
    want = class_logl(x[mv])
    r_end = float(np.max(np.abs(ll[mv] - want) / fl.logl_bound(want)))
    assert r_end <= 1.0, r_end
    assert np.all(ll > star) and np.all(np.abs(x) <= 1.0)
    print('RATIO %-22s %-14s %-12s x_dim %3d  history logL %.3g  endpoints logL %.3g' % ('NestedSampler slice', flow, name, D, r_hist, r_end))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def raw_slice_call(net, spline, like_id, C=8):
    """nnest_slice_steps / nnest_spline_slice_steps on guarded buffers: (rc, message, the buffers, the guards)"""
    from nnest_amd import _lib
    D = net.D
    z = torch.full((C, D), 0.25, dtype=torch.float32, device='cuda')
    x = torch.full((C, D), -7.0, dtype=torch.float32, device='cuda')
    logl = torch.full((C,), -3.5, dtype=torch.float64, device='cuda')
    cnt = [torch.full((C,), -77, dtype=torch.int32, device='cuda') for _ in range(3)]
    lk = _lib.like_spec(like_id, 5.0, None)
    form = (0,) if spline else ()
    rc = net._sym['slice'](net._h, ctypes.byref(lk), _lib.ptr(z), _lib.ptr(x), _lib.ptr(logl), -1e9, 0.5, 2, C, 8, 32, *form, None, 1, 0,
                           None, _lib.ptr(cnt[0]), _lib.ptr(cnt[1]), _lib.ptr(cnt[2]), _lib.current_stream(net.device))
    msg = _lib.load().nnest_hip_last_error()
    torch.cuda.synchronize()
    kept = (bool(torch.all(z == 0.25)) and bool(torch.all(x == -7.0)) and bool(torch.all(logl == -3.5))
            and all(bool(torch.all(t == -77)) for t in cnt))
    return rc, (msg.decode() if msg else ''), kept


REFUSALS = [('eggbox', 3, 'Eggbox is defined for x_dim = 2'), ('gaussmix', 1, 'GaussianMix needs x_dim >= 2'), (99, 3, 'unknown likelihood id 99'),
            (-1, 3, 'unknown likelihood id -1')]


@pytest.mark.parametrize('like,D,msg', REFUSALS, ids=['%s-d%d' % r[:2] for r in REFUSALS])
def test_a_likelihood_the_kernels_do_not_take_is_refused(like, D, msg):
    """at nnest_slice_steps, nnest_spline_slice_steps and slice_rounds(like_id=...): NNEST_E_ARG with the reason, and z, x, logl and
    the counters keep their guard pattern.  (A spline flow has x_dim >= 2, so GaussianMix at x_dim 1 cannot reach its kernel.)"""
    from nnest_amd import _lib, flow
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.slice_rounds import slice_rounds
    from nnest_amd.spline import HipSpline
    like_id = fl.LIKES[like]['id'] if isinstance(like, str) else like
    rc, text, kept = raw_slice_call(flow.HipNVP(D, 16, 3, 1, seed=3), False, like_id)
    assert rc == 1 and msg in text and kept, (rc, text, kept)
    if D >= 2:
        rc, text, kept = raw_slice_call(HipSpline(D, 16, 3, seed=3), True, like_id)
        assert rc == 1 and msg in text and kept, (rc, text, kept)
    else:
        with pytest.raises(_lib.NnestHipError):
            HipSpline(D, 16, 3, seed=3)
    ch = HipCholesky(D)
    z = torch.full((8, D), 0.25, dtype=torch.float32, device='cuda')
    logl = torch.full((8,), -3.5, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.NnestHipError) as ei:
        slice_rounds(ch, z, logl, -1e9, 0.5, 2, like_id=like_id, like_scale=5.0, seed=1)
    assert ei.value.code == 1 and msg in str(ei.value)
    assert bool(torch.all(z == 0.25)) and bool(torch.all(logl == -3.5))
    # the Python entry raises the same refusal
    nvp = flow.HipNVP(D, 16, 3, 1, seed=3)
    with pytest.raises(_lib.NnestHipError) as ei:
        nvp.slice_steps(like_id, 5.0, z, logl, -1e9, 0.5, 2)
    assert ei.value.code == 1 and msg in str(ei.value)
    assert bool(torch.all(z == 0.25)) and bool(torch.all(logl == -3.5))
