"""[UNPINNED] The slice proposal on a regression likelihood of user data, NVP side (include/nnest_hip.h nnest_slice_glm_steps;
nnest_slice_glm.hip slice_glm_kernel<U, FAM>; HipNVP.slice_steps(like_glm=...); slice_rounds(like_glm=...)).  Build-defined: the
reference proposes random-walk Metropolis moves only (nnest/sampler.py:310-316).  The cases, the oracle's likelihood, the start and the
checks are tests/slice_glm_check.py's; tests/test_slice_glm_check.py shows on the CPU that they fail a wrong kernel.

Every table row: the kernel against oracle.slice_sample on the kernel's own directions (fill_slice_noise) -- near share first, then
counters and states (`compare`), the returned logL against glm_check.exact at the kernel's own x within glm_check.bound, the box, L*
and the counters' order; the recorded-noise launch, the same launch again and a shard of it, bit for bit.  Then the safe rule, the
skipped likelihood (a start with L* = -1e300 and one with the table's L*: the counters are the oracle's, which skips nothing), the
round driver with the device likelihood, and the refusals.  One RATIO line per case.  Run with  pytest -m gpu."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc   # (checker only)
from tests import glm_check as gk
from tests import slice_glm_check as sg
from tests import slice_like_check as sl
from tests.fused_like_check import bits_equal, units

pytestmark = pytest.mark.gpu

SEED, OFF = 4242, 100
CASES = sg.NVP_TABLE + sg.NVP_EXTRA
KEYS = ('hist_x', 'x', 'n_eval', 'n_call', 'n_move', 'moved')


def cpu(t):
    return t.detach().cpu().numpy()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fused(net, c, z0, l0, star, data=None, noise=None, form=None, walker_offset=OFF, identity=False):
    """one slice_steps(like_glm=...) launch from (z0, l0): what it returned as numpy arrays (z: the final z, updated in place), logl"""
    z, logl = cuda(z0), cuda(l0)
    sd, mu = (None, None) if identity else sg.affine_of(c)
    res = net.slice_steps(None, 1.0, z, logl, star, sg.width_of(c.D), c.S, seed=SEED, walker_offset=walker_offset, history=True, noise=noise,
                          form=form, like_glm=sg.data_of(c) if data is None else data, t_std=sd, t_mean=mu)
    k = {key: cpu(res[key]) for key in KEYS}
    k['z'] = cpu(z)
    return k, cpu(logl)


def same_bits(a, b, keys=KEYS + ('z',), rows=slice(None)):
    return all(a[k].dtype == b[k].dtype and np.array_equal(np.ascontiguousarray(a[k][rows]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in keys)


def note(kernel, inst, c, C, near, same, **ratios):
    print('RATIO %-28s %-12s %-26s C %2d S %d  near %.3f  agree %.3f  %s' % (
        kernel, inst, sg.case_id(c), C, c.S, near, same.mean(), '  '.join('%s %.3g' % kv for kv in ratios.items())))


_FLOWS, _RUNS = {}, {}


def solo_flow(D):
    from nnest_amd import flow
    if D not in _FLOWS:
        nvp = flow.HipNVP(D, 16, 3, 1, seed=3)
        _FLOWS[D] = (nvp, orc.NVP(D, 16, 3, 1, nvp.store_packed()))
    return _FLOWS[D]


def oracle_run(c, star_kind='table', safe=False):
    """(z0, l0, star, dz on the device, oracle result, margins) of a case on the kernel's own directions; star_kind 'free': L* =
    -1e300 from the same start; safe: under the descriptor with NaN offsets.  Computed once, shared, never changed"""
    key = (c, star_kind, safe)
    if key not in _RUNS:
        nvp, o = solo_flow(c.D)
        z0, l0, star = sg.start(c, lambda u: cpu(nvp.forward(u)[0]))
        if star_kind == 'free':
            star = -1e300
        dz = nvp.fill_slice_noise(c.S, len(l0), seed=SEED, walker_offset=OFF)
        margins = np.empty((c.S, len(l0)))
        ev = (lambda x: sg.exact_logl(c, x, sg.non_finite_data(c))) if safe else None
        ref = sg.slice_sample(o, c, z0, l0, star, cpu(dz), SEED, OFF, evaluate=ev, margins=margins)
        _RUNS[key] = (z0, l0, star, dz, ref, margins)
    return _RUNS[key]


def test_launch_has_the_new_argument():
    """(the parent commit fails here and in every test below: slice_steps has no like_glm)"""
    import inspect
    from nnest_amd import flow
    assert {'like_glm', 't_std', 't_mean'} <= set(inspect.signature(flow.HipNVP.slice_steps).parameters)
    assert solo_flow(2)[0].slice_glm_refusal() is None and solo_flow(2)[0].slice_glm_refusal(2) is None


@pytest.mark.parametrize('c', CASES, ids=[sg.case_id(c) for c in CASES])
def test_kernel_vs_oracle(c):
    nvp, o = solo_flow(c.D)
    z0, l0, star, dz, ref, margins = oracle_run(c)
    C = len(l0)
    inst = '<%d, %d>' % (units(c.D), sg.FAM[c.family])
    k, logl = fused(nvp, c, z0, l0, star)
    same, near, r_x, r_ll = sg.hold(c, k, logl, ref, margins, l0, star, what='slice_glm_kernel %s %s' % (inst, sg.case_id(c)))
    assert np.array_equal(k['moved'], (k['hist_x'][:, 0] != k['x']).all(1))   # NNEST_MH_ALL_MOVED: the first x against the last
    note('slice_glm_kernel', inst, c, C, near, same, x=r_x, logL=r_ll, n_eval=k['n_eval'].mean(), n_call=k['n_call'].mean())
    k2, logl2 = fused(nvp, c, z0, l0, star, noise=dz)   # the recorded-noise path replays the in-kernel draws
    assert same_bits(k, k2) and np.array_equal(logl, logl2), 'recorded noise'
    k3, logl3 = fused(nvp, c, z0, l0, star)             # the same launch twice
    assert same_bits(k, k3) and np.array_equal(logl, logl3), 'the same launch twice'
    h = C // 2                                           # a shard: the second half of the walkers, at their own offset
    k4, logl4 = fused(nvp, c, z0[h:], l0[h:], star, walker_offset=OFF + h)
    assert same_bits(k, k4, rows=slice(h, None)) and np.array_equal(logl[h:], logl4), 'shard'


def test_null_t_is_the_identity():
    """t_std = t_mean = NULL against the vectors (1, 0): the same bits"""
    c = sg.Case('logistic', 2, 257, 1.0, 3, False)
    nvp, o = solo_flow(c.D)
    z0, l0, star = sg.start(c, lambda u: cpu(nvp.forward(u)[0]))
    a, la = fused(nvp, c, z0, l0, star)
    b, lb = fused(nvp, c, z0, l0, star, identity=True)
    assert same_bits(a, b) and np.array_equal(la, lb) and a['n_move'].sum() > 0


SAFE_CASES = [sg.NVP_TABLE[0], sg.NVP_TABLE[2]]   # U = 1 (two pass groups) and U = 3 (the weights in LDS)


@pytest.mark.parametrize('c', SAFE_CASES, ids=[sg.case_id(c) for c in SAFE_CASES])
def test_non_finite_logl_counts_as_minus_1e100(c):
    """NaN offsets (the library refuses a non-finite logl0 at the entry; the arrays' contents are the caller's) from a start with
    finite logl: every candidate's logL is non-finite, counts as -1e100 and fails logL > L*.  No update moves; z, every state and logl
    keep their bits; n_call and n_eval are the oracle's"""
    nvp, o = solo_flow(c.D)
    z0, l0, star, dz, ref, margins = oracle_run(c, safe=True)
    k, logl = fused(nvp, c, z0, l0, star, data=sg.non_finite_data(c))
    sl.check_nothing_moves(k, ref, z0, l0, k['z'], logl, what=sg.case_id(c))
    assert not k['moved'].any() and k['n_call'].sum() > 0
    print('SAFE %s: %d walkers, %d candidates, %d with a likelihood, none moved' % (sg.case_id(c), len(l0), int(k['n_eval'].sum()), int(k['n_call'].sum())))


SKIP_CASES = [sg.NVP_TABLE[1], sg.NVP_TABLE[4]]


@pytest.mark.parametrize('c', SKIP_CASES, ids=[sg.case_id(c) for c in SKIP_CASES])
def test_the_skipped_likelihood_shows_in_no_counter(c):
    """the oracle evaluates the likelihood at every candidate, the kernel only where pre holds.  From a start with L* = -1e300 (every
    candidate with pre is inside: the likelihood decides nothing but is still the logL returned) and from the table's L*: n_eval and
    n_call are the oracle's on every walker the oracle did not have within 2e-4 of a threshold, and there are candidates without pre"""
    nvp, o = solo_flow(c.D)
    for kind in ('free', 'table'):
        z0, l0, star, dz, ref, margins = oracle_run(c, kind)
        k, logl = fused(nvp, c, z0, l0, star)
        what = 'skip %s L* %s' % (sg.case_id(c), kind)
        same, _ = sl.compare(k, ref, margins, what=what)
        firm = np.min(margins, axis=0) >= sl.TOL
        assert firm.mean() >= sl.AGREE, what
        for key in ('n_eval', 'n_call', 'n_move'):
            np.testing.assert_array_equal(k[key][firm], ref[key][firm], err_msg='%s %s' % (what, key))
        assert ref['n_call'].sum() < ref['n_eval'].sum(), what
        sg.check_logl_of_own_x(c, logl, k['x'], k['n_move'], l0, what=what)
        print('SKIP %-26s L* %-5s: n_eval %d, n_call %d (%.2f of the candidates needed a likelihood)' % (
            sg.case_id(c), kind, int(k['n_eval'].sum()), int(k['n_call'].sum()), k['n_call'].sum() / float(k['n_eval'].sum())))


def rounds(f, c, z0, l0, star, noise=None):
    from nnest_amd.slice_rounds import slice_rounds
    z, logl = cuda(z0), cuda(l0)
    sd, mu = sg.affine_of(c)
    res = slice_rounds(f, z, logl, star, sg.width_of(c.D), c.S, seed=SEED, walker_offset=OFF, history=True, noise=noise, like_glm=sg.data_of(c),
                       t_std=sd, t_mean=mu)
    k = {key: cpu(res[key]) for key in KEYS}
    k['z'] = cpu(z)
    return k, cpu(logl)


def test_rounds_with_the_device_likelihood_vs_the_same_oracle_run():
    c = sg.NVP_EXTRA[0]
    nvp, o = solo_flow(c.D)
    z0, l0, star, dz, ref, margins = oracle_run(c)
    k, logl = rounds(nvp, c, z0, l0, star)
    same, near, r_x, r_ll = sg.hold(c, k, logl, ref, margins, l0, star, what='slice_rounds like_glm %s' % sg.case_id(c))
    note('slice_rounds like_glm', 'nvp', c, len(l0), near, same, x=r_x, logL=r_ll)
    k2, logl2 = rounds(nvp, c, z0, l0, star, noise=dz)
    assert same_bits(k, k2) and np.array_equal(logl, logl2)


def test_refusals_raise_without_a_launch():
    from nnest_amd import _lib, flow
    from nnest_amd.maf import HipMAF
    c = sg.NVP_EXTRA[0]
    nvp, _ = solo_flow(c.D)
    data = sg.data_of(c)
    z = torch.full((8, c.D), 0.25, dtype=torch.float32, device='cuda')
    logl = torch.full((8,), -3.5, dtype=torch.float64, device='cuda')
    kept = lambda: bool(torch.all(z == 0.25)) and bool(torch.all(logl == -3.5))
    args = (z, logl, -1e9, 0.5, 2)
    with pytest.raises(_lib.NnestHipError, match="the likelihood's D=5 is not the flow's x_dim=%d" % c.D) as e:
        nvp.slice_steps(None, 1.0, *args, like_glm=gk.make_like(5, 30, 'logistic', 1).hip_like_glm)
    assert e.value.code == 1 and 'D=5' in (nvp.slice_glm_refusal(5) or '')
    with pytest.raises(ValueError, match="family='probit'"):
        nvp.slice_steps(None, 1.0, *args, like_glm=dict(data, family='probit'))
    with pytest.raises(_lib.NnestHipError, match='glm: family=7'):
        nvp.slice_steps(None, 1.0, *args, like_glm=dict(data, family=7))
    with pytest.raises(_lib.NnestHipError, match='glm: n=65537'):
        nvp.slice_steps(None, 1.0, *args, like_glm=dict(data, n=65537))
    with pytest.raises(_lib.NnestHipError, match='max_shrink=61'):
        nvp.slice_steps(None, 1.0, *args, like_glm=data, max_shrink=61)
    with pytest.raises(ValueError, match='like_glm goes with like_id=None'):
        nvp.slice_steps(0, 5.0, *args, like_glm=data)
    with pytest.raises(ValueError, match='both or neither'):
        nvp.slice_steps(None, 1.0, *args, like_glm=data, t_std=np.ones(c.D))
    maf = HipMAF(c.D, 16, 3, seed=1)
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        maf.slice_steps(None, 1.0, *args, like_glm=data)
    with pytest.raises(NotImplementedError):
        maf.slice_glm_refusal()
    other = flow.HipNVP(c.D, 32, 3, 1, seed=3)   # (not the default shape)
    assert 'hidden 16' in other.slice_glm_refusal()
    with pytest.raises(_lib.NnestHipError, match='hidden 16') as e:
        other.slice_steps(None, 1.0, *args, like_glm=data)
    assert e.value.code == _lib.NNEST_E_UNSUPPORTED
    assert kept()
