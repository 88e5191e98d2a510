"""The slice proposal keeps its target: every device implementation (the solo kernel of the default NVP, the spline kernel in its
wave, team and pair forms, the round driver for every other flow and both likelihood routes) started from an EXACT uniform sample of
A = {x in [-1, 1]^D : logL(x) > L*} must leave it uniform on A and must be reversible (tests/slice_invariance.py).  This holds
whatever the flow, so the flows are seeded random (non-identity) ones, with the identity NVP as a control.

The settings cover a binding stepping-out budget (max_stepout 1 or 2, width small against A: the cap is reached), the sampler's own
setting at x_dim 50 (max_stepout 8, width 2 / sqrt(D)) and a budget the box always stops first (a control).  With the budget capped
per side instead of split at random (Neal 2003, sec. 4.1) the binding settings fail.  Run with  pytest -m gpu."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
from oracle import oracle as orc  # noqa: E402  (checker only)
from tests import slice_invariance as si  # noqa: E402

G = os.path.join(os.path.dirname(__file__), 'golden')
SCALE = 5.0
LIKE = {'rosenbrock': 0, 'himmelblau': 2}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda')


def constraint(kind, D):
    """(likelihood name, L*, host test of A in float64 or None for the box): the box alone; Rosenbrock at its median over the box (a
    curved, non-convex A); 2-D Himmelblau at logL > -10 (four separate lobes, so a line meets A in several intervals)"""
    if kind == 'box':
        return 'rosenbrock', -1e30, None
    if kind == 'rosen':
        star = -4400.0
    elif kind == 'himmel':
        assert D == 2
        star = -10.0
    else:
        raise ValueError(kind)
    name = 'himmelblau' if kind == 'himmel' else 'rosenbrock'
    return name, star, lambda x: orc.loglike(name, x, SCALE) > star


def make_flow(kind, D):
    from nnest_amd.flow import HipNVP
    if kind in ('nvp', 'identity'):
        f = HipNVP(D, 16, 3, 1, seed=3)
        if kind == 'identity':
            f.load_packed(np.zeros_like(f.store_packed()))
        return f
    if kind == 'spline':
        from nnest_amd.spline import HipSpline
        return HipSpline(D, 16, 3, 8, 3.0, seed=3)   # (ActNorm's first-batch initialisation runs on the start's forward)
    if kind == 'maf':
        from nnest_amd.maf import HipMAF
        return HipMAF(D, 16, 3, 1, seed=3)
    if kind == 'cholesky':
        from nnest_amd.cholesky import HipCholesky
        g = np.load(os.path.join(G, 'cholesky_d5.npz'))
        assert int(g['D']) == D
        f = HipCholesky(D)
        f.load_packed(g['w0'])
        return f
    if kind == 'fastslow':
        from nnest_amd.fastslow import HipFastSlowNVP
        g = np.load(os.path.join(G, 'fastslow_s2_f3.npz'))
        assert int(g['S']) + int(g['F']) == D
        f = HipFastSlowNVP(int(g['F']), int(g['S']), 16, 3, 1)
        f.load_packed(g['w_trained'])
        return f
    raise ValueError(kind)


def exact_start(flow, D, N, cons, seed):
    """N points uniform on A (host, float64, by rejection), their latent images (the flow's forward) and logL (the library's
    likelihood kernel), without the rows whose float32 round trip leaves A; and an independent uniform sample of A for comparison"""
    from nnest_amd import flow as _flow
    name, star, inside = cons
    rng = np.random.RandomState(seed)
    x = si.uniform_on(rng, N, D, inside)
    fresh = si.uniform_on(rng, N, D, inside)
    z, _ = flow.forward(x.astype(np.float32))
    z = z.contiguous()
    xr, _ = flow.inverse(z)
    logl = _flow.loglike(LIKE[name], xr.contiguous(), SCALE, device=z.device).double()
    keep = (torch.all(torch.abs(xr) <= 1.0, dim=1) & (logl > star)).cpu().numpy()
    assert 1.0 - keep.mean() < 1e-4, 1.0 - keep.mean()
    k = torch.from_numpy(np.flatnonzero(keep)).to(z.device)
    z, logl, xr = z[k].contiguous(), logl[k].contiguous(), xr[k].contiguous()
    return z, logl, xr.cpu().numpy().astype(np.float64), fresh[:z.shape[0]]


def check(step, flow, D, N, cons, width, max_stepout, seed=1):
    """one update (exchangeability of (x0, x1); stationarity of x1), four more (stationarity of x5): one decision at si.ALPHA.
    step(flow, z, logl, star, width, steps, max_stepout, seed) updates z, logl in place and returns (x, n_eval) on the device."""
    name, star, _ = cons
    z, logl, x0, fresh = exact_start(flow, D, N, cons, seed)
    scalars = (si.box_depth,)
    if name == 'himmelblau' or star > -1e29:
        def loglike(x):
            return orc.loglike(name, x, SCALE)
        scalars = (si.box_depth, loglike)
    x1, ne1 = step(flow, z, logl, star, width, 1, max_stepout, 1000 + seed)
    x1 = x1.cpu().numpy().astype(np.float64)
    x5, ne5 = step(flow, z, logl, star, width, 4, max_stepout, 2000 + seed)
    x5 = x5.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(x5) <= 1.0) and bool(torch.all(logl > star))
    p = {}
    for tag, pv in (('S1', si.stationarity_pvalues(x1, fresh, scalars)), ('S5', si.stationarity_pvalues(x5, fresh, scalars)),
                    ('ex', si.exchangeability_pvalues(x0, x1, scalars))):
        p.update({'%s:%s' % (tag, k): v for k, v in pv.items()})
    worst = min(p, key=p.get)
    print('N=%d D=%d max_stepout=%d width=%.3g: min p %s=%.3g (x %d), n_eval/update %.3f'
          % (z.shape[0], D, max_stepout, width, worst, p[worst], len(p), float(ne1.double().mean() + ne5.double().mean()) / 5.0))
    si.assert_invariant(p)


def solo_step(flow, z, logl, star, width, steps, max_stepout, seed, like_id):
    r = flow.slice_steps(like_id, SCALE, z, logl, star, width, steps, max_stepout=max_stepout, seed=seed)
    return r['x'], r['n_eval']


# (constraint, x_dim, flow, max_stepout, width, walkers)
SOLO = [('box', 2, 'nvp', 1, 0.1, 1 << 20),            # binding
        ('box', 2, 'identity', 1, 0.1, 1 << 20),       # binding, identity control of the flow
        ('rosen', 2, 'nvp', 2, 0.05, 1 << 20),         # binding, curved A
        ('himmel', 2, 'nvp', 1, 0.02, 1 << 20),        # binding, four lobes
        ('box', 2, 'nvp', 1000, 0.1, 1 << 20),         # never binds: the box stops every expansion
        ('box', 50, 'nvp', 8, 2.0 / np.sqrt(50), 1 << 18)]   # the sampler's setting


@pytest.mark.parametrize('cons,D,kind,m,width,N', SOLO, ids=['%s-d%d-%s-m%d' % c[:4] for c in SOLO])
def test_solo_slice_keeps_the_uniform_target(dev, cons, D, kind, m, width, N):
    c = constraint(cons, D)
    check(lambda *a: solo_step(*a, like_id=LIKE[c[0]]), make_flow(kind, D), D, N, c, width, m)


SPLINE = [('box', 2, 'wave', 1, 0.1, 1 << 18), ('box', 2, 'team', 1, 0.1, 1 << 18), ('box', 33, 'pair', 1, 0.02, 1 << 18),
          ('himmel', 2, 'team', 1, 0.02, 1 << 18), ('box', 2, 'wave', 1000, 0.1, 1 << 18)]


@pytest.mark.parametrize('cons,D,form,m,width,N', SPLINE, ids=['%s-d%d-%s-m%d' % c[:4] for c in SPLINE])
def test_spline_slice_keeps_the_uniform_target(dev, cons, D, form, m, width, N):
    c = constraint(cons, D)
    sp = make_flow('spline', D)

    def step(flow, z, logl, star, width, steps, max_stepout, seed):
        assert flow.slice_form_for(z.shape[0], form) == form
        r = flow.slice_steps(LIKE[c[0]], SCALE, z, logl, star, width, steps, max_stepout=max_stepout, seed=seed, form=form)
        return r['x'], r['n_eval']
    check(step, sp, D, N, c, width, m)


ROUNDS = [('box', 2, 'maf', 1, 0.1, 1 << 18, 'device'), ('rosen', 2, 'maf', 2, 0.05, 1 << 18, 'device'),
          ('box', 5, 'cholesky', 1, 0.05, 1 << 18, 'device'), ('box', 5, 'fastslow', 1, 0.05, 1 << 18, 'device'),
          ('box', 2, 'nvp', 1, 0.1, 1 << 17, 'host')]


@pytest.mark.parametrize('cons,D,kind,m,width,N,route', ROUNDS, ids=['%s-d%d-%s-m%d-%s' % (c[:4] + c[6:]) for c in ROUNDS])
def test_slice_rounds_keep_the_uniform_target(dev, cons, D, kind, m, width, N, route):
    from nnest_amd.slice_rounds import slice_rounds
    c = constraint(cons, D)

    def step(flow, z, logl, star, width, steps, max_stepout, seed):
        if route == 'host':
            kw = dict(loglike=lambda x: orc.loglike(c[0], x, SCALE))
        else:
            kw = dict(like_id=LIKE[c[0]], like_scale=SCALE)
        r = slice_rounds(flow, z, logl, star, width, steps, max_stepout=max_stepout, seed=seed, **kw)
        return r['x'], r['n_eval']
    check(step, make_flow(kind, D), D, N, c, width, m)
