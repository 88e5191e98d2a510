"""GPU checks of the two likelihoods of user data in the spline flow's TEAM TILE (include/nnest_hip.h nnest_spline_mcmc_gdata_steps,
nnest_spline_mcmc_glm_steps; nnest_amd/csrc/mcmc_gdata.h gdata_tile_loglike<NT>, nnest_amd/csrc/glm_data.h glm_tile_loglike<NT, FAM>)
at every key 10 NT + NH of spl_tile_for_shape and every edge of their blocks: spline_mcmc_gdata_kernel_team<NT, NH> at both sides of
every 16-row block and every 32-column block (tile_like_check.GDATA_CASES: every (rb, tau) skip is executed),
spline_mcmc_glm_kernel_team<NT, NH, FAM> at both families with 1, 2, 4, 5 and 13 row blocks (tile_like_check.GLM_CASES: idle waves,
the second accumulator of NT = 1, ragged last blocks).  The likelihood-alone entries nnest_loglike_gdata / nnest_loglike_glm are
solo-layout kernels; the tile has no such entry, so it is reached through the walk's evaluator (steps = 0) and the walk itself.

Targets and transforms are the existing replays': tests/gdata_check.replay_target, tests/glm_check.make_like, affine(D, D), a box
of +-2.5 on T(x); the flows are tests/test_gpu_fused_likes.spline_flow's.  Per case, on C = 40 walkers (a last tile of 8; row 1 outside
the box, row 2 with a NaN):
  the evaluator: logL against float64 (gdata_check.exact / glm_check.exact) on T of the kernel's own x within the a-priori bound
    B (gdata_check.bound / glm_check.bound: it holds for any summation order, so for the tile's); lp - logL and x against the oracle
    within tests/test_gpu_fused_likes.spline_tols; lp = -inf outside the box, logL = -1e100 on the NaN row;
  position independence: the start reversed gives the rows reversed, its first 1 and 17 rows give the first 1 and 17 rows, bit for bit;
  masking (GLM): the padding behind n dirtied as tests/test_gpu_mcmc_glm.py dirties it changes no bit;
  the walk: six steps at beta = 0.5, global_every = 3, adapt_steps = 4 and a step of the walker's own, checked as the rich runs of
    tests/test_gpu_walk_likes.py with B in the place of fused_like_check.logl_bound.  Seeds: tile_like_check.DATA_SEEDS, chosen on the
    CPU (tools/walk_like_cases.py).
The spline flow does not exist at x_dim 1 (nnest_spline_create refuses the shape): GaussianData's x_dim 1 is held to that refusal."""
import numpy as np
import pytest

from tests import fused_like_check as fl
from tests import glm_check as gk
from tests import tile_like_check as tl
from tests.test_gpu_fused_likes import cpu, note, spline_flow, spline_tols
from tests.test_gpu_walk_likes import check_walk, same_bits, walk_history

pytestmark = pytest.mark.gpu

C, S = tl.C_DATA, tl.S


def test_tables_reach_every_instantiation():
    assert {tl.key(D, H) for D, H in tl.GDATA_CASES if D >= 2} == {11, 21, 31, 41, 12, 22}
    assert {(tl.key(D, H), fam) for D, H, fam, _ in tl.GLM_CASES} == {(k, f) for k in (11, 21, 31, 41, 12, 22) for f in gk.FAMILIES}
    assert len(tl.GLM_CASES) == len(tl.GLM_DIMS) * 2 * len(tl.GLM_NS)


def test_x_dim_1_has_no_spline_flow():
    """the one shape of the tables the library cannot launch: it is refused where the flow is made, in the library's words"""
    from nnest_amd._lib import NnestHipError
    from nnest_amd.spline import HipSpline
    assert (1, 16) in tl.GDATA_CASES
    with pytest.raises(NnestHipError, match='bad shape D=1 H=16'):
        HipSpline(1, 16, 3, seed=17)


def flow_rows(what, o, z, x, lp, logl, beta, sd, mu, box, ld_tol, x_tol):
    """x against the oracle's inverse of the kernel's own z, lp - beta logL (float64 from the exported logL) against its log-det on the
    rows inside the box by the kernel's own x, -inf exactly outside; a row with a NaN in z is left out.  Returns the worst error /
    tolerance of x and of the log-det"""
    z, x, lp, logl = np.asarray(z, np.float32), np.asarray(x, np.float32), np.asarray(lp, np.float64), np.asarray(logl, np.float64)
    ok = ~np.isnan(z).any(1)
    z, x, lp, logl = z[ok], x[ok], lp[ok], logl[ok]
    xo, ldo = o.inverse(z)
    r_x = float(np.max(np.abs(x - xo) / x_tol(xo)))
    assert r_x <= 1.0, '%s: x against the oracle: %.3g of the tolerance' % (what, r_x)
    with np.errstate(invalid='ignore'):
        lp1 = np.where(np.isfinite(lp), (lp - beta * logl) + logl, lp)
    r_ld = fl.check_lp_split(lp1, logl, ldo, fl.in_box(fl.T32(x, sd, mu), -box, box), ld_tol(np.asarray(ldo, np.float64)), what=what)
    return r_x, r_ld


def run_case(kind, sp, o, D, H, fam=None, n=None):
    data = tl.data_like(kind, D, fam, n)
    ratio = tl.gdata_ratio if kind == 'gdata' else tl.glm_ratio
    like_kw = (lambda d: dict(like_data=d)) if kind == 'gdata' else (lambda d: dict(like_glm=d))
    sd, mu = tl.affine(D, D)
    box = np.full(D, tl.HALF, np.float32)
    seed = tl.DATA_SEEDS[(kind, D, H) if kind == 'gdata' else (kind, D, H, fam, n)]
    step = 1.0 / np.sqrt(D)
    key = tl.key(D, H)
    what = '%s key %d x_dim %d%s' % (kind, key, D, '' if kind == 'gdata' else ' %s n %d' % (fam, n))
    z0, _ = sp.forward(tl.data_start_x(D))
    z0 = z0.contiguous()
    ld_tol, x_tol = spline_tols(key, o, cpu(z0))
    base = dict(t_std=sd, t_mean=mu, lo=-box, hi=box, seed=seed)
    kw = dict(base, **like_kw(data))
    ends = ('x', 'lp', 'logl')
    # the evaluator
    begin = sp.mcmc_steps(None, z0, 0, step, **kw)
    x, lp, logl = (cpu(begin[k]) for k in ends)
    r_ll = ratio(logl, data, fl.T32(x, sd, mu))
    assert r_ll <= 1.0, '%s: logL of the kernel\'s own x: %.3g of B' % (what, r_ll)
    assert lp[1] == -np.inf and np.isfinite(logl[1]) and logl[2] == fl.SAFE, what
    assert np.isfinite(lp[np.arange(C) != 2]).sum() > C // 4, what
    r_x, r_ld = flow_rows(what + ' start', o, cpu(z0), x, lp, logl, 1.0, sd, mu, box, ld_tol, x_tol)
    # position independence
    clean = ~np.isnan(cpu(z0)).any(1)
    back = sp.mcmc_steps(None, z0.flip(0).contiguous(), 0, step, **kw)
    for k in ends:
        assert same_bits(cpu(back[k])[::-1], begin[k], clean if k == 'x' else None), '%s: reversed rows: %s' % (what, k)
    for m in (1, 17):
        part = sp.mcmc_steps(None, z0[:m].contiguous(), 0, step, **kw)
        for k in ends:
            assert same_bits(part[k], cpu(begin[k])[:m], clean[:m] if k == 'x' else None), '%s: the first %d rows: %s' % (what, m, k)
    # masking
    if kind == 'glm':
        dirty = dict(data, at=np.array(data['at'], np.float32), y=np.array(data['y'], np.float32), o=np.array(data['o'], np.float32))
        dirty['at'][:, n:] = np.random.RandomState(n).normal(size=dirty['at'][:, n:].shape) * 1e6
        dirty['y'][n:] = 7.0
        dirty['o'][n:] = np.nan
        masked = sp.mcmc_steps(None, z0, 0, step, **dict(base, **like_kw(dirty)))
        for k in ends:
            assert same_bits(masked[k], begin[k], clean if k == 'x' else None), '%s: dirty padding: %s' % (what, k)
    # the walk
    from nnest_amd import flow
    beta, k, adapt, spread = tl.DATA_CONFIG
    Z, X, LL, LP, SIG, n_acc, n_glob, ok = walk_history(sp, None, z0, step, kw, beta, k, adapt, spread)
    r_ll = max(r_ll, ratio(LL.reshape(-1), data, fl.T32(X.reshape(-1, D), sd, mu)))
    assert r_ll <= 1.0, '%s: logL of the kernel\'s own x along the walk: %.3g of B' % (what, r_ll)
    assert LP[1, 0] == -np.inf and LL[2, 0] == fl.SAFE, what
    w_x, w_ld = flow_rows(what, o, Z.reshape(-1, D), X.reshape(-1, D), LP.reshape(-1), LL.reshape(-1), beta, sd, mu, box, ld_tol, x_tol)
    eps, u = (cpu(t) for t in flow.mcmc_fill_noise(S, C, D, seed=seed))
    local_moved, local, glob_acc, glob = check_walk(what, Z, X, LL, LP, SIG, n_acc, n_glob, ok, eps, u, k, adapt, spread)
    print('%s: local steps moved %d of %d, global proposals accepted %d of %d (walkers that start inside the box)' % (
        what, local_moved, local, glob_acc, glob))
    note('spline_mcmc_%s_kernel_team' % kind, 'key %d%s' % (key, '' if kind == 'gdata' else ' ' + fam), kind, 'n %d' % (n or 0), D,
         x=max(r_x, w_x), logL_of_B=r_ll, lp_minus_logL=max(r_ld, w_ld))
    assert 0 < local_moved < local and 1 <= glob_acc <= glob - 1, what


@pytest.mark.parametrize('D,H', [c for c in tl.GDATA_CASES if c[0] >= 2], ids=lambda v: str(v))
def test_gdata_tile(D, H):
    sp, o = spline_flow(D, H, C)
    run_case('gdata', sp, o, D, H)


@pytest.mark.parametrize('fam', gk.FAMILIES)
@pytest.mark.parametrize('D,H', tl.GLM_DIMS, ids=lambda v: str(v))
def test_glm_tile(D, H, fam):
    sp, o = spline_flow(D, H, C)
    for n in tl.GLM_NS:
        run_case('glm', sp, o, D, H, fam, n)
