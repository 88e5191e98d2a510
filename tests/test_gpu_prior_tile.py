"""GPU checks of the normal priors of gauss_prior.h INSIDE the two walk kernels, at every kernel shape (include/nnest_hip.h
nnest_spline_mcmc_glm_prior_steps, nnest_mcmc_glm_prior_steps): spline_mcmc_glm_prior_kernel_team<NT, NH, FAM> at every key
10 NT + NH = 11, 21, 31, 41, 12, 22 of spl_tile_for_shape -- the prior's m and r sit in LDS behind buffers whose size depends on x_dim
and NT, are read with the stride 8 NT through a restated class split, and are staged by a loop over 32 NT --, at a ragged last lane
group (x_dim 31), an exactly full tile (64, 128) and one dimension past it (33, 65, 97); mcmc_glm_prior_kernel<U, FAM> at both sides
of every edge of U = 1 .. 4 and at x_dim 1; both families throughout.  tests/test_gpu_mcmc_glm_prior.py launches keys 11 and 21 and
no edge.  The tables, the restatements, the planted faults and the seeds are tests/prior_tile_check.py's; tests/test_prior_tile_check.py
shows on the CPU that criterion (b) below catches each planted misread of the prior at every shape where it can show.

Data, transform, box and start are the sibling cases' (tests/test_gpu_tile_data_likes.py): tests/glm_check.replay_target,
affine(D, D), +-2.5 on T(x), C = 40 walkers (a last tile of 8; row 1 outside the box, row 2 with a NaN); the prior is
tests/gauss_prior_check.replay_prior(D, width), a mean and a sigma of its own per dimension.  Per table row:
  (a) the chain to the sibling.  With the FLAT descriptor (r = 0, logc = 0.0: log pi = +0.0 on a finite row, and adding +0.0 is
      exact) the evaluator (steps = 0, beta 1 and 0.5) and the six-step walk of tile_like_check.DATA_CONFIG (beta 0.5,
      global_every 3, adapt_steps 4, a step per walker) inside the box are nnest_*_mcmc_glm_steps's, bit for bit, on every row with
      finite coordinates: histories, ends, counters.  The flow and the likelihood of the new kernels are thereby held, at every key,
      by what tests/test_gpu_tile_data_likes.py and tests/test_gpu_mcmc_glm.py hold the siblings to.  No tolerance.
  (b) the prior term alone.  Flat prior against real prior on the same start at beta 1 and 0.5: x and logL bit-equal, and on every
      finite row inside the box |lp_real - (lp_flat + exact(prior, T(x)))| <= B_pi(T(x)) + 2^-52 |lp_real|, T(x) from the kernel's own
      x (fused_like_check.T32).  DERIVED, not measured: lp = ((beta logL) + ld) + log pi with each operation rounded; the flat run
      returns the bracket exactly; the kernel's log pi is within B_pi (tests/gauss_prior_check.py: 2^-22 of the term, any order of
      summation) of float64; one float64 addition on each side is 2^-53 relative.  No flow tolerance enters.  Outside the box lp is
      -inf in both runs; on the NaN row logL is -1e100 and lp is never +inf.
  (c) along the walk.  One step a launch with lp, logL, step0 and the walkers' steps carried, and once in one launch: the same bits
      (tests/test_gpu_walk_likes.walk_history).  Every stored z is evaluated again with the flat prior: its x and logL are the stored
      bits, and (b) holds on every stored row.  tests/test_gpu_walk_likes.check_walk: a moved row is the exported draw, an unmoved
      row is the previous row bit for bit, a moved row's stored lp satisfy the kernel's own acceptance inequality, counters and
      hist_step follow the replayed rule.  x against the oracle's inverse within spline_tols / nvp_tols (tests/test_gpu_fused_likes.py),
      and lp - beta logL - exact log pi against its log-det within that plus B (tests/glm_check.py) plus B_pi.
  (d) position independence, with the prior present: the start reversed gives the rows reversed, its first 1 and 17 rows give those
      rows, and the GLM's padding behind n dirtied changes no bit.
Prior widths and seeds: prior_tile_check.PRIOR_SEEDS, chosen on the CPU (tools/walk_like_cases.py prior); under each width the float32
restatement leaves half of B_pi unused on the row's start.

Measured on the MI355X (the SHARE lines; logistic / poisson): the prior term is at most 0.76 / 0.71 (key 11), 0.30 / 0.35 (21),
0.19 / 0.23 (31), 0.22 / 0.28 (41), 0.49 / 0.64 (12), 0.27 / 0.32 (22) of B_pi + 2^-52 |lp| off lp_flat + float64 in the tile kernel and
0.75 / 0.74 (U = 1: x_dim 1 along the walk, where one term's two float32 roundings are the whole error; the widths are chosen for the
start alone), 0.28 / 0.32 (2), 0.23 / 0.23 (3), 0.17 / 0.17 (4) in the solo kernel; x uses at most 0.19 and lp - beta logL - log pi at
most 0.14 of the spline's tolerances, 0.75 and 0.014 of the NVP's; every count of moved local steps and accepted global proposals is
the CPU restatement's (tools/walk_like_cases.py prior).  A library built with r read at the stride of NT - 1 for NT >= 3 passes
every spline case of tests/test_gpu_mcmc_glm_prior.py and fails the six cases of keys 31 and 41 here, at (a)."""
import numpy as np
import pytest
import torch

from tests import fused_like_check as fl
from tests import gauss_prior_check as pk
from tests import glm_check as gk
from tests import prior_tile_check as pt
from tests import tile_like_check as tl
from tests.test_gpu_fused_likes import cpu, nvp_flow, nvp_tols, spline_flow, spline_tols
from tests.test_gpu_walk_likes import ENDS, HIST, check_walk, same_bits, walk_history

pytestmark = pytest.mark.gpu

C, S = pt.C, pt.S
KEYS = (11, 21, 31, 41, 12, 22)
SHARES = {}   # (kernel, instantiation, family) -> the worst share of B_pi seen by (b) and (c)


def test_tables_reach_every_instantiation():
    assert {(tl.key(D, H), fam) for _, D, H, fam, _ in pt.SPLINE_CASES} == {(k, f) for k in KEYS for f in gk.FAMILIES}
    assert {(fl.units(D), fam) for _, D, _, fam, _ in pt.NVP_CASES} == {(U, f) for U in (1, 2, 3, 4) for f in gk.FAMILIES}
    for U in (1, 2, 3, 4):   # the edge-full width of every U, the edge-plus-one width of every U that has one
        assert 32 * U in pt.NVP_DIMS and (U == 1 or 32 * (U - 1) + 1 in pt.NVP_DIMS)
    assert set(pt.PRIOR_SEEDS) == set(pt.CASES) and (C, S) == (40, 6)


def prior_flow_rows(what, o, z, x, lp, logl, beta, prior, data, sd, mu, box, ld_tol, x_tol):
    """tests/test_gpu_tile_data_likes.flow_rows under the prior: x against the oracle's inverse of the kernel's own z within x_tol;
    lp - beta logL - exact log pi (float64, from the exported logL and the kernel's own x) against its log-det within
    ld_tol + B + B_pi on the rows inside the box, -inf exactly outside; a row with a NaN in z is left out"""
    z, x, lp, logl = np.asarray(z, np.float32), np.asarray(x, np.float32), np.asarray(lp, np.float64), np.asarray(logl, np.float64)
    ok = ~np.isnan(z).any(1)
    z, x, lp, logl = z[ok], x[ok], lp[ok], logl[ok]
    xo, ldo = o.inverse(z)
    r_x = float(np.max(np.abs(x - xo) / x_tol(xo)))
    assert r_x <= 1.0, '%s: x against the oracle: %.3g of the tolerance' % (what, r_x)
    t = fl.T32(x, sd, mu)
    with np.errstate(invalid='ignore', over='ignore'):
        lp1 = np.where(np.isfinite(lp), ((lp - pk.exact(prior, t)) - beta * logl) + logl, lp)
        extra = gk.bound(data, t) + pk.bound(prior, t)
    tol = ld_tol(np.asarray(ldo, np.float64)) + np.where(np.isfinite(extra), extra, 0.0)
    return r_x, fl.check_lp_split(lp1, logl, ldo, fl.in_box(t, -box, box), tol, what=what)


def run_case(flow, net, o, tols, D, H, fam, n):
    from nnest_amd import flow as flow_mod
    case = (flow, D, H, fam, n)
    width, seed = pt.PRIOR_SEEDS[case]
    data = tl.data_like('glm', D, fam, n)
    prior = pk.descriptor(pk.replay_prior(D, width))
    flat = pt.flat(prior)
    sd, mu = tl.affine(D, D)
    box = np.full(D, tl.HALF, np.float32)
    step = 1.0 / np.sqrt(D)
    inst = 'key %d' % tl.key(D, H) if flow == 'spline' else 'U %d' % fl.units(D)
    kernel = 'spline_mcmc_glm_prior_kernel_team' if flow == 'spline' else 'mcmc_glm_prior_kernel'
    what = '%s %s x_dim %d %s n %d' % (kernel, inst, D, fam, n)
    assert net.mcmc_glm_prior_refusal() is None, what
    z0, _ = net.forward(tl.data_start_x(D))
    z0 = z0.contiguous()
    ok = ~np.isnan(cpu(z0)).any(1)
    assert not ok[2] and ok.sum() == C - 1
    ld_tol, x_tol = tols(z0)
    base = dict(t_std=sd, t_mean=mu, lo=-box, hi=box, seed=seed)
    sib_kw = dict(base, like_glm=data)
    ends = ('x', 'lp', 'logl')
    worst = 0.0

    def held(x, lp_real, lp_flat, tag):
        t = fl.T32(x, sd, mu)
        share = pt.prior_term_share(lp_real, lp_flat, prior, t, fl.in_box(t, -box, box))
        assert share <= 1.0, '%s: %s: the prior term is %.3g of B_pi + 2^-52 |lp| off lp_flat + float64' % (what, tag, share)
        return share

    # (a) the evaluator and (b) the prior term alone, at both powers
    begin = {}
    for beta in pt.BETAS:
        sib = net.mcmc_steps(None, z0, 0, step, beta=beta, **sib_kw)
        f = net.mcmc_steps(None, z0, 0, step, beta=beta, prior_gauss=flat, **sib_kw)
        r = net.mcmc_steps(None, z0, 0, step, beta=beta, prior_gauss=prior, **sib_kw)
        for k in ends:
            assert same_bits(f[k], sib[k], ok), '%s: beta %g: the flat evaluator against the sibling: %s' % (what, beta, k)
        assert same_bits(r['x'], f['x'], ok) and same_bits(r['logl'], f['logl']), '%s: beta %g: x or logL changes with the prior' % (what, beta)
        x, lp_r, lp_f, logl = cpu(r['x']), cpu(r['lp']), cpu(f['lp']), cpu(r['logl'])
        x[2] = np.nan   # (the NaN row: no coordinate of it is compared)
        worst = max(worst, held(x, lp_r, lp_f, 'beta %g' % beta))
        assert lp_r[1] == -np.inf and lp_f[1] == -np.inf and np.isfinite(logl[1]), what
        assert logl[2] == fl.SAFE and not lp_r[2] == np.inf and not lp_f[2] == np.inf, what
        assert np.isfinite(lp_r[ok]).sum() > C // 4 and not np.array_equal(lp_r[ok], lp_f[ok]), what
        begin[beta] = r
    r_x, r_ld = prior_flow_rows(what + ' start', o, cpu(z0), cpu(begin[1.0]['x']), cpu(begin[1.0]['lp']), cpu(begin[1.0]['logl']), 1.0, prior,
                                data, sd, mu, box, ld_tol, x_tol)

    # (a) the walk
    beta, k, adapt, spread = tl.DATA_CONFIG
    step_in = torch.from_numpy(tl.step_spread(C, D)).to(z0.device)
    cfg = dict(sib_kw, beta=beta, global_every=k, adapt_steps=adapt, adapt_rate=tl.RATE, target_accept=tl.TARGET, step_in=step_in)
    sib = net.mcmc_steps(None, z0, S, step, **cfg)
    ours = net.mcmc_steps(None, z0, S, step, prior_gauss=flat, **cfg)
    for key in HIST + ('hist_step',) + ENDS + ('step', 'n_accept', 'n_accept_global'):
        assert same_bits(ours[key], sib[key], ok), '%s: the flat walk against the sibling: %s' % (what, key)
    assert 0 < int(sib['n_accept'].sum()) < C * S

    # (d) position independence, with the prior present
    kw = dict(sib_kw, prior_gauss=prior)
    b1 = begin[1.0]
    back = net.mcmc_steps(None, z0.flip(0).contiguous(), 0, step, beta=1.0, **kw)
    for key in ends:
        assert same_bits(cpu(back[key])[::-1], b1[key], ok if key == 'x' else None), '%s: reversed rows: %s' % (what, key)
    for m in (1, 17):
        part = net.mcmc_steps(None, z0[:m].contiguous(), 0, step, beta=1.0, **kw)
        for key in ends:
            assert same_bits(part[key], cpu(b1[key])[:m], ok[:m] if key == 'x' else None), '%s: the first %d rows: %s' % (what, m, key)
    dirty = dict(data, at=np.array(data['at'], np.float32), y=np.array(data['y'], np.float32), o=np.array(data['o'], np.float32))
    dirty['at'][:, n:] = np.random.RandomState(n).normal(size=dirty['at'][:, n:].shape) * 1e6
    dirty['y'][n:] = 7.0
    dirty['o'][n:] = np.nan
    masked = net.mcmc_steps(None, z0, 0, step, beta=1.0, **dict(kw, like_glm=dirty))
    for key in ends:
        assert same_bits(masked[key], b1[key], ok if key == 'x' else None), '%s: dirty padding: %s' % (what, key)

    # (c) along the walk
    Z, X, LL, LP, SIG, n_acc, n_glob, ok_w = walk_history(net, None, z0, step, kw, beta, k, adapt, spread)
    assert np.array_equal(ok_w, ok) and LP[1, 0] == -np.inf and LL[2, 0] == fl.SAFE, what
    again = net.mcmc_steps(None, torch.from_numpy(np.ascontiguousarray(Z.reshape(-1, D))).to(z0.device), 0, step, beta=beta, prior_gauss=flat, **sib_kw)
    rows = np.repeat(ok, S + 1)
    assert same_bits(again['x'], X.reshape(-1, D), rows) and same_bits(again['logl'], LL.reshape(-1), rows), \
        '%s: a stored row evaluated again is not the stored x and logL' % what
    Xc = X.reshape(-1, D).copy()
    Xc[~rows] = np.nan
    worst = max(worst, held(Xc, LP.reshape(-1), cpu(again['lp']), 'along the walk'))
    w_x, w_ld = prior_flow_rows(what, o, Z.reshape(-1, D), X.reshape(-1, D), LP.reshape(-1), LL.reshape(-1), beta, prior, data, sd, mu, box,
                                ld_tol, x_tol)
    eps, u = (cpu(t) for t in flow_mod.mcmc_fill_noise(S, C, D, seed=seed))
    local_moved, local, glob_acc, glob = check_walk(what, Z, X, LL, LP, SIG, n_acc, n_glob, ok, eps, u, k, adapt, spread)
    print('%s: width %g seed %d: the prior term at most %.3g of its bound; x %.3g, lp - beta logL - log pi %.3g of the tolerance; local steps '
          'moved %d of %d, global proposals accepted %d of %d (walkers that start inside the box)'
          % (what, width, seed, worst, max(r_x, w_x), max(r_ld, w_ld), local_moved, local, glob_acc, glob))
    assert 0 < local_moved < local and 1 <= glob_acc <= glob - 1, what
    tag = (kernel, inst, fam)
    SHARES[tag] = max(SHARES.get(tag, 0.0), worst)
    print('SHARE %-34s %-7s %-8s worst |lp_real - (lp_flat + float64 log pi)| = %.3g of B_pi + 2^-52 |lp|' % (tag + (SHARES[tag],)))


@pytest.mark.parametrize('fam', gk.FAMILIES)
@pytest.mark.parametrize('D,H', pt.SPLINE_DIMS, ids=lambda v: str(v))
def test_spline_prior_tile(D, H, fam):
    sp, o = spline_flow(D, H, C)
    for n in pt.SPLINE_NS:
        run_case('spline', sp, o, lambda z0: spline_tols(tl.key(D, H), o, cpu(z0)), D, H, fam, n)


@pytest.mark.parametrize('fam', gk.FAMILIES)
@pytest.mark.parametrize('D', pt.NVP_DIMS)
def test_nvp_prior_solo(D, fam):
    net, o = nvp_flow(D)
    run_case('nvp', net, o, lambda z0: nvp_tols(D, net, o, z0, tag='prior walk'), D, 16, fam, pt.NVP_N)
