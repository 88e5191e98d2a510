"""CPU checks of the checker of tests/test_gpu_mh_glm.py and tests/test_gpu_spline_mh_glm.py (tests/mh_glm_check.py): the restatement
alone on a seeded random orc.NVP(D, 16, 3, 1) (weights N(0, 0.15^2)) with numpy draws.
- the tables reach every <U, FAM> and <NT, NH> they claim, at S > lag + 2 for every lag;
- the cap condition: for every row of the NVP table and two noise seeds, the near share -- from the oracle alone -- stays within
  1 - AGREE, under the fixed step and the batch rule;
- the restatement is held to something: with exact_logl swapped for an analytic likelihood it reproduces oracle.mcmc_sample (the
  pinned C oracle) on an orc.NVP at lag 0, 1 and 3, decision for decision;
- a stand-in kernel -- the restatement with glm_check.float32_eval for the likelihood -- passes `hold` under every rule, and each
  planted fault fails it: the likelihood counted at every proposal, n_call counting acc, the box on T(x), a vote applied one step
  early, t_mean dropped, the vote's total taken over workgroups;
- the library declares the new entries, the Makefile builds both units (the spline's without MachineLICM), _lib binds them."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import glm_check as gk
from tests import mh_glm_check as mg
from tests import slice_like_check as sl
from tests.fused_like_check import units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mg.NVP_TABLE + mg.NVP_EXTRA
BY_ID = {mg.case_id(c): c for c in CASES}
NEW = ('nnest_mh_glm_steps', 'nnest_spline_mh_glm_steps', 'nnest_mh_glm_check', 'nnest_spline_mh_glm_check')
RULES = [('fixed', 0)] + [('batch', lag) for lag in mg.LAGS] + [('tile', 0)]


def random_flow(D):
    n = orc.NVP(D, 16, 3, 1).n
    return orc.NVP(D, 16, 3, 1, (np.random.RandomState(D).normal(size=n) * 0.15).astype(np.float32))


_RUNS = {}


def oracle_run(c, rule='fixed', lag=0, seed=0):
    """(flow, z0, l0, star, dz, u, restatement, margins) of a case on draws of `seed`; computed once, never changed"""
    key = (c, rule, lag, seed)
    if key not in _RUNS:
        o = random_flow(c.D)
        z0, l0, star = mg.start(c, lambda x: o.forward(x.astype(np.float32))[0])
        C = len(l0)
        r = np.random.RandomState(100 + seed)
        dz = r.standard_normal((c.S, C, c.D)).astype(np.float32)
        u = r.uniform(size=(c.S, C)).astype(np.float32)
        margins = np.empty((c.S, C))
        ref = mg.trace(o, c, z0, l0, star, mg.step_of(c.D), dz, u, rule, lag, margins=margins)
        _RUNS[key] = (o, z0, l0, star, dz, u, ref, margins)
    return _RUNS[key]


def kernel_likelihood(c, drop_mean=False):
    """what a kernel computes -- glm_check.float32_eval on the float32 T(x) --, or that with t_mean dropped from T"""
    def evaluate(x):
        sd, mu = mg.affine_of(c)
        t = (np.asarray(x, np.float32) * sd).astype(np.float32) + (np.zeros_like(mu) if drop_mean else mu)
        return gk.float32_eval(mg.data_of(c), t, 'reversed')
    return evaluate


def stand_in(c, rule, lag, fault=None):
    o, z0, l0, star, dz, u, ref, margins = oracle_run(c, rule, lag)
    return mg.trace(o, c, z0, l0, star, mg.step_of(c.D), dz, u, rule, lag, evaluate=kernel_likelihood(c, fault == 't_mean'),
                    fault=None if fault == 't_mean' else fault)


def held(c, rule, lag, r, what):
    """what the GPU tests assert of a kernel's output, in their order"""
    o, z0, l0, star, dz, u, ref, margins = oracle_run(c, rule, lag)
    return mg.hold(c, mg.as_kernel(r), ref, margins, l0, star, rule, lag, what=what)


def test_tables_reach_every_instantiation_they_claim():
    assert [(units(c.D), c.family) for c in mg.NVP_TABLE] == [(1, 'logistic'), (2, 'poisson'), (3, 'logistic'), (4, 'logistic'), (4, 'poisson')]
    assert {c.n for c in mg.NVP_TABLE} == {257, 64, 65, 300}
    assert all(not c.affine for c in mg.NVP_TABLE) and all(c.affine for c in mg.NVP_EXTRA)
    assert {(units(sc.case.D), sc.H // 16) for sc in mg.SPLINE_TABLE} == {(1, 1), (2, 1), (3, 1), (4, 1), (1, 2)}
    assert all(sc.C == 19 for sc in mg.SPLINE_TABLE)
    for c in CASES + [sc.case for sc in mg.SPLINE_TABLE]:
        assert 6 <= c.S <= 8 and c.S > max(mg.LAGS) + 2
    o, z0, l0, star = oracle_run(mg.NVP_TABLE[0])[:4]
    assert len(l0) == 51 and (len(l0) + 3) // 4 == 13 and len(l0) % 4 != 0   # 13 workgroups, the last ragged


@pytest.mark.parametrize('cid', sorted(BY_ID))
def test_cap_condition_holds_for_the_nvp_table(cid):
    c = BY_ID[cid]
    shares = [mg.near_share(oracle_run(c, rule, 0, s)[7]) for s in range(2) for rule in ('fixed', 'batch')]
    print('NEAR %-26s %s' % (cid, ' '.join('%.3f' % s for s in shares)))
    assert max(shares) <= mg.CAP
    ref = oracle_run(c)[6]
    # the case exercises every branch: proposals with and without pre, with pre and below L*, accepted
    assert (~ref['pre']).any() and (ref['pre'] & ~ref['acc']).any() and 0.1 < ref['acc'].mean()


@pytest.mark.parametrize('lag', mg.LAGS)
def test_restatement_reproduces_the_pinned_oracle(lag):
    """oracle.mcmc_sample (nnest_oracle.c) on an orc.NVP with the Rosenbrock likelihood, the batch rule at this lag: the same chains,
    counters, votes and scale, decision for decision"""
    D, C, S = 5, 37, 12
    o = random_flow(D)
    r = np.random.RandomState(11 + lag)
    init = r.uniform(-0.6, 0.6, size=(C, D))
    l0 = orc.loglike('rosenbrock', init, 5.0)
    star = float(np.quantile(l0, 0.2))
    init, l0 = init[l0 > star], l0[l0 > star]
    C = len(l0)
    dz = r.standard_normal((S, C, D)).astype(np.float32)
    u = r.uniform(size=(S, C)).astype(np.float32)
    step = 0.3
    samples, latent, loglikes, scale, ncall, (acc, rej) = orc.mcmc_sample(o, 'rosenbrock', 5.0, init, l0, star, step, True, dz, u, lag=lag)
    c = mg.Case('logistic', D, 64, 5.0, S, False)   # (its likelihood is not read: `evaluate` below)
    tr = mg.trace(o, c, latent[:, 0], l0, star, step, dz, u, 'batch', lag, evaluate=lambda x: orc.loglike('rosenbrock', x, 5.0))
    assert tr['n_call'].sum() == ncall and tr['n_accept'].sum() == acc and S * C - tr['n_accept'].sum() == rej
    assert np.array_equal(np.any(samples[:, 1:] != samples[:, :-1], axis=2).T, tr['acc'])   # decision for decision
    np.testing.assert_allclose(tr['x'], samples, rtol=0, atol=1e-6)
    np.testing.assert_allclose(tr['logl'], loglikes, rtol=1e-12)
    assert abs(tr['scale'][0] - scale) <= 1e-12 * scale
    assert 0 < acc < S * C and len(set(tr['acc'].sum(1) * 2 > C)) == 2   # votes of both kinds


STAND_INS = [(c, rule, lag) for c in (mg.NVP_TABLE[1], mg.NVP_EXTRA[0]) for rule, lag in RULES]


@pytest.mark.parametrize('c,rule,lag', STAND_INS, ids=['%s-%s%d' % (mg.case_id(c), rule, lag) for c, rule, lag in STAND_INS])
def test_a_float32_kernel_passes(c, rule, lag):
    agree, near, r_x, r_ll, full = held(c, rule, lag, stand_in(c, rule, lag), 'stand-in')
    assert agree.mean() >= sl.AGREE


FAULTS = [('count_all', 'fixed', 0), ('ncall_acc', 'fixed', 0), ('box_on_T', 'fixed', 0), ('early_vote', 'batch', 1), ('early_vote', 'batch', 3),
          ('t_mean', 'fixed', 0), ('total_wg', 'batch', 0), ('total_wg', 'batch', 1)]   # (at lag 3 the first S - 4 counts of this row are above C / 2 either way)


@pytest.mark.parametrize('fault,rule,lag', FAULTS, ids=['%s-%s%d' % f for f in FAULTS])
def test_planted_faults_fail(fault, rule, lag):
    c = mg.NVP_EXTRA[0]   # (the row whose T has a mean)
    held(c, rule, lag, stand_in(c, rule, lag), 'clean')
    with pytest.raises(AssertionError):
        held(c, rule, lag, stand_in(c, rule, lag, fault), fault)


def test_the_library_declares_builds_and_binds_the_entries():
    from nnest_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    make = open(os.path.join(ROOT, 'nnest_amd', 'csrc', 'Makefile')).read()
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['nnest_mh_glm_steps']) == len(_lib.SIGNATURES['nnest_spline_mh_glm_steps']) == 23
    srcs = re.search(r'^SRCS := (.*)$', make, re.M).group(1).split()
    assert 'nnest_mh_glm.hip' in srcs and 'nnest_spline_mh_glm.hip' in srcs
    licm = re.search(r'^LICM_OFF := (.*)$', make, re.M).group(1).split()
    assert 'nnest_spline_mh_glm' in licm and 'nnest_mh_glm' not in licm
    from nnest_amd import flow, spline
    assert 'mh_glm_refusal' in dir(flow.HipNVP) and 'mh_glm_refusal' in dir(spline.HipSpline)
