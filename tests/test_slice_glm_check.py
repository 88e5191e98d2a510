"""CPU checks of the checker of tests/test_gpu_slice_glm.py and tests/test_gpu_spline_slice_glm.py (tests/slice_glm_check.py): the
oracle alone on a seeded random orc.NVP(D, 16, 3, 1) (weights N(0, 0.15^2)) with numpy normal directions.
- the tables reach every <U, FAM> and <NT, NH> they claim;
- the cap condition: for every row of the NVP table and three direction seeds, near_share <= 0.2 -- the share of walkers on which a
  correct kernel may differ from the oracle stays within what the 80 % criterion allows;
- planted faults: oracle.slice_sample runs a second time as a stand-in kernel whose likelihood is glm_check.float32_eval (eta in
  float32 in the order 'forward', 'reversed' or 'pairwise': each passes), then wrong in one way each -- t_mean dropped, the offset
  dropped, rows >= n counted, the family swapped, the box tested on T(x) against +-1, a non-finite logL mapped to 0 --, and each wrong
  version fails `compare`, the own-x check or `check_nothing_moves`;
- the library declares the new entries, the Makefile builds the spline unit without MachineLICM, and the Python bindings refuse what
  they must without a device."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import glm_check as gk
from tests import slice_glm_check as sg
from tests import slice_like_check as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, OFF = 4242, 100
CASES = sg.NVP_TABLE + sg.NVP_EXTRA
BY_ID = {sg.case_id(c): c for c in CASES}
NEW = ('nnest_slice_glm_steps', 'nnest_spline_slice_glm_steps', 'nnest_slice_glm_check', 'nnest_spline_slice_glm_check')


def random_flow(D):
    n = orc.NVP(D, 16, 3, 1).n
    return orc.NVP(D, 16, 3, 1, (np.random.RandomState(D).normal(size=n) * 0.15).astype(np.float32))


_RUNS = {}


def oracle_run(c, dz_seed=0, safe=False):
    """(flow, z0, l0, star, dz, oracle result, margins) of a case on directions of seed dz_seed -- safe: under the descriptor with NaN
    offsets, from the start of the clean one; computed once, never changed"""
    key = (c, dz_seed, safe)
    if key not in _RUNS:
        o = random_flow(c.D)
        z0, l0, star = sg.start(c, lambda u: o.forward(u.astype(np.float32))[0])
        C = len(l0)
        dz = np.random.RandomState(100 + dz_seed).standard_normal((c.S, C, c.D)).astype(np.float32)
        margins = np.empty((c.S, C))
        ev = (lambda x: sg.exact_logl(c, x, sg.non_finite_data(c))) if safe else None
        ref = sg.slice_sample(o, c, z0, l0, star, dz, SEED, OFF, evaluate=ev, margins=margins)
        _RUNS[key] = (o, z0, l0, star, dz, ref, margins)
    return _RUNS[key]


FAULTS = ('t_mean', 'offset', 'padding', 'family', 'box_on_T', 'finite')


def kernel_likelihood(c, order='forward', fault=None, safe=False):
    """what a kernel computes -- glm_check.float32_eval on the float32 T(x) --, or that with one planted fault: 't_mean' dropped from
    T; the 'offset' dropped; 'padding': the rows >= n counted (n taken for ld); the 'family' swapped; 'finite': a non-finite logL mapped
    to 0 and not to -1e100"""
    data = dict(sg.non_finite_data(c) if safe else sg.data_of(c))
    if fault == 'offset':
        data['o'] = np.zeros_like(data['o'])
    if fault == 'padding':
        data['n'] = data['at'].shape[1]
    if fault == 'family':
        data['family'] = 'poisson' if c.family == 'logistic' else 'logistic'

    def evaluate(x):
        sd, mu = sg.affine_of(c)
        t = (np.asarray(x, np.float32) * sd).astype(np.float32) + (np.zeros_like(mu) if fault == 't_mean' else mu)
        out = gk.float32_eval(data, t, order)
        if fault == 'finite':
            out = np.where(out == gk.SAFE, 0.0, out)
        return out
    return evaluate


def stand_in(c, order='forward', fault=None, safe=False):
    o, z0, l0, star, dz, ref, margins = oracle_run(c, safe=safe)
    real = orc.prior_inbox
    if fault == 'box_on_T':   # the box tested on T(x) against +-1, not on x
        orc.prior_inbox = lambda x: real(sg.T32(c, x))
    try:
        return sg.slice_sample(o, c, z0, l0, star, dz, SEED, OFF, evaluate=kernel_likelihood(c, order, fault, safe))
    finally:
        orc.prior_inbox = real


def held(c, r, what):
    """what the GPU tests assert of a kernel's output, in their order"""
    o, z0, l0, star, dz, ref, margins = oracle_run(c)
    sg.hold(c, sl.as_kernel(r), r['logl'], ref, margins, l0, star, what=what)


def test_tables_reach_every_instantiation_they_claim():
    from tests.fused_like_check import units
    assert [(units(c.D), c.family) for c in sg.NVP_TABLE] == [(1, 'logistic'), (2, 'poisson'), (3, 'logistic'), (4, 'logistic'), (4, 'poisson')]
    assert [(c.D, c.n, c.scale, c.S) for c in sg.NVP_TABLE] == [(2, 257, 5.0, 4), (33, 257, 3.0, 4), (65, 64, 5.0, 3), (128, 65, 5.0, 3),
                                                                (128, 300, 3.0, 2)]
    assert all(not c.affine for c in sg.NVP_TABLE) and all(c.affine for c in sg.NVP_EXTRA)
    # passes of 64 rows, four to a group: two groups with a ragged second, exactly one pass, ragged last passes
    assert {c.n for c in sg.NVP_TABLE} == {257, 64, 65, 300} and 257 > 4 * 64 and 257 % 64 != 0
    assert {sg.spline_key(sc) for sc in sg.SPLINE_TABLE} == {(1, 1), (2, 1), (3, 1), (4, 1), (1, 2)}
    assert [sc.case.D for sc in sg.SPLINE_TABLE if sc.golden is None] == [2, 33, 70, 100]
    assert {sc.case.family for sc in sg.SPLINE_TABLE} == set(gk.FAMILIES) and {sc.case.n for sc in sg.SPLINE_TABLE} == {65, 257}
    for sc in sg.SPLINE_TABLE:
        assert sc.C % 16 != 0 and sc.C > 16 and sc.case.S == (3 if sc.case.D <= 33 else 2)
        assert sc.golden is None or os.path.exists(os.path.join(ROOT, 'tests', 'golden', sc.golden))
    for c in CASES + [sc.case for sc in sg.SPLINE_TABLE]:
        d = sg.data_of(c)
        assert d['family'] == c.family and d['n'] == c.n and d['at'].shape == (c.D, (c.n + 63) // 64 * 64)
        sd, mu = sg.affine_of(c)
        assert sd.dtype == mu.dtype == np.float32 and (np.any(mu != 0) and len(set(sd)) > 1) == c.affine


@pytest.mark.parametrize('cid', sorted(BY_ID))
def test_cap_condition_holds_for_the_nvp_table(cid):
    c = BY_ID[cid]
    shares = [sl.near_share(oracle_run(c, s)[6]) for s in range(3)]
    o, z0, l0, star, dz, ref, margins = oracle_run(c)
    print('NEAR %-26s S %d  %s   n_eval %.1f n_call %.1f per walker' % (cid, c.S, '  '.join('%.3f' % v for v in shares),
                                                                       ref['n_eval'].mean(), ref['n_call'].mean()))
    assert max(shares) <= 1.0 - sl.AGREE, (cid, shares)
    assert len(l0) % 4 != 0 and np.all(l0 > star)
    assert ref['n_move'].mean() > 0.9 * c.S   # (the walk is a walk: nearly every update moves)
    assert ref['n_call'].sum() < ref['n_eval'].sum()   # (there are candidates whose likelihood a kernel skips)


@pytest.mark.parametrize('order', ['forward', 'reversed', 'pairwise'])
@pytest.mark.parametrize('cid', sorted(BY_ID))
def test_a_legal_evaluation_passes(cid, order):
    c = BY_ID[cid]
    held(c, stand_in(c, order), '%s %s' % (cid, order))


PLANTED = [('t_mean', 'poisson-d7-n65-affine'), ('offset', 'logistic-d2-n257'), ('offset', 'poisson-d128-n300'),
           ('padding', 'logistic-d2-n257'), ('padding', 'poisson-d33-n257'), ('padding', 'logistic-d128-n65'),
           ('family', 'logistic-d65-n64'), ('family', 'poisson-d33-n257'), ('box_on_T', 'logistic-d2-n257'), ('box_on_T', 'poisson-d7-n65-affine')]


@pytest.mark.parametrize('fault,cid', PLANTED, ids=['%s-%s' % p for p in PLANTED])
def test_a_planted_fault_fails(fault, cid):
    c = BY_ID[cid]
    r = stand_in(c, 'forward', fault)
    with pytest.raises(AssertionError):
        held(c, r, '%s with %s wrong' % (cid, fault))


@pytest.mark.parametrize('cid', ['logistic-d2-n257', 'poisson-d33-n257'])
def test_the_safe_rule_check_passes_the_rule_and_fails_a_finite_value(cid):
    """NaN offsets from a start with finite logl: under the safe rule nothing moves; a kernel that maps the non-finite logL to a
    finite value walks, and the check fails it"""
    c = BY_ID[cid]
    o, z0, l0, star, dz, ref, margins = oracle_run(c, safe=True)
    assert np.all(np.isfinite(l0)) and np.all(ref['n_move'] == 0) and np.all(ref['n_call'] > 0)
    good = stand_in(c, 'forward', None, safe=True)
    sl.check_nothing_moves(sl.as_kernel(good), ref, z0, l0, good['z'], good['logl'], what='safe')
    bad = stand_in(c, 'forward', 'finite', safe=True)
    assert bad['n_move'].sum() > 0
    with pytest.raises(AssertionError):
        sl.check_nothing_moves(sl.as_kernel(bad), ref, z0, l0, bad['z'], bad['logl'], what='finite')


def test_the_oracle_likelihood_is_put_back():
    real = orc.loglike
    with pytest.raises(RuntimeError):
        with sg.oracle_likelihood(lambda x: np.zeros(len(x))):
            assert orc.loglike is not real and orc.loglike('anything', np.zeros((3, 2)), 7.0, None).tolist() == [0.0, 0.0, 0.0]
            raise RuntimeError('inside')
    assert orc.loglike is real


# ---- the library, the build and the bindings, without a device --------------------------------------------------------------------
def test_header_and_signatures_name_the_new_entries():
    from nnest_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, text), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['nnest_slice_glm_steps']) == len(_lib.SIGNATURES['nnest_slice_steps']) + 2
    assert _lib.SIGNATURES['nnest_spline_slice_glm_steps'] == _lib.SIGNATURES['nnest_slice_glm_steps']   # (one form: no flags word)
    lib = _lib.load()
    assert lib.nnest_hip_version() == 15 and all(hasattr(lib, n) for n in NEW)


def test_makefile_builds_both_units_and_the_spline_one_without_machine_licm():
    mk = open(os.path.join(ROOT, 'nnest_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    assert 'nnest_slice_glm.hip' in srcs and 'nnest_spline_slice_glm.hip' in srcs
    licm_off = re.search(r'^LICM_OFF := (.*)$', mk, re.M).group(1).split()
    assert 'nnest_spline_slice_glm' in licm_off and 'nnest_slice_glm' not in licm_off
    for unit in ('nnest_slice_glm', 'nnest_spline_slice_glm'):
        deps = re.search(r'^%s\.o: (.*)$' % unit, mk, re.M).group(1)
        assert 'slice_glm.h' in deps and 'glm_data.h' in deps, unit


def test_argument_errors_need_no_device():
    """the checks in front of the handle: a NULL descriptor, a bad family, too many rows, T half given, the rule's ranges"""
    import ctypes
    from nnest_amd import _lib
    lib = _lib.load()
    E_ARG = 1   # NNEST_E_ARG (include/nnest_hip.h)
    good = dict(at=1, y=1, o=1, logl0=0.0, n=64, ld=64, D=3, family=0)

    def call(fn, spec, t_std=None, t_mean=None, width=0.5, steps=2, max_stepout=8, max_shrink=32):
        s = None if spec is None else ctypes.byref(_lib.GlmSpec(spec['at'], spec['y'], spec['o'], spec['logl0'], spec['n'], spec['ld'], spec['D'],
                                                               spec['family']))
        rc = fn(None, s, t_std, t_mean, None, None, None, -1.0, width, steps, 4, max_stepout, max_shrink, None, 1, 0, None, None, None, None, None)
        return rc, (lib.nnest_hip_last_error() or b'').decode()

    for fn in (lib.nnest_slice_glm_steps, lib.nnest_spline_slice_glm_steps):
        for want, kw in (('glm is NULL', dict(spec=None)), ('glm: family=7', dict(spec=dict(good, family=7))),
                         ('glm: n=65537', dict(spec=dict(good, n=65537, ld=65600))), ('glm: logl0=', dict(spec=dict(good, logl0=float('nan')))),
                         ('both or neither', dict(spec=good, t_std=1)), ('max_shrink=61', dict(spec=good, max_shrink=61)),
                         ('max_stepout=-1', dict(spec=good, max_stepout=-1)), ('width=0', dict(spec=good, width=0.0)),
                         ('NULL handle', dict(spec=good))):
            rc, text = call(fn, **kw)
            assert rc == E_ARG and want in text, (want, rc, text)
    for fn in (lib.nnest_slice_glm_check, lib.nnest_spline_slice_glm_check):
        assert fn(None, 3) == E_ARG and b'NULL handle' in lib.nnest_hip_last_error()


class _Bound(object):
    """a flow object with the bindings' methods and no handle: what slice_steps refuses before it touches one"""

    def __init__(self, cls, **sym):
        self.__class__ = type('Fake' + cls.__name__, (cls,), {'__del__': lambda self: None, '__init__': lambda self: None})
        self._sym = sym
        self.D = 3


def test_bindings_refuse_without_a_launch():
    from nnest_amd import flow
    from nnest_amd.spline import HipSpline
    data = gk.make_like(3, 10, 'logistic', 1).hip_like_glm
    nvp = _Bound(flow.HipNVP, slice=None, slice_glm=None)
    with pytest.raises(ValueError, match='like_glm goes with like_id=None'):
        nvp.slice_steps(0, 5.0, None, None, 0.0, 0.5, 2, like_glm=data)
    with pytest.raises(ValueError, match='t_std and t_mean go only with a like_glm'):
        nvp.slice_steps(0, 5.0, None, None, 0.0, 0.5, 2, t_std=np.ones(3), t_mean=np.zeros(3))
    none = _Bound(flow.HipNVP, slice=None)   # (a family without the entry: MAF, Cholesky)
    with pytest.raises(NotImplementedError, match='regression likelihood of user data'):
        none.slice_steps(None, 1.0, None, None, 0.0, 0.5, 2, like_glm=data)
    with pytest.raises(NotImplementedError):
        none.slice_glm_refusal()
    sp = _Bound(HipSpline, slice=None, slice_glm=None)
    for form in ('wave', 'pair', 'quad'):
        with pytest.raises(ValueError, match='team form only'):
            sp._slice_glm_form_args(form)
    assert sp._slice_glm_form_args(None) == () and sp._slice_glm_form_args('team') == ()
    with pytest.raises(ValueError, match='one slice kernel form'):
        nvp._slice_glm_form_args('team')
    import inspect
    assert "slice_glm='nnest_slice_glm_steps'" in inspect.getsource(flow.HipNVP.__init__)
    assert "slice_glm='nnest_spline_slice_glm_steps'" in inspect.getsource(HipSpline.__init__)


def test_slice_rounds_takes_exactly_one_likelihood():
    from nnest_amd.slice_rounds import slice_rounds
    data = gk.make_like(3, 10, 'logistic', 1).hip_like_glm
    for kw in (dict(), dict(like_id=0, like_glm=data), dict(loglike=len, like_glm=data), dict(loglike=len, like_id=0)):
        with pytest.raises(ValueError, match='exactly one of'):
            slice_rounds(None, None, None, 0.0, 0.5, 2, **kw)
    with pytest.raises(ValueError, match='unit box without derived'):
        slice_rounds(None, None, None, 0.0, 0.5, 2, like_glm=data, num_derived=1)
    with pytest.raises(ValueError, match='only with a like_glm'):
        slice_rounds(None, None, None, 0.0, 0.5, 2, like_id=0, t_std=np.ones(3), t_mean=np.zeros(3))
