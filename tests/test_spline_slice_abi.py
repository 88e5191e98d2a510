"""CPU checks of the spline flow's slice proposal at the C-ABI and Python boundaries (no compute calls without a GPU): the header
declares and the library exports nnest_spline_slice_steps / nnest_spline_slice_form_for, HipSpline's slice proposal goes to its own
entry point, and HipCholesky's handle cannot reach the NVP's (nnest_slice_steps)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nnest_spline_slice_steps', 'nnest_spline_slice_form_for')


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'nnest_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(nnest_[a-z0-9_]+)\s*\(', text))


def test_header_declares_and_library_exports_the_spline_slice_entry_points():
    from nnest_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.nnest_hip_version() == 15


def test_spline_slice_argument_errors_are_reported_not_thrown():
    from nnest_amd import _lib
    lib = _lib.load()
    assert lib.nnest_spline_slice_form_for(None, 100, 0) == -1
    lk = _lib.like_spec(0, 5.0)
    rc = lib.nnest_spline_slice_steps(None, ctypes.byref(lk), None, None, None, 0.0, 0.5, 2, 8, 8, 32, 0, None, 0, 0, None, None, None,
                                      None, None)
    assert rc == 1 and b'NULL' in lib.nnest_hip_last_error()


def bound(cls, family, **named):
    """an instance of the flow class with its C symbols bound as its constructor binds them, without a handle (no GPU)"""
    from nnest_amd import _lib
    o = object.__new__(cls)
    o._lib = _lib.load()
    o._h = None
    o._bind(family, **named)
    return o


def test_hipspline_has_its_own_slice_method():
    """one implementation (_HipFlow.slice_steps); what makes it the spline's is the C symbol HipSpline binds and its flags word"""
    import inspect
    import pytest
    from nnest_amd import _lib
    from nnest_amd.flow import _HipFlow, HipNVP
    from nnest_amd.spline import HipSpline
    assert 'slice_steps' in HipSpline.__dict__
    assert 'slice_form_for' in HipSpline.__dict__
    assert HipSpline.slice_steps is _HipFlow.slice_steps and HipNVP.slice_steps is _HipFlow.slice_steps   # one body
    assert HipSpline.fill_slice_noise is _HipFlow.fill_slice_noise   # shape-free: the directions of every flow
    assert "slice='nnest_spline_slice_steps'" in inspect.getsource(HipSpline.__init__)
    assert "slice='nnest_slice_steps'" in inspect.getsource(HipNVP.__init__)
    lib = _lib.load()
    sp = bound(HipSpline, 'nnest_spline', slice='nnest_spline_slice_steps')
    assert sp._sym['slice'] is lib.nnest_spline_slice_steps and sp._sym['slice'] is not lib.nnest_slice_steps
    # the one difference between the two signatures: the spline's flags word (NNEST_SPLINE_SLICE_FORM)
    assert [sp._slice_form_args(f) for f in (None, 'wave', 'team', 'pair')] == [(0,), (1,), (2,), (3,)]
    with pytest.raises(ValueError):
        sp._slice_form_args('solo')
    nvp = bound(HipNVP, 'nnest_nvp', slice='nnest_slice_steps')
    assert nvp._sym['slice'] is lib.nnest_slice_steps and nvp._slice_form_args(None) == ()
    with pytest.raises(ValueError):
        nvp._slice_form_args('team')
    assert len(_lib.SIGNATURES['nnest_spline_slice_steps']) == len(_lib.SIGNATURES['nnest_slice_steps']) + 1


def test_hipcholesky_does_not_inherit_the_nvp_slice_method():
    """a family that binds no `slice` symbol cannot reach another family's entry point: the shared method refuses, and the sampler is
    told to take the round driver"""
    import inspect
    import pytest
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.maf import HipMAF
    assert 'slice' not in inspect.getsource(HipCholesky.__init__)
    for cls, family in ((HipCholesky, 'nnest_chol'), (HipMAF, 'nnest_nvp')):
        o = bound(cls, family)
        assert 'slice' not in o._sym
        assert o.supports_fused_slice(1000) is False
        with pytest.raises(NotImplementedError):
            o.slice_steps(0, 5.0, None, None, -1e9, 0.5, 2)


def test_run_py_takes_the_proposal():
    src = open(os.path.join(ROOT, 'nnest_amd', 'run.py')).read()
    assert "'--mcmc_proposal'" in src and 'mcmc_proposal=args.mcmc_proposal' in src
