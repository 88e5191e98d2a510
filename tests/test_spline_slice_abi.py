"""CPU checks of the spline flow's slice proposal at the C-ABI and Python boundaries (no compute calls without a GPU): the header
declares and the library exports nnest_spline_slice_steps / nnest_spline_slice_form_for, HipSpline has a slice method of its own,
and HipCholesky no longer inherits the NVP's (which would hand its handle to nnest_slice_steps)."""
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


def test_hipspline_has_its_own_slice_method():
    from nnest_amd.flow import _HipFlow
    from nnest_amd.spline import HipSpline
    assert 'slice_steps' in HipSpline.__dict__
    assert 'slice_form_for' in HipSpline.__dict__
    assert HipSpline.slice_steps is not _HipFlow.slice_steps
    assert HipSpline.fill_slice_noise is _HipFlow.fill_slice_noise   # shape-free: the directions of every flow


def test_hipcholesky_does_not_inherit_the_nvp_slice_method():
    from nnest_amd.cholesky import HipCholesky
    from nnest_amd.flow import _HipFlow
    assert 'slice_steps' in HipCholesky.__dict__
    assert HipCholesky.slice_steps is not _HipFlow.slice_steps


def test_run_py_takes_the_proposal():
    src = open(os.path.join(ROOT, 'nnest_amd', 'run.py')).read()
    assert "'--mcmc_proposal'" in src and 'mcmc_proposal=args.mcmc_proposal' in src
