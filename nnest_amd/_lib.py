"""ctypes binding of libnnest_hip.so (include/nnest_hip.h).

The shared library is the product: there is no CPU or PyTorch fallback.  Importing this module
without the built library raises; calling into it without a GPU returns the library's own error.
`import torch` happens first so that the library's libamdhip64.so.7 dependency resolves to the HIP
runtime PyTorch-ROCm has already loaded (one runtime per process; device pointers and streams are
shared with torch tensors).
"""
import os
import ctypes
import math

import numpy as np
import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NNEST_HIP_LIB', os.path.join(_HERE, 'libnnest_hip.so'))  # override: developer A/B builds only

NNEST_OK = 0
NNEST_E_UNSUPPORTED = 3
LIKE_IDS = {'rosenbrock': 0, 'gaussmix': 1, 'himmelblau': 2, 'gaussian': 3, 'eggbox': 4, 'shell': 5, 'double_shell': 6}
MH_DYNAMIC_STEP = 1      # per 16-walker group
MH_UNCONSTRAINED = 2
MH_DYNAMIC_BATCH = 4     # over the whole launch, as the reference (sampler.py:422-431); lag in bits 8..11
MH_FORMS = {None: 0, 'auto': 0, 'image': 1, 'reg': 2, 'team': 3, 'quad': 4, 'quad1': 5, 'solo': 6}
MH_FORM_NAMES = {v: k for k, v in MH_FORMS.items() if isinstance(k, str) and v}
MH_DEFAULT_LAG = 4      # steps between a step and the scale that reflects its batch-wide count
MH_WARM_STEPS = 16      # exact steps in front of the lagged rule where the form implements them (NNEST_MH_WARM)
MH_SYNC_ZERO_NEXT, MH_SYNC_ZERO_PREV = 1 << 29, 1 << 30   # sync_dev as one half of a double buffer (include/nnest_hip.h)
MH_ALL_MOVED = 1 << 30  # n_accept words: every coordinate of the chain's last x differs from its first (include/nnest_hip.h)
MH_SOLO_LAG = 8         # ... where the solo form runs (its steps are shorter: the same ~10 us of latency)
TRAIN_RESUME = 1
TRAIN_FINALIZE = 2
TRAIN_ONE_CU = 4


def mh_flags(dynamic=False, free=False, lag=None, form=None, warm=0):
    """flags word of nnest_mh_constrained_steps.  dynamic: False | True / 'batch' (the reference's batch-wide rule) |
    'group' (per 16 walkers); warm: NNEST_MH_WARM, exact steps in front of a lagged batch rule"""
    fl = MH_UNCONSTRAINED if free else 0
    if dynamic == 'group':
        fl |= MH_DYNAMIC_STEP
    elif dynamic:
        fl |= MH_DYNAMIC_BATCH | ((MH_DEFAULT_LAG if lag is None else int(lag)) & 15) << 8
        fl |= (min(int(warm or 0), 255) & 255) << 20
    return fl | (MH_FORMS[form] << 16)


class NnestHipError(RuntimeError):
    code = None   # NNEST_E_* of the failing call, when it came from the library


class LikeSpec(ctypes.Structure):
    """nnest_like_t (include/nnest_hip.h): likelihood id, transform scale, parameters"""
    _fields_ = [('id', ctypes.c_int), ('scale', ctypes.c_float), ('params', ctypes.c_float * 6)]


def like_spec(like_id, scale, params=None):
    lk = LikeSpec()
    lk.id = int(like_id)
    lk.scale = float(scale)
    for i, v in enumerate(params or ()):
        lk.params[i] = float(v)
    return lk


class EnsMoves(ctypes.Structure):
    """nnest_ens_moves_t (include/nnest_hip.h): the weights of the stretch and the DE move, the DE scale (0: emcee's defaults)"""
    _fields_ = [('w_stretch', ctypes.c_float), ('w_de', ctypes.c_float), ('de_gamma0', ctypes.c_float), ('de_sigma', ctypes.c_float)]


def ens_moves(moves, what='ensemble'):
    """the reference's `moves` dict (nnest/ensemble.py:113-127: names case-insensitive, weights) as an EnsMoves: {'stretch': w, 'de': w}.
    None stays None (the stretch move alone); an EnsMoves passes through.  'kde' and 'snooker' are emcee moves this build does not
    have (NotImplementedError); any other name, a negative or non-finite weight and weights that are all 0 are ValueError."""
    if moves is None or isinstance(moves, EnsMoves):
        return moves
    w = {'stretch': 0.0, 'de': 0.0}
    for k, v in dict(moves).items():
        name = str(k).lower()
        if name in ('kde', 'snooker'):
            raise NotImplementedError("%s: the '%s' move is not built (emcee's 'stretch' and 'de' moves are)" % (what, k))
        if name not in w:
            raise ValueError("%s: unknown move '%s'" % (what, k))
        v = float(v)
        if not (v >= 0.0 and v != float('inf')):
            raise ValueError("%s: the weight of move '%s' is %r (finite and not negative)" % (what, k, v))
        w[name] += v
    if w['stretch'] + w['de'] <= 0.0:
        raise ValueError('%s: the weights of the moves are all 0' % what)
    return EnsMoves(w['stretch'], w['de'], 0.0, 0.0)


def ens_moves_mix(mv, C=None, what='ensemble'):
    """whether a run with these (parsed) moves has a DE step in it; with C, the DE move's own need: two partners in either set"""
    mix = mv is not None and mv.w_de > 0.0
    if mix and C is not None and C < 4:
        raise ValueError('%s: %d walkers: the DE move needs two partners in either set (at least 4 walkers)' % (what, C))
    return mix


def moves_ref(mv):
    """the `moves` argument of a C entry: a pointer to the struct, or NULL"""
    return None if mv is None else ctypes.byref(mv)


class GdataSpec(ctypes.Structure):
    """nnest_gdata_t (include/nnest_hip.h): the Gaussian likelihood from user data -- device pointers of mu [D] and R [D, D], logl0, D"""
    _fields_ = [('mu_dev', ctypes.c_void_p), ('r_dev', ctypes.c_void_p), ('logl0', ctypes.c_double), ('D', ctypes.c_int)]


class GlmSpec(ctypes.Structure):
    """nnest_glm_t (include/nnest_hip.h): a regression likelihood of user data -- device pointers of A^T [D, ld], y [ld] and the
    offset [ld], logl0, n, ld, D, family (GLM_FAMILIES)"""
    _fields_ = [('at_dev', ctypes.c_void_p), ('y_dev', ctypes.c_void_p), ('o_dev', ctypes.c_void_p), ('logl0', ctypes.c_double),
                ('n', ctypes.c_int), ('ld', ctypes.c_int), ('D', ctypes.c_int), ('family', ctypes.c_int)]


class GaussPriorSpec(ctypes.Structure):
    """nnest_gauss_prior_t (include/nnest_hip.h): independent normal priors -- device pointers of m [D] and r = 1 / sigma [D], logc, D"""
    _fields_ = [('m_dev', ctypes.c_void_p), ('r_dev', ctypes.c_void_p), ('logc', ctypes.c_double), ('D', ctypes.c_int)]


GLM_FAMILIES = {'logistic': 0, 'poisson': 1}   # NNEST_GLM_LOGISTIC, NNEST_GLM_POISSON


class TrainResult(ctypes.Structure):
    _fields_ = [('epochs_run', ctypes.c_int), ('best_epoch', ctypes.c_int),
                ('best_validation_loss', ctypes.c_float), ('last_train_loss', ctypes.c_float),
                ('counter', ctypes.c_int), ('stopped', ctypes.c_int)]


_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_d = ctypes.c_double
_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32

# name -> argtypes; every entry point include/nnest_hip.h declares (checked by tests/test_abi.py)
SIGNATURES = {
    'nnest_hip_version': [],
    'nnest_hip_last_error': [],
    'nnest_hip_device_info': [ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.c_char_p, _i],
    'nnest_nvp_create': [_i, _i, _i, _i, ctypes.POINTER(_vp)],
    'nnest_spline_create': [_i, _i, _i, _i, _f, ctypes.POINTER(_vp)],
    'nnest_spline_destroy': [_vp],
    'nnest_spline_num_params': [_vp],
    'nnest_spline_load_weights': [_vp, _vp, _vp, _vp],
    'nnest_spline_store_weights': [_vp, _vp, _vp, _vp],
    'nnest_nvp_create_scaled': [_i, _i, _i, _i, _i, ctypes.POINTER(_vp)],
    'nnest_maf_create': [_i, _i, _i, _i, ctypes.POINTER(_vp)],
    'nnest_maf_num_groups': [_vp],
    'nnest_maf_train_epoch': [_vp, _vp, _i, _i, _f, _f, _vp, _vp],
    'nnest_nvp_destroy': [_vp],
    'nnest_nvp_num_params': [_vp],
    'nnest_nvp_set_base': [_vp, _f],
    'nnest_nvp_vjp': [_vp, _vp, _vp, _f, _i, _vp, _vp, _vp],
    'nnest_nvp_adam_step': [_vp, _vp, _f, _f, _vp],
    'nnest_spline_set_base': [_vp, _f],
    'nnest_nvp_load_weights': [_vp, _vp, _vp],
    'nnest_nvp_store_weights': [_vp, _vp, _vp],
    'nnest_nvp_device_ptrs': [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp)],
    'nnest_nvp_store_adam': [_vp, _vp, _vp, _vp],
    'nnest_nvp_load_adam': [_vp, _vp, _vp, _vp],
    'nnest_nvp_adam_state': [_vp, ctypes.POINTER(_i), _i, _i, _vp],
    'nnest_nvp_forward': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_nvp_inverse': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_nvp_log_probs': [_vp, _vp, _vp, _i, _vp],
    'nnest_nvp_inverse_loglike': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    'nnest_loglike': [_vp, _vp, _vp, _i, _i, _vp],
    'nnest_mh_constrained_steps': [_vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _vp, _vp, _u64, _u64,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_mh_sync_words': [_i],
    'nnest_mh_form_for': [_vp, _i, _i],
    'nnest_spline_mh_form_for': [_vp, _i, _i],
    'nnest_spline_slice_form_for': [_vp, _i, _i],
    'nnest_spline_slice_steps': [_vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _i, _i, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp],
    'nnest_spline_train_form': [_vp, _i],
    'nnest_spline_forward': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_spline_inverse': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_spline_log_probs': [_vp, _vp, _vp, _i, _vp],
    'nnest_spline_inverse_loglike': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    'nnest_spline_mh_constrained_steps': [_vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _vp, _vp, _u64, _u64,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_spline_vjp': [_vp, _vp, _vp, _f, _i, _vp, _vp, _vp],
    'nnest_spline_adam_step': [_vp, _vp, _f, _f, _vp],
    'nnest_spline_actnorm_init': [_vp, _vp, _i, _vp],
    'nnest_spline_loss_grad': [_vp, _vp, _i, _vp, _vp, _vp],
    'nnest_spline_train': [_vp, _vp, _i, _vp, _i, _vp, _vp, _u64, _f, _i, _i, _i, _f, _f, _vp, _vp, _vp],
    'nnest_chol_create': [_i, ctypes.POINTER(_vp)],
    'nnest_chol_destroy': [_vp],
    'nnest_chol_num_params': [_vp],
    'nnest_chol_set_base': [_vp, _f],
    'nnest_chol_load_weights': [_vp, _vp, _vp],
    'nnest_chol_store_weights': [_vp, _vp, _vp],
    'nnest_chol_forward': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_chol_inverse': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_chol_log_probs': [_vp, _vp, _vp, _i, _vp],
    'nnest_chol_loss_grad': [_vp, _vp, _i, _vp, _vp, _vp],
    'nnest_chol_adam_step': [_vp, _vp, _f, _f, _vp],
    'nnest_mh_num_groups': [_vp, _i],
    'nnest_mh_fill_noise': [_vp, _vp, _i, _i, _i, _u64, _u64, _vp],
    'nnest_nvp_train_form': [_vp, _i, _i, _vp],
    'nnest_nvp_train': [_vp, _vp, _i, _vp, _i, _vp, _vp, _u64, _f, _i, _i, _i, _f, _f, _i, _i, _vp, _vp, _vp],
    'nnest_nvp_loss_grad': [_vp, _vp, _i, _vp, _vp, _vp],
    'nnest_training_jitter': [_vp, _i, _i, _vp, _vp],
    'nnest_format_rows_e5': [_vp, ctypes.c_long, _i, _vp, ctypes.c_long, _i],
    'nnest_format_scalar_rows': [ctypes.c_char_p, _vp, _vp, ctypes.c_long, _vp, ctypes.c_long],
    'nnest_host_mcmc_consume': [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.c_longlong,
                                _d, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong],
    'nnest_host_h_update': [_d, _vp, _vp, _vp, _vp, _vp, ctypes.c_longlong],
    'nnest_slice_steps': [_vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _i, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp],
    'nnest_slice_fill_noise': [_vp, _i, _i, _i, _u64, _u64, _vp],
    'nnest_slice_rounds_create': [_i, _i, _i, ctypes.POINTER(_vp)],
    'nnest_slice_rounds_destroy': [_vp],
    'nnest_slice_rounds_begin': [_vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_slice_rounds_screen': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_slice_rounds_advance': [_vp, _vp, _vp, _vp, _vp],
    'nnest_slice_rounds_finish': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_ensemble_work_words': [_i, _i],
    'nnest_ensemble_fill_noise': [_vp, _vp, _i, _i, _u64, _u64, _vp],
    'nnest_ensemble_max_walkers': [_vp, _i],
    'nnest_ensemble_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _i, _d, _vp],
    'nnest_spline_ensemble_max_walkers': [_vp, _i],
    'nnest_spline_ensemble_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _i, _d, _vp],
    'nnest_ensemble_x_max_walkers': [_i, _i],
    'nnest_ensemble_x_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _u64, _u64, _i, _d, _vp],
    'nnest_ensemble_rounds_propose': [_vp, _i, _i, _i, _i, _i, _u64, _u64, _vp, _vp, _vp],
    'nnest_ensemble_rounds_accept': [_vp, _i, _i, _i, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _i, _d, _vp],
    'nnest_ensemble_moves_threshold': [_vp],
    'nnest_ensemble_moves_max_walkers': [_vp, _i, _vp],
    'nnest_ensemble_x_moves_max_walkers': [_i, _i, _vp],
    'nnest_ensemble_moves_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _i, _d, _vp,
                                   _vp],
    'nnest_ensemble_x_moves_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _u64, _u64, _i, _d, _vp,
                                     _vp],
    'nnest_ensemble_rounds_moves_propose': [_vp, _i, _i, _i, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp],
    'nnest_ensemble_rounds_moves_accept': [_vp, _i, _i, _i, _i, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _i, _d, _vp, _vp],
    'nnest_ensemble_fill_moves': [_vp, _vp, _vp, _vp, _i, _i, _i, _u64, _u64, _vp, _vp],
    'nnest_mcmc_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64, _u64, _vp],
    'nnest_spline_mcmc_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64, _u64,
                                _vp],
    'nnest_mcmc_fill_noise': [_vp, _vp, _i, _i, _i, _u64, _u64, _u64, _vp],
    # the tempered target of the two entries above: their arguments plus `double beta` before `stream`
    'nnest_mcmc_tempered_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64,
                                  _u64, _d, _vp],
    'nnest_spline_mcmc_tempered_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                         _u64, _u64, _d, _vp],
    # the mixed walk: the tempered entries' arguments plus `int global_every, int *n_accept_global_dev` before `stream`
    'nnest_mcmc_mixed_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64,
                               _u64, _d, _i, _vp, _vp],
    'nnest_spline_mcmc_mixed_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                      _u64, _u64, _d, _i, _vp, _vp],
    'nnest_mcmc_mixed_check': [_vp, _i],
    'nnest_spline_mcmc_mixed_check': [_vp, _i],
    # the adaptive walk: the mixed entries' arguments up to n_accept_global_dev, then `const double *step_in_dev, double *step_out_dev,
    # double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept` before `stream`
    'nnest_mcmc_adapt_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64,
                               _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_spline_mcmc_adapt_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                      _u64, _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_mcmc_adapt_check': [_vp, _i],
    'nnest_spline_mcmc_adapt_check': [_vp, _i],
    # the Gaussian likelihood from user data: the adaptive entries' arguments with `const nnest_gdata_t *gdata` for `like`;
    # (gdata, t_dev, logl_dev, N, D, stream); (handle, D)
    'nnest_mcmc_gdata_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64,
                               _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_spline_mcmc_gdata_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                      _u64, _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_loglike_gdata': [_vp, _vp, _vp, _i, _i, _vp],
    'nnest_mcmc_gdata_check': [_vp, _i],
    'nnest_spline_mcmc_gdata_check': [_vp, _i],
    # the regression likelihoods of user data: the same three forms with `const nnest_glm_t *glm`
    'nnest_mcmc_glm_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64, _u64,
                             _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_spline_mcmc_glm_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                    _u64, _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_loglike_glm': [_vp, _vp, _vp, _i, _i, _vp],
    'nnest_mcmc_glm_check': [_vp, _i],
    'nnest_spline_mcmc_glm_check': [_vp, _i],
    # the slice proposal on them: nnest_slice_steps's arguments with `const nnest_glm_t *glm, const float *t_std_dev, const float
    # *t_mean_dev` for `like` (the spline's takes no flags word: one form); (handle, D)
    'nnest_slice_glm_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _i, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp],
    'nnest_spline_slice_glm_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _i, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp],
    'nnest_slice_glm_check': [_vp, _i],
    'nnest_spline_slice_glm_check': [_vp, _i],
    # the constrained Metropolis proposal on them: nnest_mh_constrained_steps's arguments with `const nnest_glm_t *glm, const float
    # *t_std_dev, const float *t_mean_dev` for `like`; (handle, D, C, flags)
    'nnest_mh_glm_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_spline_mh_glm_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _f, _i, _i, _i, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_mh_glm_check': [_vp, _i, _i, _i],
    'nnest_spline_mh_glm_check': [_vp, _i, _i, _i],
    # their pointwise predictive statistics: (S, n); (glm, t_dev, stats_dev, partials_dev, S, D, stream)
    'nnest_glm_pointwise_groups': [_i, _i],
    'nnest_glm_pointwise': [_vp, _vp, _vp, _vp, _i, _i, _vp],
    'nnest_glm_predict': [_vp, _vp, _vp, _vp, _i, _i, _vp],
    # the matrix of terms (glm, t_dev, out_dev, S, D, stream); Pareto-smoothed leave-one-out: (S); (S, n);
    # (glm, t_dev, stats_dev, out_dev, work_dev, S, D, stream)
    'nnest_glm_terms': [_vp, _vp, _vp, _i, _i, _vp],
    'nnest_glm_psis_tail_cap': [_i],
    'nnest_glm_psis_work_bytes': [_i, _i],
    'nnest_glm_psis': [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    # gradient and curvature at one theta: (n, D); (glm, theta_dev, out_dev, partials_dev, D, stream); the Newton step:
    # (curv_dev, prior or NULL, theta_dev, step_dev, chol_dev, info_dev, D, stream)
    'nnest_glm_curv_groups': [_i, _i],
    'nnest_glm_curv': [_vp, _vp, _vp, _vp, _i, _vp],
    'nnest_glm_newton_solve': [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    # normal priors beside them: the glm entries' arguments with `const nnest_gauss_prior_t *prior` after `glm`;
    # (prior, t_dev, logp_dev, N, D, stream); (handle, D)
    'nnest_mcmc_glm_prior_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                   _u64, _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_spline_mcmc_glm_prior_steps': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f,
                                          _u64, _u64, _u64, _d, _i, _vp, _vp, _vp, _vp, _u32, _d, _d, _vp],
    'nnest_logprior_gauss': [_vp, _vp, _vp, _i, _i, _vp],
    'nnest_mcmc_glm_prior_check': [_vp, _i],
    'nnest_spline_mcmc_glm_prior_check': [_vp, _i],
    # (logl_dev, N, beta, ess_fraction, out_dev [4], m_dev [N] int64, stream)
    'nnest_smc_reweight': [_vp, _i, _d, _d, _vp, _vp, _vp],
    # (m_dev, N, D, seed, stage, theta_in_dev, logl_in_dev, anc_out_dev, theta_out_dev, logl_out_dev, stream)
    'nnest_smc_resample': [_vp, _i, _i, _u64, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    'nnest_importance_groups': [_i, _i],
    'nnest_importance_check': [_vp, _i],
    'nnest_spline_importance_check': [_vp, _i],
    'nnest_importance_evidence': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u64, _u64, _vp],
    'nnest_spline_importance_evidence': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u64, _u64, _vp],
    'nnest_importance_glm_check': [_vp, _i],
    'nnest_spline_importance_glm_check': [_vp, _i],
    'nnest_importance_glm_evidence': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u64, _u64, _vp],
    'nnest_spline_importance_glm_evidence': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u64, _u64, _vp],
    'nnest_importance_fill_noise': [_vp, _i, _i, _u64, _u64, _vp],
    'nnest_host_prior_consume': [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 ctypes.c_longlong, _d, ctypes.c_longlong, ctypes.c_longlong, _d, _d, _i],
    'nnest_chain_stats_work_words': [_i, _i, _i],
    'nnest_chain_autocorr_work_words': [_i, _i, _i],
    'nnest_chain_autocorr': [_vp, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp, _vp],
    'nnest_chain_stats': [_vp, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    'nnest_chain_stats_chains': [_vp, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp],
    'nnest_chain_stats_prepare': [_vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    'nnest_chain_stats_lags': [_vp, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, _vp, _i, _i, _i, _vp, _vp, _vp],
    'nnest_chain_stats_advance': [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    'nnest_chain_stats_finish': [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
}
CHAIN_STATS_ALL_LAGS, CHAIN_STATS_NO_ESS, CHAIN_STATS_RHAT_AT_MEAN = 1, 2, 4   # include/nnest_hip.h NNEST_CHAIN_STATS_*
HOST_FINISHED, HOST_RETRAIN, HOST_NEED_SAMPLES, HOST_LOG, HOST_CHECKPOINT, HOST_DEAD_FULL = range(6)   # include/nnest_hip.h NNEST_HOST_*
HOST_EXPIRED = 6
HOST_TOP, HOST_AFTER_TRAIN, HOST_AFTER_SAMPLES, HOST_AFTER_LOG = range(4)


def merge_importance(parts):
    """the sums (a, S1, S2, n_live) of the union of sample sets from the sums of each (include/nnest_hip.h
    nnest_importance_evidence): a = max a_i, S1 = sum S1_i e^(a_i - a), S2 = sum S2_i e^(2 (a_i - a)); float64"""
    parts = [tuple(float(v) for v in p) for p in parts]
    a = max([p[0] for p in parts], default=-math.inf)
    s1 = s2 = n = 0.0
    for ai, s1i, s2i, ni in parts:
        if ai == -math.inf:   # (nothing live in this part: its sums are 0)
            continue
        e = math.exp(ai - a)
        s1 += s1i * e
        s2 += s2i * e * e
        n += ni
    return a, s1, s2, n


def importance_result(a, S1, S2, n_live, M):
    """the estimate from the sums of M samples: logz_x = a + log S1 - log M (log Z over x), ess = S1^2 / S2,
    logzerr = sqrt((M / ess - 1) / (M - 1)) (the delta-method standard error of log Z: the relative standard error of the mean
    weight), max_weight_share = 1 / S1 (the largest weight's share of the total).  Everything dead: logz_x = -inf, ess = 0,
    logzerr = inf"""
    M = int(M)
    if not (M > 0 and n_live > 0 and S1 > 0.0 and a > -math.inf):
        return dict(logz_x=-math.inf, ess=0.0, logzerr=math.inf, max_weight_share=math.nan, n_live=int(n_live), n_samples=M)
    ess = S1 * S1 / S2
    err = math.sqrt(max(M / ess - 1.0, 0.0) / (M - 1)) if M > 1 else math.inf
    return dict(logz_x=a + math.log(S1) - math.log(M), ess=ess, logzerr=err, max_weight_share=1.0 / S1, n_live=int(n_live), n_samples=M)


def _merge_shifted(m1, s1, m2, s2, powers=(1,)):
    """max-shifted sums of two sets: m = max(m1, m2), each s[k] = s1[k] e^(powers[k] (m1 - m)) + s2[k] e^(powers[k] (m2 - m));
    -inf beside -inf has the factor 1, on sums of 0"""
    m = np.maximum(m1, m2)
    with np.errstate(invalid='ignore'):
        e1 = np.where(m1 == m, 1.0, np.exp(m1 - m))
        e2 = np.where(m2 == m, 1.0, np.exp(m2 - m))
    return m, [a * e1 ** p + b * e2 ** p for a, b, p in zip(s1, s2, powers)]


def _merge_moments(n1, mean1, M21, n2, mean2, M22):
    """Chan, Golub & LeVeque's rule for (count, mean, M2) of the union of two sets; an empty side leaves the other as it is"""
    n = n1 + n2
    safe = np.where(n > 0, n, 1.0)
    d = mean2 - mean1
    mean = np.where(n1 == 0, mean2, np.where(n2 == 0, mean1, (n1 * mean1 + n2 * mean2) / safe))
    M2 = np.where(n1 == 0, M22, np.where(n2 == 0, M21, (M21 + M22) + d * d * (n1 * n2 / safe)))
    return n, np.where(n > 0, mean, 0.0), np.where(n > 0, M2, 0.0)


def empty_glm_pointwise(n, slots=8):
    """the statistics of no draws at all: [n, 8] rows {-inf, 0, -inf, 0, 0, 0, 0, 0}, or [n, 3] zeros (nnest_glm_predict)"""
    out = np.zeros((int(n), int(slots)), np.float64)
    if slots == 8:
        out[:, 0] = out[:, 2] = -np.inf
    return out


def merge_glm_pointwise(p, q):
    """the per-row statistics of the union of two sets of draws from the statistics of each (include/nnest_hip.h
    nnest_glm_pointwise: [n, 8] = {a, P, b, Q, Q2, cnt, mean, M2}; nnest_glm_predict: [n, 3] = {cnt, mean, M2}): the max-shifted
    sums rescaled to the common maximum, Chan's rule for (cnt, mean, M2).  float64 numpy; the result of a run cut into launches is
    the single launch's up to reordered float64 addition"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    if p.shape != q.shape or p.ndim != 2 or p.shape[1] not in (3, 8):
        raise ValueError('merge_glm_pointwise: two arrays shaped [n, 8] or [n, 3], got %s and %s' % (p.shape, q.shape))
    out = np.empty_like(p)
    k = p.shape[1] - 3
    if k:
        out[:, 0], (out[:, 1],) = _merge_shifted(p[:, 0], [p[:, 1]], q[:, 0], [q[:, 1]])
        out[:, 2], (out[:, 3], out[:, 4]) = _merge_shifted(p[:, 2], [p[:, 3], p[:, 4]], q[:, 2], [q[:, 3], q[:, 4]], powers=(1, 2))
    out[:, k], out[:, k + 1], out[:, k + 2] = _merge_moments(p[:, k], p[:, k + 1], p[:, k + 2], q[:, k], q[:, k + 1], q[:, k + 2])
    return out


class HostState(ctypes.Structure):   # nnest_host_state_t
    _fields_ = [('logz', _d), ('logvol', _d), ('fraction_remain', _d), ('max_logl', _d), ('loglstar', _d),
                ('it', ctypes.c_longlong), ('n_dead', ctypes.c_longlong),
                ('accept_point', _i), ('nb', _i), ('first_time', _i), ('resume', _i), ('worst', _i), ('pad_', _i)]


class HostPrior(ctypes.Structure):   # nnest_host_prior_t
    _fields_ = [('pos', ctypes.c_longlong), ('k', ctypes.c_longlong), ('hits', ctypes.c_longlong), ('n', ctypes.c_longlong),
                ('n_cand', ctypes.c_longlong), ('pending_calls', ctypes.c_longlong), ('total_calls', ctypes.c_longlong),
                ('block_next', ctypes.c_longlong), ('ncs', _d * 20), ('mean_calls', _d), ('ncs_len', _i), ('expired', _i)]


_lib = None


def load():
    """Load libnnest_hip.so (built by __graft_entry__.build() / make -C nnest_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NnestHipError('%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                                '(hipcc --offload-arch=gfx950).  There is no CPU fallback.' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.argtypes = argtypes
            fn.restype = (ctypes.c_char_p if name == 'nnest_hip_last_error' else ctypes.c_long if name in ('nnest_format_rows_e5', 'nnest_format_scalar_rows')
                          else ctypes.c_double if name == 'nnest_host_h_update'
                          else ctypes.c_longlong if name == 'nnest_glm_psis_work_bytes' else ctypes.c_int)
        _lib = lib
    return _lib


def check(rc):
    if rc != NNEST_OK:
        msg = load().nnest_hip_last_error()
        err = NnestHipError('libnnest_hip error %d: %s' % (rc, msg.decode() if msg else '?'))
        err.code = rc
        raise err


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_info():
    n = ctypes.c_int(0)
    clk = ctypes.c_int(0)
    buf = ctypes.create_string_buffer(256)
    check(load().nnest_hip_device_info(ctypes.byref(n), ctypes.byref(clk), buf, 256))
    return {'num_cu': n.value, 'clock_khz': clk.value, 'name': buf.value.decode()}
