// nnest_abi.hip -- the extern "C" surface of libnnest_hip.so (include/nnest_hip.h): handle management,
// argument checks, error reporting.  No torch types, no exceptions across the boundary.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdarg.h>

#include "nnest_internal.h"
#include "mh_common.h"
#include "ensemble_common.h"
#include "mcmc_walk.h"
#include "importance_walk.h"
#include "mcmc_mixed.h"
#include "mcmc_adapt.h"
#include "mcmc_gdata.h"
#include "glm_data.h"
#include "glm_pointwise.h"
#include "glm_psis.h"
#include "gauss_prior.h"
#include "importance_glm.h"
#include "glm_newton.h"
#include "slice_glm.h"
#include <limits.h>
#include "mh_glm.h"

using namespace nnest;

struct nnest_nvp {
    FlowShape s;
    int device;
    int num_cu;
    int num_params;
    float *w;        // packed weights (state_dict order)
    float *adam_m;   // exp_avg
    float *adam_v;   // exp_avg_sq
    float *best_w;   // best-validation snapshot (Trainer.train's deepcopy, trainer.py:194, :208)
    float *img;      // MFMA fragment image of w
    int *adam_step;  // device int: torch.optim.Adam state['step']
    float *train_ws; // training workspace
    int *fwd_pos;    // packed parameter -> element of the forward fragment image (-1: absent)
    int *bwd_pos;    // packed parameter -> element of the backward fragment image
    size_t train_ws_floats;
    float *img_bwd;  // MAF: the transposed fragment image (the RealNVP training kernels keep theirs in the workspace / LDS)
    int *gpos;       // MAF: packed parameter -> slot of a tile's weight-gradient buffer
    unsigned int *ticket; // MAF: block counter of the fused update kernel (nnest_maf_train_epoch)
};

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace nnest {
void set_last_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }
}  // namespace nnest

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) return fail(NNEST_E_HIP, "%s: %s", #expr, hipGetErrorString(e__));       \
    } while (0)

// the fragment image(s) of the handle's flow from its packed weights
static hipError_t refresh_images(nnest_nvp *h, hipStream_t st) {
    if (h->s.kind == FLOW_KIND_MAF) return launch_maf_repack(h->w, h->img, h->img_bwd, h->s, st);
    if (h->s.scale_mode != NNEST_SCALE_AFFINE) {
        hipError_t e = launch_zero_scale_nets(h->w, h->s, st);  // unused slots stay 0
        if (e != hipSuccess) return e;
    }
    return launch_repack(h->w, h->img, h->s, st);
}

extern "C" {

int nnest_hip_version(void) { return NNEST_HIP_ABI_VERSION; }

const char *nnest_hip_last_error(void) { return g_err; }

int nnest_hip_device_info(int *num_cu, int *clock_khz, char *name, int name_len) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, dev));
    if (num_cu) *num_cu = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    if (name && name_len > 0) {
        snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    }
    return NNEST_OK;
}

int nnest_nvp_create(int D, int H, int B, int L, nnest_nvp_t **out) {
    return nnest_nvp_create_scaled(D, H, B, L, NNEST_SCALE_AFFINE, out);
}

int nnest_nvp_create_scaled(int D, int H, int B, int L, int scale_mode, nnest_nvp_t **out) {
    if (!out) return fail(NNEST_E_ARG, "out is NULL");
    *out = nullptr;
    if (D < 1 || H < 1 || B < 1 || L < 0) return fail(NNEST_E_ARG, "bad shape D=%d H=%d B=%d L=%d", D, H, B, L);
    if (scale_mode < NNEST_SCALE_AFFINE || scale_mode > NNEST_SCALE_CONSTANT)
        return fail(NNEST_E_ARG, "scale_mode=%d (0 '', 1 'translate', 2 'constant')", scale_mode);
    if (scale_mode == NNEST_SCALE_CONSTANT && B > 8)
        return fail(NNEST_E_UNSUPPORTED, "scale='constant' with num_blocks=%d > 8", B);
    if (H % 16 != 0)
        return fail(NNEST_E_UNSUPPORTED, "hidden_dim=%d: the gfx950 kernels tile the hidden layer by 16 (MFMA 16x16x4)", H);
    FlowShape s;
    s.D = D; s.H = H; s.B = B; s.L = L;
    s.NT = ((D + 1) / 2 + 15) / 16;
    s.NH = H / 16;
    s.net_floats = frag_net_floats(s.NT, s.NH, L);
    s.image_floats = B * 2 * s.net_floats;
    s.net_params = H * D + H + L * (H * H + H) + D * H + D;
    s.scale_mode = scale_mode;
    s.kind = FLOW_KIND_NVP;
    s.G = 0;
    s.base_beta = 0.f;
    s.base_const = -0.91893853320467274f;  // -log(2 pi) / 2
    if (!shape_supported(s))
        return fail(NNEST_E_UNSUPPORTED, "x_dim=%d hidden_dim=%d not instantiated (x_dim<=128 at H=16, <=64 at H=32, <=32 at H=64)", D, H);
    nnest_nvp *h = new nnest_nvp();
    memset(h, 0, sizeof(*h));
    h->s = s;
    h->num_params = s.num_params();
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail(NNEST_E_HIP, "hipGetDevice failed (no GPU?)"); }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, h->device) != hipSuccess) { delete h; return fail(NNEST_E_HIP, "hipGetDeviceProperties failed"); }
    h->num_cu = p.multiProcessorCount;
    size_t nb = (size_t)h->num_params * sizeof(float);
    h->train_ws_floats = train_workspace_floats(s, 128);
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&h->w, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->adam_m, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->adam_v, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->best_w, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->img, (size_t)s.image_alloc_floats() * sizeof(float));   // (+ the solo lane image behind it)
    if (e == hipSuccess) e = hipMalloc((void **)&h->adam_step, sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&h->train_ws, h->train_ws_floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&h->fwd_pos, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->bwd_pos, nb);
    if (e == hipSuccess) e = launch_build_pos(h->fwd_pos, h->bwd_pos, s, 0);
    if (e == hipSuccess) e = solo_prepare_device(h->device, 0);   // the step rule's table of this device, once per process
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e == hipSuccess) e = hipMemset(h->w, 0, nb);
    if (e == hipSuccess) e = hipMemset(h->adam_m, 0, nb);
    if (e == hipSuccess) e = hipMemset(h->adam_v, 0, nb);
    if (e == hipSuccess) e = hipMemset(h->adam_step, 0, sizeof(int));
    if (e == hipSuccess) e = hipMemset(h->img, 0, (size_t)s.image_alloc_floats() * sizeof(float));
    // (zero weights: both images, all zeros, are those of the weights from the first moment on)
    if (e != hipSuccess) {
        nnest_nvp_destroy(h);
        return fail(NNEST_E_HIP, "device allocation failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return NNEST_OK;
}

int nnest_maf_create(int D, int H, int B, int L, nnest_nvp_t **out) {
    if (!out) return fail(NNEST_E_ARG, "out is NULL");
    *out = nullptr;
    if (D < 2 || H < 1 || B < 1 || L < 0) return fail(NNEST_E_ARG, "bad shape D=%d H=%d B=%d L=%d (a MAF needs x_dim >= 2)", D, H, B, L);
    if (H != 16) return fail(NNEST_E_UNSUPPORTED, "maf: hidden_dim=%d, the kernels are instantiated for 16", H);
    FlowShape s;
    s.D = D; s.H = H; s.B = B; s.L = L;
    s.NT = ((D + 1) / 2 + 15) / 16;
    s.NH = H / 16;
    s.net_floats = frag_net_floats(2 * s.NT, s.NH, L);                 // fragments over both parity classes: 2 NT tiles
    s.image_floats = B * 2 * s.net_floats + B * 16 * 2 * s.NT;         // + the group of every slot, per block
    s.net_params = H * D + H + L * (H * H + H) + D * H + D;
    s.scale_mode = NNEST_SCALE_AFFINE;
    s.kind = FLOW_KIND_MAF;
    s.G = maf_num_groups(D, H);
    s.base_beta = 0.f;
    s.base_const = -0.91893853320467274f;
    if (s.NT > 4 || !maf_shape_supported(s))
        return fail(NNEST_E_UNSUPPORTED, "maf: x_dim=%d num_blocks=%d num_layers=%d: the fragment image (%d floats) has to fit one CU's LDS and x_dim <= 128", D, B, L, s.image_floats);
    nnest_nvp *h = new nnest_nvp();
    memset(h, 0, sizeof(*h));
    h->s = s;
    h->num_params = s.num_params();
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail(NNEST_E_HIP, "hipGetDevice failed (no GPU?)"); }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, h->device) != hipSuccess) { delete h; return fail(NNEST_E_HIP, "hipGetDeviceProperties failed"); }
    h->num_cu = p.multiProcessorCount;
    const size_t nb = (size_t)h->num_params * sizeof(float), ib = (size_t)s.image_floats * sizeof(float);
    h->train_ws_floats = maf_workspace_floats(s);
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&h->w, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->adam_m, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->adam_v, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->best_w, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->img, ib);
    if (e == hipSuccess) e = hipMalloc((void **)&h->img_bwd, ib);
    if (e == hipSuccess) e = hipMalloc((void **)&h->adam_step, sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&h->train_ws, h->train_ws_floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&h->gpos, nb);
    if (e == hipSuccess) e = launch_maf_build_gpos(h->gpos, s, 0);
    if (e == hipSuccess) e = hipMalloc((void **)&h->fwd_pos, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->bwd_pos, nb);
    if (e == hipSuccess) e = launch_maf_build_pos(h->fwd_pos, h->bwd_pos, s, 0);
    if (e == hipSuccess) e = hipMalloc((void **)&h->ticket, sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(h->ticket, 0, sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(h->w, 0, nb);
    if (e == hipSuccess) e = hipMemset(h->adam_m, 0, nb);
    if (e == hipSuccess) e = hipMemset(h->adam_v, 0, nb);
    if (e == hipSuccess) e = hipMemset(h->adam_step, 0, sizeof(int));
    if (e == hipSuccess) e = refresh_images(h, 0);
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) {
        nnest_nvp_destroy(h);
        return fail(NNEST_E_HIP, "device allocation failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return NNEST_OK;
}

int nnest_maf_num_groups(const nnest_nvp_t *h) { return (h && h->s.kind == FLOW_KIND_MAF) ? h->s.G : -1; }

int nnest_nvp_destroy(nnest_nvp_t *h) {
    if (!h) return NNEST_OK;
    (void)hipFree(h->w); (void)hipFree(h->adam_m); (void)hipFree(h->adam_v); (void)hipFree(h->best_w); (void)hipFree(h->img);
    (void)hipFree(h->adam_step); (void)hipFree(h->train_ws); (void)hipFree(h->fwd_pos); (void)hipFree(h->bwd_pos);
    (void)hipFree(h->img_bwd); (void)hipFree(h->gpos); (void)hipFree(h->ticket);
    delete h;
    return NNEST_OK;
}

int nnest_nvp_num_params(const nnest_nvp_t *h) { return h ? h->num_params : -1; }

int nnest_nvp_set_base(nnest_nvp_t *h, float beta) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (!(beta >= 0.f)) return fail(NNEST_E_ARG, "beta=%g: 0 selects N(0, I), beta > 0 GeneralisedNormal(0, 1, beta)", (double)beta);
    h->s.base_beta = beta;
    h->s.base_const = beta == 0.f ? -0.91893853320467274f : (float)(log((double)beta) - log(2.0) - lgamma(1.0 / (double)beta));
    return NNEST_OK;
}

int nnest_nvp_load_weights(nnest_nvp_t *h, const float *packed_host, void *stream) {
    if (!h || !packed_host) return fail(NNEST_E_ARG, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->w, packed_host, (size_t)h->num_params * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(refresh_images(h, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NNEST_OK;
}

int nnest_nvp_store_weights(nnest_nvp_t *h, float *packed_host, void *stream) {
    if (!h || !packed_host) return fail(NNEST_E_ARG, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(packed_host, h->w, (size_t)h->num_params * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NNEST_OK;
}

int nnest_nvp_device_ptrs(nnest_nvp_t *h, float **w_dev, float **m_dev, float **v_dev) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (w_dev) *w_dev = h->w;
    if (m_dev) *m_dev = h->adam_m;
    if (v_dev) *v_dev = h->adam_v;
    return NNEST_OK;
}

int nnest_nvp_store_adam(nnest_nvp_t *h, float *exp_avg_host, float *exp_avg_sq_host, void *stream) {
    if (!h || !exp_avg_host || !exp_avg_sq_host) return fail(NNEST_E_ARG, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    size_t nb = (size_t)h->num_params * sizeof(float);
    HIP_TRY(hipMemcpyAsync(exp_avg_host, h->adam_m, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(exp_avg_sq_host, h->adam_v, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NNEST_OK;
}

int nnest_nvp_load_adam(nnest_nvp_t *h, const float *exp_avg_host, const float *exp_avg_sq_host, void *stream) {
    if (!h || !exp_avg_host || !exp_avg_sq_host) return fail(NNEST_E_ARG, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    size_t nb = (size_t)h->num_params * sizeof(float);
    HIP_TRY(hipMemcpyAsync(h->adam_m, exp_avg_host, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->adam_v, exp_avg_sq_host, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NNEST_OK;
}

int nnest_nvp_adam_state(nnest_nvp_t *h, int *step_count, int set_step, int reset_moments, void *stream) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    hipStream_t st = (hipStream_t)stream;
    if (reset_moments) {
        HIP_TRY(hipMemsetAsync(h->adam_m, 0, (size_t)h->num_params * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(h->adam_v, 0, (size_t)h->num_params * sizeof(float), st));
    }
    if (set_step >= 0) HIP_TRY(hipMemcpyAsync(h->adam_step, &set_step, sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (step_count) {
        HIP_TRY(hipMemcpyAsync(step_count, h->adam_step, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return NNEST_OK;
}

static int check_rows(const nnest_nvp_t *h, const void *a, const void *b, int N) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (N < 0) return fail(NNEST_E_ARG, "N=%d < 0", N);
    if (N > 0 && (!a || !b)) return fail(NNEST_E_ARG, "NULL device buffer");
    return NNEST_OK;
}

int nnest_nvp_forward(nnest_nvp_t *h, const float *x_dev, float *z_dev, float *logdet_dev, int N, void *stream) {
    int rc = check_rows(h, x_dev, z_dev, N);
    if (rc) return rc;
    HIP_TRY(launch_pass(h->img, h->s, PASS_FORWARD, x_dev, z_dev, logdet_dev, nullptr, nullptr, N, LikeSpec(), h->num_cu,
                        (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_nvp_inverse(nnest_nvp_t *h, const float *z_dev, float *x_dev, float *logdet_dev, int N, void *stream) {
    int rc = check_rows(h, z_dev, x_dev, N);
    if (rc) return rc;
    HIP_TRY(launch_pass(h->img, h->s, PASS_INVERSE, z_dev, x_dev, logdet_dev, nullptr, nullptr, N, LikeSpec(), h->num_cu,
                        (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_nvp_log_probs(nnest_nvp_t *h, const float *x_dev, float *logp_dev, int N, void *stream) {
    int rc = check_rows(h, x_dev, logp_dev, N);
    if (rc) return rc;
    HIP_TRY(launch_pass(h->img, h->s, PASS_LOGPROB, x_dev, logp_dev, nullptr, nullptr, nullptr, N, LikeSpec(), h->num_cu,
                        (hipStream_t)stream));
    return NNEST_OK;
}

static int check_like(const nnest_like_t *like, int D, LikeSpec *out) {
    if (!like) return fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    if (like->id == NNEST_LIKE_EGGBOX && D != 2) return fail(NNEST_E_ARG, "Eggbox is defined for x_dim = 2 (likelihoods.py:97-102)");
    if (like->id == NNEST_LIKE_GAUSSMIX && D < 2) return fail(NNEST_E_ARG, "GaussianMix needs x_dim >= 2");
    out->id = like->id;
    out->scale = like->scale;
    for (int i = 0; i < 6; ++i) out->p[i] = like->params[i];
    return NNEST_OK;
}

int nnest_nvp_inverse_loglike(nnest_nvp_t *h, const nnest_like_t *like, const float *z_dev, float *x_dev,
                              float *logdet_dev, double *logl_dev, int *inbox_dev, int N, void *stream) {
    int rc = check_rows(h, z_dev, logl_dev, N);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = check_like(like, h->s.D, &lk))) return rc;
    HIP_TRY(launch_pass(h->img, h->s, PASS_INVERSE_LOGLIKE, z_dev, x_dev, logdet_dev, logl_dev, inbox_dev, N, lk,
                        h->num_cu, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_loglike(const nnest_like_t *like, const float *x_unit_dev, double *logl_dev, int N, int D, void *stream) {
    if (N < 0 || D < 1) return fail(NNEST_E_ARG, "bad N=%d D=%d", N, D);
    LikeSpec lk;
    int rc = check_like(like, D, &lk);
    if (rc) return rc;
    if (D > 128) return fail(NNEST_E_UNSUPPORTED, "x_dim=%d > 128", D);
    if (N > 0 && (!x_unit_dev || !logl_dev)) return fail(NNEST_E_ARG, "NULL device buffer");
    int dev = 0, num_cu = 256;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_TRY(launch_loglike(lk, x_unit_dev, logl_dev, N, D, num_cu, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_mh_constrained_steps(nnest_nvp_t *h, const nnest_like_t *like, float *z_dev, float *x_dev,
                               double *logl_dev, double loglstar, float step_size, int steps, int C, int flags,
                               const float *noise_dz_dev, const float *noise_u_dev, uint64_t seed,
                               uint64_t walker_offset, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev,
                               int *n_call_dev, float *scale_out_dev, void *sync_dev, void *stream) {
    int rc = check_rows(h, z_dev, logl_dev, C);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = check_like(like, h->s.D, &lk))) return rc;
    if (steps < 0) return fail(NNEST_E_ARG, "steps=%d < 0", steps);
    if ((noise_dz_dev == nullptr) != (noise_u_dev == nullptr))
        return fail(NNEST_E_ARG, "noise_dz_dev and noise_u_dev must both be given or both be NULL");
    if ((flags & NNEST_MH_DYNAMIC_BATCH) && !sync_dev) return fail(NNEST_E_ARG, "NNEST_MH_DYNAMIC_BATCH needs sync_dev");
    hipError_t e = launch_mh(h->img, h->s, lk, z_dev, x_dev, logl_dev, loglstar, step_size, steps, C, flags,
                             noise_dz_dev, noise_u_dev, seed, walker_offset, hist_x_dev, hist_logl_dev, n_accept_dev, n_call_dev,
                             scale_out_dev, h->w, (unsigned long long *)sync_dev, h->num_cu, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration)
        return fail(NNEST_E_UNSUPPORTED, "no kernel form for C=%d walkers with flags 0x%x (pinned form not applicable to this "
                                         "shape / population, or the batch-wide step rule on a grid that may not be resident)", C, flags);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mh: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_slice_steps(nnest_nvp_t *h, const nnest_like_t *like, float *z_dev, float *x_dev, double *logl_dev, double loglstar,
                      float width, int steps, int C, int max_stepout, int max_shrink, const float *noise_dz_dev, uint64_t seed,
                      uint64_t walker_offset, float *hist_x_dev, int *n_call_dev, int *n_move_dev, int *n_eval_dev, void *stream) {
    int rc = check_rows(h, z_dev, logl_dev, C);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = check_like(like, h->s.D, &lk))) return rc;
    if (!slice_params_ok(steps, max_stepout, max_shrink, width))
        return fail(NNEST_E_ARG, "steps=%d max_stepout=%d (0..2^24) max_shrink=%d (1..60) width=%g", steps, max_stepout, max_shrink, (double)width);
    if (!slice_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "slice proposal: hidden 16, 3 blocks, 1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128");
    const SliceArgs a = {z_dev, x_dev, logl_dev, loglstar, width, steps, C, max_stepout, max_shrink, lk, seed, walker_offset, noise_dz_dev,
                         hist_x_dev, nullptr, n_call_dev, n_move_dev, n_eval_dev};
    hipError_t e = launch_slice_solo(h->s, h->img + h->s.solo_image_offset(), a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_slice_solo: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_slice_fill_noise(float *dz_dev, int steps, int C, int D, uint64_t seed, uint64_t walker_offset, void *stream) {
    if (!dz_dev || steps < 0 || C < 0 || D < 1) return fail(NNEST_E_ARG, "bad argument");
    HIP_TRY(launch_slice_fill_noise(dz_dev, steps, C, D, seed, walker_offset, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_ensemble_work_words(int C, int steps) {
    if (C < 0 || steps < 0) return -1;
    const size_t w = ensemble_work_words(C, steps);
    return w > (size_t)0x7fffffff ? -1 : (int)w;
}

}  // extern "C"
int nnest::mcmc_args(McmcArgs *a, const float *t_std, const float *t_mean, const float *lo, const float *hi, const float *z_in,
                     const double *lp_in, const double *logl_in, float *z_out, float *x_out, double *lp_out, double *logl_out,
                     float *hist_z, float *hist_x, double *hist_logl, int *n_accept, int C, int steps, float step_size, uint64_t step0,
                     uint64_t seed, uint64_t walker_offset) {
    if (C < 1 || steps < 0) return fail(NNEST_E_ARG, "mcmc: C=%d (>= 1 walkers) steps=%d (>= 0)", C, steps);
    if (!isfinite(step_size) || step_size < 0.f) return fail(NNEST_E_ARG, "mcmc: step_size=%g (finite, >= 0)", (double)step_size);
    if (!z_in || !x_out || !lp_out || !logl_out || (steps > 0 && !z_out)) return fail(NNEST_E_ARG, "NULL device buffer");
    if (!t_std != !t_mean) return fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (!lo != !hi) return fail(NNEST_E_ARG, "lo_dev and hi_dev: both or neither");
    if (!lp_in != !logl_in) return fail(NNEST_E_ARG, "lp_in_dev and logl_in_dev: both or neither");
    if ((!hist_z != !hist_x) || (!hist_z != !hist_logl)) return fail(NNEST_E_ARG, "hist_z_dev, hist_x_dev and hist_logl_dev: all or none");
    a->t_std = t_std; a->t_mean = t_mean; a->lo = lo; a->hi = hi;
    a->z_in = z_in; a->lp_in = lp_in; a->logl_in = logl_in;
    a->z_out = z_out; a->x_out = x_out; a->lp_out = lp_out; a->logl_out = logl_out;
    a->hist_z = hist_z; a->hist_x = hist_x; a->hist_logl = hist_logl; a->n_accept = n_accept;
    a->C = C; a->S = steps; a->step = step_size; a->step0 = (uint32_t)step0; a->seed = seed; a->walker_offset = walker_offset;
    return NNEST_OK;
}
int nnest::mcmc_beta_ok(double beta) {
    if (!isfinite(beta) || beta < 0.0) return fail(NNEST_E_ARG, "mcmc: beta=%g (the likelihood's power: finite, >= 0)", beta);
    return NNEST_OK;
}
int nnest::mcmc_mixed_every_ok(int global_every) {
    if (global_every < 0)
        return fail(NNEST_E_ARG, "mcmc mixed: global_every=%d (every how many steps a global step is taken: >= 0, 0: never)", global_every);
    return NNEST_OK;
}
int nnest::mcmc_adapt_rule_ok(double adapt_rate, double target_accept) {
    if (!isfinite(adapt_rate) || adapt_rate < 0.0 || adapt_rate > 1.0)
        return fail(NNEST_E_ARG, "mcmc adapt: adapt_rate=%g (the gain of the step-size rule: finite, in [0, 1])", adapt_rate);
    if (!(target_accept > 0.0 && target_accept < 1.0))
        return fail(NNEST_E_ARG, "mcmc adapt: target_accept=%g (the acceptance the rule aims at: strictly inside (0, 1))", target_accept);
    return NNEST_OK;
}
// D: what the descriptor's dimension must be (the flow's x_dim, or the D argument of nnest_loglike_gdata)
int nnest::gdata_ok(const nnest_gdata_t *g, int D, GdataSpec *out) {
    if (!g) return fail(NNEST_E_ARG, "gdata is NULL");
    if (!g->mu_dev || !g->r_dev) return fail(NNEST_E_ARG, "gdata: NULL mu_dev or r_dev");
    if (g->D < 1 || g->D > 128) return fail(NNEST_E_ARG, "gdata: D=%d (1 .. 128)", g->D);
    if (g->D != D) return fail(NNEST_E_ARG, "gdata: the likelihood's D=%d is not D=%d", g->D, D);
    if (!isfinite(g->logl0)) return fail(NNEST_E_ARG, "gdata: logl0=%g (finite)", g->logl0);
    out->mu = g->mu_dev; out->r = g->r_dev; out->logl0 = g->logl0; out->D = g->D;
    return NNEST_OK;
}
// D: what the descriptor's dimension must be (the flow's x_dim, or the D argument of nnest_loglike_glm)
int nnest::glm_ok(const nnest_glm_t *g, int D, GlmSpec *out) {
    if (!g) return fail(NNEST_E_ARG, "glm is NULL");
    if (!g->at_dev || !g->y_dev || !g->o_dev) return fail(NNEST_E_ARG, "glm: NULL at_dev, y_dev or o_dev");
    if (g->D < 1 || g->D > 128) return fail(NNEST_E_ARG, "glm: D=%d (1 .. 128)", g->D);
    if (g->D != D) return fail(NNEST_E_ARG, "glm: the likelihood's D=%d is not D=%d", g->D, D);
    if (g->n < 1 || g->n > GLM_MAX_ROWS) return fail(NNEST_E_ARG, "glm: n=%d (1 .. %d rows)", g->n, GLM_MAX_ROWS);
    if (g->ld < g->n || g->ld > GLM_MAX_ROWS || g->ld % 64 != 0)
        return fail(NNEST_E_ARG, "glm: ld=%d (a multiple of 64, n=%d .. %d)", g->ld, g->n, GLM_MAX_ROWS);
    if (g->family != NNEST_GLM_LOGISTIC && g->family != NNEST_GLM_POISSON)
        return fail(NNEST_E_ARG, "glm: family=%d (NNEST_GLM_LOGISTIC = 0, NNEST_GLM_POISSON = 1)", g->family);
    if (!isfinite(g->logl0)) return fail(NNEST_E_ARG, "glm: logl0=%g (finite)", g->logl0);
    out->at = g->at_dev; out->y = g->y_dev; out->o = g->o_dev; out->logl0 = g->logl0;
    out->n = g->n; out->ld = g->ld; out->D = g->D; out->family = g->family;
    return NNEST_OK;
}
// D: what the descriptor's dimension must be (the flow's x_dim, or the D argument of nnest_logprior_gauss)
int nnest::gauss_prior_ok(const nnest_gauss_prior_t *g, int D, GaussPriorSpec *out, const char *what) {
    if (!g) return fail(NNEST_E_ARG, "prior is NULL");
    if (!g->m_dev || !g->r_dev) return fail(NNEST_E_ARG, "prior: NULL m_dev or r_dev");
    if (g->D < 1 || g->D > 128) return fail(NNEST_E_ARG, "prior: D=%d (1 .. 128)", g->D);
    if (g->D != D) return fail(NNEST_E_ARG, "the prior's D=%d is not %s=%d", g->D, what, D);
    if (!isfinite(g->logc)) return fail(NNEST_E_ARG, "prior: logc=%g (finite)", g->logc);
    out->m = g->m_dev; out->r = g->r_dev; out->logc = g->logc; out->D = g->D;
    return NNEST_OK;
}
int nnest::importance_args(ImpArgs *a, const float *t_std, const float *t_mean, const float *lo, const float *hi, float *z_out, float *x_out,
                           double *logl_out, double *logw_out, double *partials, double *sums, int M, uint64_t seed, uint64_t sample_offset) {
    if (M < 0 || M > (1 << 30)) return fail(NNEST_E_ARG, "importance: M=%d (0 .. 2^30 samples a launch)", M);
    if (!sums || (M > 0 && !partials)) return fail(NNEST_E_ARG, "importance: NULL sums_dev or partials_dev");
    if (!t_std != !t_mean) return fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (!lo != !hi) return fail(NNEST_E_ARG, "lo_dev and hi_dev: both or neither");
    if ((!z_out != !x_out) || (!z_out != !logl_out) || (!z_out != !logw_out))
        return fail(NNEST_E_ARG, "z_out_dev, x_out_dev, logl_out_dev and logw_out_dev: all or none");
    a->t_std = t_std; a->t_mean = t_mean; a->lo = lo; a->hi = hi;
    a->z_out = z_out; a->x_out = x_out; a->logl_out = logl_out; a->logw_out = logw_out;
    a->partials = partials; a->sums = sums; a->M = M; a->seed = seed; a->sample_offset = sample_offset;
    return NNEST_OK;
}
int nnest::ensemble_sizes(int C, int steps) {
    if (C < 2 || C > (1 << 16) || steps < 0) return fail(NNEST_E_ARG, "ensemble: C=%d (2..65536 walkers) steps=%d", C, steps);
    if (nnest_ensemble_work_words(C, steps) < 0) return fail(NNEST_E_ARG, "ensemble: C=%d x steps=%d: the work buffer exceeds 2^31 words", C, steps);
    return NNEST_OK;
}
// the moves of a run from the caller's weights (NULL: the stretch move alone): the step threshold thr = floor(p_stretch 2^24), float64,
// and the DE scale with emcee's defaults for 0.  A DE step needs two distinct partners in either set: C >= 4
static int ens_resolve_moves(const nnest_ens_moves_t *m, int C, int D, EnsMoves *out) {
    out->thr = ENS_THR_ALWAYS;
    out->g0 = out->sigma = 0.f;
    if (!m) return NNEST_OK;
    const double ws = (double)m->w_stretch, wd = (double)m->w_de;
    if (!(isfinite(ws) && isfinite(wd)) || ws < 0.0 || wd < 0.0 || ws + wd <= 0.0)
        return fail(NNEST_E_ARG, "ensemble moves: weights stretch=%g de=%g (finite, >= 0, not both 0)", ws, wd);
    if (!(isfinite(m->de_gamma0) && isfinite(m->de_sigma)) || m->de_gamma0 < 0.f || m->de_sigma < 0.f)
        return fail(NNEST_E_ARG, "ensemble moves: de_gamma0=%g de_sigma=%g (finite, >= 0; 0: emcee's default)", (double)m->de_gamma0, (double)m->de_sigma);
    if (wd > 0.0 && C < 4) return fail(NNEST_E_ARG, "ensemble moves: C=%d walkers: the DE move needs two partners in either set (C >= 4)", C);
    if (D < 1) return fail(NNEST_E_ARG, "ensemble moves: D=%d", D);
    out->thr = (uint32_t)floor(ws / (ws + wd) * 16777216.0);
    out->g0 = m->de_gamma0 != 0.f ? m->de_gamma0 : (float)(2.38 / sqrt(2.0 * (double)D));
    out->sigma = m->de_sigma != 0.f ? m->de_sigma : 1e-5f;
    return NNEST_OK;
}

extern "C" {

int nnest_ensemble_moves_threshold(const nnest_ens_moves_t *moves) {
    EnsMoves mv;
    if (ens_resolve_moves(moves, 4, 1, &mv)) return -1;
    return (int)mv.thr;
}

int nnest_ensemble_fill_moves(const int *work_dev, int *move_dev, int *b_dev, float *gamma_dev, int C, int D, int steps, uint64_t step0,
                              uint64_t seed, const nnest_ens_moves_t *moves, void *stream) {
    int rc = ensemble_sizes(C, steps);
    if (rc) return rc;
    if (!work_dev) return fail(NNEST_E_ARG, "NULL work_dev");
    if (C < 4) return fail(NNEST_E_ARG, "ensemble moves: C=%d walkers: the DE move needs two partners in either set (C >= 4)", C);
    EnsMoves mv;
    const nnest_ens_moves_t dflt = {1.f, 0.f, 0.f, 0.f};   // (no weights: every step a stretch step, the DE draws at emcee's default scale)
    if ((rc = ens_resolve_moves(moves ? moves : &dflt, C, D, &mv))) return rc;
    HIP_TRY(launch_ensemble_fill_moves(work_dev, move_dev, b_dev, gamma_dev, C, steps, (uint32_t)step0, seed, mv, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_ensemble_fill_noise(int *work_dev, float *u_dev, int C, int steps, uint64_t step0, uint64_t seed, void *stream) {
    int rc = ensemble_sizes(C, steps);
    if (rc) return rc;
    if (!work_dev) return fail(NNEST_E_ARG, "NULL work_dev");
    HIP_TRY(launch_ensemble_split(work_dev, u_dev, C, steps, (uint32_t)step0, seed, (hipStream_t)stream));
    return NNEST_OK;
}

// (the checks that need no handle come first: they answer on a machine without a GPU, where no handle can exist)
// beta NULL: nnest_mcmc_steps; else nnest_mcmc_tempered_steps at *beta
static int mcmc_steps_entry(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                            const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                            float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                            double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                            uint64_t walker_offset, const double *beta, void *stream) {
    if (!like) return fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    int rc;
    if (beta && (rc = mcmc_beta_ok(*beta))) return rc;
    McmcTemperedArgs a;
    memset(&a, 0, sizeof(a));
    a.beta = beta ? *beta : 1.0;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if ((rc = check_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "mcmc: hidden 16, 3 blocks, 1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128");
    hipError_t e = beta ? launch_mcmc_tempered(h->s, h->w, a, (hipStream_t)stream) : launch_mcmc(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mcmc: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mcmc: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_mcmc_steps(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                     const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                     float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                     double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                     uint64_t walker_offset, void *stream) {
    return mcmc_steps_entry(h, like, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                            logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed,
                            walker_offset, nullptr, stream);
}

int nnest_mcmc_tempered_steps(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                              const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev,
                              float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev,
                              float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size,
                              uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, void *stream) {
    return mcmc_steps_entry(h, like, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                            logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed,
                            walker_offset, &beta, stream);
}

int nnest_mcmc_fill_noise(float *dz_dev, float *u_dev, int steps, int C, int D, uint64_t step0, uint64_t seed, uint64_t walker_offset,
                          void *stream) {
    if (steps < 0 || C < 0 || D < 1) return fail(NNEST_E_ARG, "mcmc_fill_noise: steps=%d C=%d D=%d", steps, C, D);
    HIP_TRY(launch_mcmc_fill_noise(dz_dev, u_dev, steps, C, D, (uint32_t)step0, seed, walker_offset, (hipStream_t)stream));
    return NNEST_OK;
}

// what nnest_mcmc_mixed_steps takes, asked before a launch (and by the entry itself): the refusals name their reason -- the base's
// in the words of nnest_importance_check
int nnest_mcmc_mixed_check(nnest_nvp_t *h, int like_id) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return fail(NNEST_E_UNSUPPORTED, "mcmc mixed: unknown likelihood id %d", like_id);
    if (h->s.base_beta != 0.f)
        return fail(NNEST_E_UNSUPPORTED, "mcmc mixed: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only", (double)h->s.base_beta);
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "mcmc mixed: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (h->s.NT < 1 || h->s.NT > 4) return fail(NNEST_E_UNSUPPORTED, "mcmc mixed: x_dim=%d not instantiated", h->s.D);
    return NNEST_OK;
}

// (as nnest_mcmc_steps: the checks that need no handle come first)
int nnest_mcmc_mixed_steps(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, void *stream) {
    if (!like) return fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    int rc;
    if ((rc = mcmc_beta_ok(beta))) return rc;
    if ((rc = mcmc_mixed_every_ok(global_every))) return rc;
    McmcMixedArgs a;
    memset(&a, 0, sizeof(a));
    a.beta = beta;
    a.global_every = global_every;
    a.n_accept_global = n_accept_global_dev;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if ((rc = nnest_mcmc_mixed_check(h, like->id))) return rc;
    if ((rc = check_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    hipError_t e = launch_mcmc_mixed(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mcmc mixed: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mcmc_mixed: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_mcmc_adapt_steps takes, asked before a launch (and by the entry itself): as nnest_mcmc_mixed_check answers
int nnest_mcmc_adapt_check(nnest_nvp_t *h, int like_id) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return fail(NNEST_E_UNSUPPORTED, "mcmc adapt: unknown likelihood id %d", like_id);
    if (h->s.base_beta != 0.f)
        return fail(NNEST_E_UNSUPPORTED, "mcmc adapt: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only", (double)h->s.base_beta);
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "mcmc adapt: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (h->s.NT < 1 || h->s.NT > 4) return fail(NNEST_E_UNSUPPORTED, "mcmc adapt: x_dim=%d not instantiated", h->s.D);
    return NNEST_OK;
}

// (as nnest_mcmc_mixed_steps: the checks that need no handle come first)
int nnest_mcmc_adapt_steps(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, const double *step_in_dev,
                           double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept,
                           void *stream) {
    if (!like) return fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    int rc;
    if ((rc = mcmc_beta_ok(beta))) return rc;
    if ((rc = mcmc_mixed_every_ok(global_every))) return rc;
    if ((rc = mcmc_adapt_rule_ok(adapt_rate, target_accept))) return rc;
    McmcAdaptArgs a;
    memset(&a, 0, sizeof(a));
    a.beta = beta;
    a.global_every = global_every;
    a.n_accept_global = n_accept_global_dev;
    a.step_in = step_in_dev;
    a.step_out = step_out_dev;
    a.hist_step = hist_step_dev;
    a.adapt_steps = adapt_steps;
    a.adapt_rate = adapt_rate;
    a.target_accept = target_accept;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if ((rc = nnest_mcmc_adapt_check(h, like->id))) return rc;
    if ((rc = check_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    hipError_t e = launch_mcmc_adapt(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mcmc adapt: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mcmc_adapt: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// the Gaussian likelihood from user data (nnest_mcmc_gdata.hip): the likelihood alone
int nnest_loglike_gdata(const nnest_gdata_t *gdata, const float *t_dev, double *logl_dev, int N, int D, void *stream) {
    GdataSpec gd;
    int rc;
    if ((rc = gdata_ok(gdata, D, &gd))) return rc;
    if (N < 0) return fail(NNEST_E_ARG, "loglike gdata: N=%d (>= 0)", N);
    if (N > 0 && (!t_dev || !logl_dev)) return fail(NNEST_E_ARG, "NULL device buffer");
    hipError_t e = launch_loglike_gdata(gd, t_dev, logl_dev, N, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_loglike_gdata: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_mcmc_gdata_steps takes, asked before a launch (and by the entry itself): the shapes and the base of
// nnest_mcmc_adapt_check, and a descriptor of the flow's x_dim
int nnest_mcmc_gdata_check(nnest_nvp_t *h, int D) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (h->s.base_beta != 0.f)
        return fail(NNEST_E_UNSUPPORTED, "mcmc gdata: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only", (double)h->s.base_beta);
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "mcmc gdata: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (h->s.NT < 1 || h->s.NT > 4) return fail(NNEST_E_UNSUPPORTED, "mcmc gdata: x_dim=%d not instantiated", h->s.D);
    if (D != h->s.D) return fail(NNEST_E_ARG, "mcmc gdata: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// (as nnest_mcmc_adapt_steps: the checks that need no handle come first)
int nnest_mcmc_gdata_steps(nnest_nvp_t *h, const nnest_gdata_t *gdata, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, const double *step_in_dev,
                           double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept,
                           void *stream) {
    McmcGdataArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = gdata_ok(gdata, gdata ? gdata->D : 0, &a.gd))) return rc;
    if ((rc = mcmc_beta_ok(beta))) return rc;
    if ((rc = mcmc_mixed_every_ok(global_every))) return rc;
    if ((rc = mcmc_adapt_rule_ok(adapt_rate, target_accept))) return rc;
    a.beta = beta;
    a.global_every = global_every;
    a.n_accept_global = n_accept_global_dev;
    a.step_in = step_in_dev;
    a.step_out = step_out_dev;
    a.hist_step = hist_step_dev;
    a.adapt_steps = adapt_steps;
    a.adapt_rate = adapt_rate;
    a.target_accept = target_accept;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if ((rc = nnest_mcmc_gdata_check(h, a.gd.D))) return rc;
    a.like.scale = 1.0f;
    hipError_t e = launch_mcmc_gdata(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mcmc gdata: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mcmc_gdata: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// the regression likelihoods of the user's data (nnest_mcmc_glm.hip, glm_data.h): the likelihood alone
int nnest_loglike_glm(const nnest_glm_t *glm, const float *t_dev, double *logl_dev, int N, int D, void *stream) {
    GlmSpec gl;
    int rc;
    if ((rc = glm_ok(glm, D, &gl))) return rc;
    if (N < 0) return fail(NNEST_E_ARG, "loglike glm: N=%d (>= 0)", N);
    if (N > 0 && (!t_dev || !logl_dev)) return fail(NNEST_E_ARG, "NULL device buffer");
    hipError_t e = launch_loglike_glm(gl, t_dev, logl_dev, N, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_loglike_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// the pointwise predictive statistics of these likelihoods over a set of draws (nnest_glm_pointwise.hip, glm_pointwise.h)
int nnest_glm_pointwise_groups(int S, int n) {
    if (S < 0 || S > GLMPW_MAX_DRAWS || n < 1 || n > GLM_MAX_ROWS) return -1;
    return glm_pointwise_groups(S, n);
}

static int glm_pointwise_entry(const char *what, int predict, const nnest_glm_t *glm, const float *t_dev, double *stats_dev,
                               double *partials_dev, int S, int D, void *stream) {
    GlmSpec gl;
    int rc;
    if ((rc = glm_ok(glm, D, &gl))) return rc;
    if (S < 0 || S > GLMPW_MAX_DRAWS) return fail(NNEST_E_ARG, "%s: S=%d (0 .. %d draws)", what, S, GLMPW_MAX_DRAWS);
    if (!t_dev || !stats_dev || !partials_dev)
        return fail(NNEST_E_ARG, "%s: NULL t_dev=%p, stats_dev=%p or partials_dev=%p", what, (const void *)t_dev, (void *)stats_dev, (void *)partials_dev);
    hipError_t e = launch_glm_pointwise(gl, t_dev, stats_dev, partials_dev, S, predict, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_glm_pointwise: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_glm_pointwise(const nnest_glm_t *glm, const float *t_dev, double *stats_dev, double *partials_dev, int S, int D, void *stream) {
    return glm_pointwise_entry("glm pointwise", 0, glm, t_dev, stats_dev, partials_dev, S, D, stream);
}

int nnest_glm_predict(const nnest_glm_t *glm, const float *t_dev, double *stats_dev, double *partials_dev, int S, int D, void *stream) {
    return glm_pointwise_entry("glm predict", 1, glm, t_dev, stats_dev, partials_dev, S, D, stream);
}

// their matrix of terms and Pareto-smoothed leave-one-out (nnest_glm_psis.hip, glm_psis.h)
int nnest_glm_terms(const nnest_glm_t *glm, const float *t_dev, double *out_dev, int S, int D, void *stream) {
    GlmSpec gl;
    int rc;
    if ((rc = glm_ok(glm, D, &gl))) return rc;
    if (S < 0 || S > GLMPW_MAX_DRAWS || (long long)S * gl.n > GLMPSIS_MAX_TERMS)
        return fail(NNEST_E_ARG, "glm terms: S=%d, n=%d (S >= 0, S n <= %lld)", S, gl.n, GLMPSIS_MAX_TERMS);
    if (!t_dev || !out_dev) return fail(NNEST_E_ARG, "glm terms: NULL t_dev=%p or out_dev=%p", (const void *)t_dev, (void *)out_dev);
    hipError_t e = launch_glm_terms(gl, t_dev, out_dev, S, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_glm_terms: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_glm_psis_tail_cap(int S) {
    if (S < 0 || S > GLMPSIS_MAX_DRAWS) return -1;
    return glm_psis_tail_cap(S);
}

long long nnest_glm_psis_work_bytes(int S, int n) {
    if (S < 0 || S > GLMPSIS_MAX_DRAWS || n < 1 || n > GLM_MAX_ROWS) return -1;
    const long long bytes = glm_psis_work(S, n).bytes;
    return bytes > GLMPSIS_MAX_WORK ? -1 : bytes;
}

int nnest_glm_psis(const nnest_glm_t *glm, const float *t_dev, const double *stats_dev, double *out_dev, void *work_dev, int S, int D,
                   void *stream) {
    GlmSpec gl;
    int rc;
    if ((rc = glm_ok(glm, D, &gl))) return rc;
    if (S < 0 || S > GLMPSIS_MAX_DRAWS) return fail(NNEST_E_ARG, "glm psis: S=%d (0 .. %d draws in one call: thin a longer run)", S, GLMPSIS_MAX_DRAWS);
    if (nnest_glm_psis_work_bytes(S, gl.n) < 0)
        return fail(NNEST_E_ARG, "glm psis: S=%d, n=%d need more than %lld bytes of work (thin the draws)", S, gl.n, GLMPSIS_MAX_WORK);
    if (!t_dev || !stats_dev || !out_dev || !work_dev)
        return fail(NNEST_E_ARG, "glm psis: NULL t_dev=%p, stats_dev=%p, out_dev=%p or work_dev=%p", (const void *)t_dev, (const void *)stats_dev,
                    (void *)out_dev, work_dev);
    hipError_t e = launch_glm_psis(gl, t_dev, stats_dev, out_dev, work_dev, S, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_glm_psis: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_mcmc_glm_steps takes, asked before a launch (and by the entry itself): the shapes and the base of
// nnest_mcmc_adapt_check, and a descriptor of the flow's x_dim
int nnest_mcmc_glm_check(nnest_nvp_t *h, int D) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (h->s.base_beta != 0.f)
        return fail(NNEST_E_UNSUPPORTED, "mcmc glm: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only", (double)h->s.base_beta);
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "mcmc glm: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (h->s.NT < 1 || h->s.NT > 4) return fail(NNEST_E_UNSUPPORTED, "mcmc glm: x_dim=%d not instantiated", h->s.D);
    if (D != h->s.D) return fail(NNEST_E_ARG, "mcmc glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// (as nnest_mcmc_adapt_steps: the checks that need no handle come first)
int nnest_mcmc_glm_steps(nnest_nvp_t *h, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, const double *step_in_dev,
                           double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept,
                           void *stream) {
    McmcGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if ((rc = mcmc_beta_ok(beta))) return rc;
    if ((rc = mcmc_mixed_every_ok(global_every))) return rc;
    if ((rc = mcmc_adapt_rule_ok(adapt_rate, target_accept))) return rc;
    a.beta = beta;
    a.global_every = global_every;
    a.n_accept_global = n_accept_global_dev;
    a.step_in = step_in_dev;
    a.step_out = step_out_dev;
    a.hist_step = hist_step_dev;
    a.adapt_steps = adapt_steps;
    a.adapt_rate = adapt_rate;
    a.target_accept = target_accept;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if ((rc = nnest_mcmc_glm_check(h, a.gl.D))) return rc;
    a.like.scale = 1.0f;
    hipError_t e = launch_mcmc_glm(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mcmc glm: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mcmc_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_slice_glm_steps takes, asked before a launch (and by the entry itself): the shapes of nnest_slice_steps, and a
// descriptor of the flow's x_dim
int nnest_slice_glm_check(nnest_nvp_t *h, int D) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (!slice_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "slice glm: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (D != h->s.D) return fail(NNEST_E_ARG, "slice glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// the slice proposal on the regression likelihoods of the user's data (nnest_slice_glm.hip); the argument checks of nnest_slice_steps
// and glm_ok (those that need no handle come first)
int nnest_slice_glm_steps(nnest_nvp_t *h, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, float *z_dev,
                          float *x_dev, double *logl_dev, double loglstar, float width, int steps, int C, int max_stepout, int max_shrink,
                          const float *noise_dz_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev, int *n_call_dev,
                          int *n_move_dev, int *n_eval_dev, void *stream) {
    SliceGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if (!t_std_dev != !t_mean_dev) return fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (!slice_params_ok(steps, max_stepout, max_shrink, width))
        return fail(NNEST_E_ARG, "steps=%d max_stepout=%d (0..2^24) max_shrink=%d (1..60) width=%g", steps, max_stepout, max_shrink, (double)width);
    if ((rc = check_rows(h, z_dev, logl_dev, C))) return rc;
    if ((rc = nnest_slice_glm_check(h, a.gl.D))) return rc;
    a.z = z_dev; a.x = x_dev; a.logl = logl_dev; a.loglstar = loglstar; a.width = width; a.steps = steps; a.C = C;
    a.max_out = max_stepout; a.max_shrink = max_shrink; a.like.scale = 1.0f; a.seed = seed; a.walker_offset = walker_offset;
    a.noise_dz = noise_dz_dev; a.hist_x = hist_x_dev; a.n_call = n_call_dev; a.n_move = n_move_dev; a.n_eval = n_eval_dev;
    a.t_std = t_std_dev; a.t_mean = t_mean_dev;
    hipError_t e = launch_slice_glm(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "slice glm: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_slice_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_mh_glm_steps takes, asked before a launch (and by the entry itself): the flags' three settings less the per-tile rule, the
// shapes of nnest_slice_steps, a descriptor of the flow's x_dim, and -- under the batch rule -- a grid that is proven resident
int nnest_mh_glm_check(nnest_nvp_t *h, int D, int C, int flags) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (!mh_glm_flags_ok(flags, false))
        return fail(NNEST_E_ARG, "mh glm: flags 0x%x: 0 (fixed step) or NNEST_MH_DYNAMIC_BATCH | NNEST_MH_LAG(0..15); the unconstrained walk is "
                    "nnest_mcmc_glm_steps, one walker per wave has no per-tile rule, and there are no forms, warm-up steps or sync halves", flags);
    if (!slice_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "mh glm: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (D != h->s.D) return fail(NNEST_E_ARG, "mh glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    if (C < 0) return fail(NNEST_E_ARG, "mh glm: C=%d < 0", C);
    if (flags & NNEST_MH_DYNAMIC_BATCH) {   // (the smaller of the two families' grids: the verdict holds for either)
        int cap = INT_MAX;
        for (int fam : {GLM_LOGISTIC, GLM_POISSON}) {
            MhGlmArgs probe;
            memset(&probe, 0, sizeof(probe));
            probe.gl.family = fam;
            int c = 0;
            hipError_t e = launch_mh_glm(h->s, h->w, probe, h->num_cu, &c, nullptr);
            if (e != hipSuccess) return fail(NNEST_E_HIP, "mh glm: occupancy query: %s", hipGetErrorString(e));
            cap = c < cap ? c : cap;
        }
        if ((C + 3) / 4 > cap)
            return fail(NNEST_E_UNSUPPORTED, "mh glm: the batch-wide step rule needs every workgroup resident: C=%d walkers are %d workgroups, "
                        "%d fit this device", C, (C + 3) / 4, cap);
    }
    return NNEST_OK;
}

// the constrained Metropolis proposal on the regression likelihoods of the user's data (nnest_mh_glm.hip); the argument checks of
// nnest_mh_constrained_steps and glm_ok (those that need no handle come first)
int nnest_mh_glm_steps(nnest_nvp_t *h, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, float *z_dev, float *x_dev,
                       double *logl_dev, double loglstar, float step_size, int steps, int C, int flags, const float *noise_dz_dev,
                       const float *noise_u_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev, double *hist_logl_dev,
                       int *n_accept_dev, int *n_call_dev, float *scale_out_dev, void *sync_dev, void *stream) {
    MhGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if (!t_std_dev != !t_mean_dev) return fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (steps < 0) return fail(NNEST_E_ARG, "steps=%d < 0", steps);
    if ((noise_dz_dev == nullptr) != (noise_u_dev == nullptr))
        return fail(NNEST_E_ARG, "noise_dz_dev and noise_u_dev must both be given or both be NULL");
    if ((rc = check_rows(h, z_dev, logl_dev, C))) return rc;
    if ((rc = nnest_mh_glm_check(h, a.gl.D, C, flags))) return rc;
    if ((flags & NNEST_MH_DYNAMIC_BATCH) && !sync_dev) return fail(NNEST_E_ARG, "NNEST_MH_DYNAMIC_BATCH needs sync_dev");
    a.z = z_dev; a.x = x_dev; a.logl = logl_dev; a.loglstar = loglstar; a.step_size = step_size; a.steps = steps; a.C = C; a.flags = flags;
    a.like.scale = 1.0f; a.noise_dz = noise_dz_dev; a.noise_u = noise_u_dev; a.seed = seed; a.walker_offset = walker_offset;
    a.hist_x = hist_x_dev; a.hist_logl = hist_logl_dev; a.n_accept = n_accept_dev; a.n_call = n_call_dev; a.scale_out = scale_out_dev;
    a.sync = (flags & NNEST_MH_DYNAMIC_BATCH) ? (unsigned long long *)sync_dev : nullptr;
    a.sync_err = a.sync ? reinterpret_cast<int *>(a.sync + mh_sync_words(steps)) : nullptr;   // the word behind the counters
    a.t_std = t_std_dev; a.t_mean = t_mean_dev;
    hipError_t e = launch_mh_glm(h->s, h->w, a, h->num_cu, nullptr, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mh glm: x_dim=%d not instantiated", h->s.D);
    if (e == hipErrorLaunchOutOfResources)
        return fail(NNEST_E_UNSUPPORTED, "mh glm: the batch-wide step rule needs every workgroup resident: C=%d walkers do not fit this device", C);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mh_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// the normal priors beside the regression likelihoods (nnest_mcmc_glm_prior.hip, gauss_prior.h): the prior alone
int nnest_logprior_gauss(const nnest_gauss_prior_t *prior, const float *t_dev, double *logp_dev, int N, int D, void *stream) {
    GaussPriorSpec p;
    int rc;
    if ((rc = gauss_prior_ok(prior, D, &p, "D"))) return rc;
    if (N < 0) return fail(NNEST_E_ARG, "logprior gauss: N=%d (>= 0)", N);
    if (N > 0 && (!t_dev || !logp_dev)) return fail(NNEST_E_ARG, "NULL device buffer");
    hipError_t e = launch_logprior_gauss(p, t_dev, logp_dev, N, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_logprior_gauss: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// the gradient and curvature of the regression likelihoods at one theta, and the Newton step under the normal priors
// (nnest_glm_newton.hip, glm_newton.h)
int nnest_glm_curv_groups(int n, int D) {
    if (n < 1 || n > GLM_MAX_ROWS || D < 1 || D > 128) return -1;
    return glm_curv_groups(n, D);
}

int nnest_glm_curv(const nnest_glm_t *glm, const double *theta_dev, double *out_dev, double *partials_dev, int D, void *stream) {
    GlmSpec gl;
    int rc;
    if ((rc = glm_ok(glm, D, &gl))) return rc;
    if (!theta_dev || !out_dev || !partials_dev)
        return fail(NNEST_E_ARG, "glm curv: NULL theta_dev=%p, out_dev=%p or partials_dev=%p", (const void *)theta_dev, (void *)out_dev,
                    (void *)partials_dev);
    hipError_t e = launch_glm_curv(gl, theta_dev, out_dev, partials_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_glm_curv: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_glm_newton_solve(const double *curv_dev, const nnest_gauss_prior_t *prior, const double *theta_dev, double *step_dev,
                           double *chol_dev, double *info_dev, int D, void *stream) {
    if (D < 1 || D > 128) return fail(NNEST_E_ARG, "glm newton solve: D=%d (1 .. 128)", D);
    GaussPriorSpec p;
    int rc;
    if (prior && (rc = gauss_prior_ok(prior, D, &p, "D"))) return rc;
    if (!curv_dev || !theta_dev || !step_dev || !chol_dev || !info_dev)
        return fail(NNEST_E_ARG, "glm newton solve: NULL curv_dev=%p, theta_dev=%p, step_dev=%p, chol_dev=%p or info_dev=%p", (const void *)curv_dev,
                    (const void *)theta_dev, (void *)step_dev, (void *)chol_dev, (void *)info_dev);
    hipError_t e = launch_glm_newton_solve(curv_dev, prior ? &p : nullptr, theta_dev, step_dev, chol_dev, info_dev, D, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_glm_newton_solve: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_mcmc_glm_prior_steps takes, asked before a launch (and by the entry itself): nnest_mcmc_glm_check's verdict -- the
// kernel is that kernel's with a prior term, so the same shapes and base
int nnest_mcmc_glm_prior_check(nnest_nvp_t *h, int D) { return nnest_mcmc_glm_check(h, D); }

// (as nnest_mcmc_glm_steps: the checks that need no handle come first)
int nnest_mcmc_glm_prior_steps(nnest_nvp_t *h, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior, const float *t_std_dev,
                               const float *t_mean_dev, const float *lo_dev, const float *hi_dev, const float *z_in_dev,
                               const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev,
                               double *logl_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C,
                               int steps, float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta,
                               int global_every, int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev,
                               double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream) {
    McmcGlmPriorArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if ((rc = gauss_prior_ok(prior, h ? h->s.D : prior ? prior->D : 0, &a.pr))) return rc;   // (no handle: refused below)
    if ((rc = mcmc_beta_ok(beta))) return rc;
    if ((rc = mcmc_mixed_every_ok(global_every))) return rc;
    if ((rc = mcmc_adapt_rule_ok(adapt_rate, target_accept))) return rc;
    a.beta = beta;
    a.global_every = global_every;
    a.n_accept_global = n_accept_global_dev;
    a.step_in = step_in_dev;
    a.step_out = step_out_dev;
    a.hist_step = hist_step_dev;
    a.adapt_steps = adapt_steps;
    a.adapt_rate = adapt_rate;
    a.target_accept = target_accept;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if ((rc = nnest_mcmc_glm_prior_check(h, a.gl.D))) return rc;
    a.like.scale = 1.0f;
    hipError_t e = launch_mcmc_glm_prior(h->s, h->w, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(NNEST_E_UNSUPPORTED, "mcmc glm prior: x_dim=%d not instantiated", h->s.D);
    if (e != hipSuccess) return fail(NNEST_E_HIP, "launch_mcmc_glm_prior: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_importance_evidence takes, asked before a launch (and by the entry itself): the refusals name their reason
int nnest_importance_check(nnest_nvp_t *h, int like_id) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return fail(NNEST_E_UNSUPPORTED, "importance: unknown likelihood id %d", like_id);
    if (h->s.base_beta != 0.f)
        return fail(NNEST_E_UNSUPPORTED, "importance: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only", (double)h->s.base_beta);
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "importance: x_dim=%d hidden=%d blocks=%d layers=%d scale mode %d: the kernel takes hidden 16, 3 blocks, "
                    "1 layer, scale '' (the one-sample-per-wave layout), x_dim <= 128", h->s.D, h->s.H, h->s.B, h->s.L, h->s.scale_mode);
    if (h->s.NT < 1 || h->s.NT > 4) return fail(NNEST_E_UNSUPPORTED, "importance: x_dim=%d not instantiated", h->s.D);
    return NNEST_OK;
}

// (as nnest_mcmc_steps: the checks that need no handle come first)
int nnest_importance_evidence(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                              const float *hi_dev, float *z_out_dev, float *x_out_dev, double *logl_out_dev, double *logw_out_dev,
                              double *partials_dev, double *sums_dev, int M, uint64_t seed, uint64_t sample_offset, void *stream) {
    if (!like) return fail(NNEST_E_ARG, "like is NULL");
    ImpArgs a;
    memset(&a, 0, sizeof(a));
    int rc = importance_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_out_dev, x_out_dev, logl_out_dev, logw_out_dev, partials_dev,
                             sums_dev, M, seed, sample_offset);
    if (rc) return rc;
    if ((rc = nnest_importance_check(h, like->id))) return rc;
    if ((rc = check_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    a.groups = importance_groups(M, IMP_NVP_TILE, h->num_cu);
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_importance_begin(sums_dev, st));
    HIP_TRY(launch_importance(h->s, h->w, a, st));
    HIP_TRY(launch_importance_combine(partials_dev, sums_dev, a.groups, st));
    return NNEST_OK;
}

// what nnest_importance_glm_evidence takes, asked before a launch (and by the entry itself): nnest_importance_check's verdict on the
// shape and the base -- the kernel is that kernel's on another target --, and a descriptor of the flow's x_dim
int nnest_importance_glm_check(nnest_nvp_t *h, int D) {
    int rc;
    if ((rc = nnest_importance_check(h, NNEST_LIKE_GAUSSIAN))) return rc;
    if (D != h->s.D) return fail(NNEST_E_ARG, "importance glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// (as nnest_importance_evidence: the checks that need no handle come first)
int nnest_importance_glm_evidence(nnest_nvp_t *h, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior, const float *t_std_dev,
                                  const float *t_mean_dev, const float *lo_dev, const float *hi_dev, float *z_out_dev, float *x_out_dev,
                                  double *logl_out_dev, double *logw_out_dev, double *partials_dev, double *sums_dev, int M, uint64_t seed,
                                  uint64_t sample_offset, void *stream) {
    ImpGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc = importance_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_out_dev, x_out_dev, logl_out_dev, logw_out_dev, partials_dev,
                             sums_dev, M, seed, sample_offset);
    if (rc) return rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if (prior) {
        if ((rc = gauss_prior_ok(prior, h ? h->s.D : prior->D, &a.pr))) return rc;   // (no handle: refused below)
        if (lo_dev) return fail(NNEST_E_ARG, "importance glm: a prior together with the box lo_dev / hi_dev (one or the other)");
        a.prior = 1;
    }
    if ((rc = nnest_importance_glm_check(h, a.gl.D))) return rc;
    a.like.scale = 1.0f;
    a.groups = importance_groups(M, IMP_NVP_TILE, h->num_cu);
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_importance_begin(sums_dev, st));
    HIP_TRY(launch_importance_glm(h->s, h->w, a, st));
    HIP_TRY(launch_importance_combine(partials_dev, sums_dev, a.groups, st));
    return NNEST_OK;
}

int nnest_importance_groups(int M, int tile) {
    if (M < 0 || (tile != IMP_NVP_TILE && tile != IMP_SPLINE_TILE)) return -1;
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return -1;
    return importance_groups(M, tile, p.multiProcessorCount);
}

int nnest_importance_fill_noise(float *z_dev, int M, int D, uint64_t seed, uint64_t sample_offset, void *stream) {
    if (M < 0 || D < 1 || (M > 0 && !z_dev)) return fail(NNEST_E_ARG, "importance_fill_noise: M=%d D=%d z_dev=%p", M, D, (void *)z_dev);
    HIP_TRY(launch_importance_fill_noise(z_dev, M, D, seed, sample_offset, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_ensemble_moves_max_walkers(nnest_nvp_t *h, int like_id, const nnest_ens_moves_t *moves) {
    if (!h || !ensemble_form_eligible(h->s)) return -1;
    EnsMoves mv;
    if (ens_resolve_moves(moves, 4, h->s.D, &mv)) return -1;
    int n = 0;
    if (ensemble_max_walkers(h->s, like_id, mv, h->num_cu, &n) != hipSuccess) return -1;
    return n;
}

int nnest_ensemble_max_walkers(nnest_nvp_t *h, int like_id) { return nnest_ensemble_moves_max_walkers(h, like_id, nullptr); }

int nnest_ensemble_moves_steps(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                               const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, float *z_out_dev,
                               float *x_out_dev, double *lp_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_lp_dev,
                               int *n_accept_dev, int *work_dev, int C, int steps, uint64_t step0, uint64_t seed, int constrained,
                               double loglstar, void *stream, const nnest_ens_moves_t *moves) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    int rc = ensemble_sizes(C, steps);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = check_like(like, h->s.D, &lk))) return rc;
    lk.scale = 1.0f;
    EnsMoves mv;
    if ((rc = ens_resolve_moves(moves, C, h->s.D, &mv))) return rc;
    if (!t_std_dev || !t_mean_dev || !z_in_dev || !z_out_dev || !x_out_dev || !lp_out_dev || !work_dev ||
        (steps > 0 && (!hist_z_dev || !hist_x_dev || !hist_lp_dev)))
        return fail(NNEST_E_ARG, "NULL device buffer");
    if (!lo_dev != !hi_dev) return fail(NNEST_E_ARG, "lo_dev and hi_dev: both or neither");
    if ((const void *)z_in_dev == (const void *)z_out_dev) return fail(NNEST_E_ARG, "z_in_dev must not be z_out_dev (partners read it during the launch)");
    if (!ensemble_form_eligible(h->s))
        return fail(NNEST_E_UNSUPPORTED, "ensemble: hidden 16, 3 blocks, 1 layer, scale '' (the one-walker-per-wave layout), x_dim <= 128");
    char msg[400];
    msg[0] = 0;
    rc = launch_ensemble(h->s, h->w, lk, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                         hist_z_dev, hist_x_dev, hist_lp_dev, n_accept_dev, work_dev, C, steps, (uint32_t)step0, seed, constrained ? 1 : 0,
                         loglstar, mv, h->num_cu, (hipStream_t)stream, msg, sizeof(msg));
    if (rc) return fail(rc, "%s", msg);
    return NNEST_OK;
}

int nnest_ensemble_steps(nnest_nvp_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                         const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, float *z_out_dev, float *x_out_dev,
                         double *lp_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *work_dev,
                         int C, int steps, uint64_t step0, uint64_t seed, int constrained, double loglstar, void *stream) {
    return nnest_ensemble_moves_steps(h, like, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                                      hist_z_dev, hist_x_dev, hist_lp_dev, n_accept_dev, work_dev, C, steps, step0, seed, constrained,
                                      loglstar, stream, nullptr);
}

static int ensemble_x_like(int D, int like_id) {
    if (D < 1) return fail(NNEST_E_ARG, "ensemble_x: x_dim=%d", D);
    if (D > 128) return fail(NNEST_E_UNSUPPORTED, "ensemble_x: x_dim=%d > 128 (the one-walker-per-wave layout)", D);
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return fail(NNEST_E_ARG, "unknown likelihood id %d", like_id);
    return NNEST_OK;
}

static int current_num_cu(int *num_cu) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    return NNEST_OK;
}

int nnest_ensemble_x_moves_max_walkers(int D, int like_id, const nnest_ens_moves_t *moves) {
    int n = 0, num_cu = 0;
    EnsMoves mv;
    if (ensemble_x_like(D, like_id) || ens_resolve_moves(moves, 4, D, &mv) || current_num_cu(&num_cu)) return -1;
    if (ensemble_x_max_walkers(D, like_id, mv, num_cu, &n) != hipSuccess) return -1;
    return n;
}

int nnest_ensemble_x_max_walkers(int D, int like_id) { return nnest_ensemble_x_moves_max_walkers(D, like_id, nullptr); }

int nnest_ensemble_x_moves_steps(const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                                 const float *hi_dev, const float *x_in_dev, const double *lp_in_dev, float *x_out_dev, float *tx_out_dev,
                                 double *lp_out_dev, float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *work_dev, int C, int D,
                                 int steps, uint64_t step0, uint64_t seed, int constrained, double loglstar, void *stream,
                                 const nnest_ens_moves_t *moves) {
    if (!like) return fail(NNEST_E_ARG, "like is NULL");
    int rc = ensemble_x_like(D, like->id);
    if (rc) return rc;
    if ((rc = ensemble_sizes(C, steps))) return rc;
    EnsMoves mv;
    if ((rc = ens_resolve_moves(moves, C, D, &mv))) return rc;
    LikeSpec lk;
    if ((rc = check_like(like, D, &lk))) return rc;
    lk.scale = 1.0f;
    if (!x_in_dev || !x_out_dev || !lp_out_dev || !work_dev || (steps > 0 && (!hist_x_dev || !hist_lp_dev)))
        return fail(NNEST_E_ARG, "NULL device buffer");
    if (!t_std_dev != !t_mean_dev) return fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (!lo_dev != !hi_dev) return fail(NNEST_E_ARG, "lo_dev and hi_dev: both or neither");
    if ((const void *)x_in_dev == (const void *)x_out_dev) return fail(NNEST_E_ARG, "x_in_dev must not be x_out_dev (partners read it during the launch)");
    int num_cu = 0;
    if ((rc = current_num_cu(&num_cu))) return rc;
    char msg[400];
    msg[0] = 0;
    rc = launch_ensemble_x(D, lk, t_std_dev, t_mean_dev, lo_dev, hi_dev, x_in_dev, lp_in_dev, x_out_dev, tx_out_dev, lp_out_dev, hist_x_dev,
                           hist_lp_dev, n_accept_dev, work_dev, C, steps, (uint32_t)step0, seed, constrained ? 1 : 0, loglstar, mv, num_cu,
                           (hipStream_t)stream, msg, sizeof(msg));
    if (rc) return fail(rc, "%s", msg);
    return NNEST_OK;
}

int nnest_ensemble_x_steps(const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                           const float *x_in_dev, const double *lp_in_dev, float *x_out_dev, float *tx_out_dev, double *lp_out_dev,
                           float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *work_dev, int C, int D, int steps, uint64_t step0,
                           uint64_t seed, int constrained, double loglstar, void *stream) {
    return nnest_ensemble_x_moves_steps(like, t_std_dev, t_mean_dev, lo_dev, hi_dev, x_in_dev, lp_in_dev, x_out_dev, tx_out_dev, lp_out_dev,
                                        hist_x_dev, hist_lp_dev, n_accept_dev, work_dev, C, D, steps, step0, seed, constrained, loglstar,
                                        stream, nullptr);
}

int nnest_ensemble_rounds_moves_propose(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                        const float *z_cur_dev, float *q_dev, void *stream, const nnest_ens_moves_t *moves) {
    int rc = ensemble_sizes(C, steps);
    if (rc) return rc;
    EnsMoves mv;
    if ((rc = ens_resolve_moves(moves, C, D, &mv))) return rc;
    if (!work_dev || !z_cur_dev || !q_dev) return fail(NNEST_E_ARG, "NULL device buffer");
    if (D < 1 || i < 0 || i >= steps || (half != 0 && half != 1)) return fail(NNEST_E_ARG, "D=%d i=%d (steps %d) half=%d", D, i, steps, half);
    const int rows = half ? C / 2 : (C + 1) / 2;
    HIP_TRY(launch_ensemble_propose(work_dev, C, steps, D, i, half, (uint32_t)step0, seed, mv, z_cur_dev, q_dev, rows, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_ensemble_rounds_propose(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                  const float *z_cur_dev, float *q_dev, void *stream) {
    return nnest_ensemble_rounds_moves_propose(work_dev, C, steps, D, i, half, step0, seed, z_cur_dev, q_dev, stream, nullptr);
}

int nnest_ensemble_rounds_moves_accept(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                       const float *q_dev, const float *x_dev, const float *ld_dev, const double *logl_dev,
                                       const double *lprior_dev, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                                       const float *hi_dev, float *z_cur_dev, float *x_cur_dev, double *lp_cur_dev, float *hist_z_dev,
                                       float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *acc_rows_dev, int constrained,
                                       double loglstar, void *stream, const nnest_ens_moves_t *moves) {
    int rc = ensemble_sizes(C, steps);
    if (rc) return rc;
    EnsMoves mv;
    if ((rc = ens_resolve_moves(moves, C, D, &mv))) return rc;
    if (D < 1 || half < -1 || half > 1 || (half >= 0 && (i < 0 || i >= steps))) return fail(NNEST_E_ARG, "D=%d i=%d (steps %d) half=%d", D, i, steps, half);
    if (!work_dev || !q_dev || !x_dev || !ld_dev || !logl_dev || !z_cur_dev || !x_cur_dev || !lp_cur_dev ||
        (half >= 0 && (!hist_z_dev || !hist_x_dev || !hist_lp_dev)))
        return fail(NNEST_E_ARG, "NULL device buffer");
    if (!lo_dev != !hi_dev) return fail(NNEST_E_ARG, "lo_dev and hi_dev: both or neither");
    if (lo_dev && !lprior_dev && (!t_std_dev || !t_mean_dev)) return fail(NNEST_E_ARG, "the box needs t_std_dev and t_mean_dev");
    const int rows = half < 0 ? C : half ? C / 2 : (C + 1) / 2;
    HIP_TRY(launch_ensemble_accept(work_dev, C, steps, D, half < 0 ? 0 : i, half, (uint32_t)step0, seed, mv, q_dev, x_dev, ld_dev, logl_dev,
                                   lprior_dev, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_cur_dev, x_cur_dev, lp_cur_dev, hist_z_dev,
                                   hist_x_dev, hist_lp_dev, n_accept_dev, acc_rows_dev, constrained ? 1 : 0, loglstar, rows,
                                   (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_ensemble_rounds_accept(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                 const float *q_dev, const float *x_dev, const float *ld_dev, const double *logl_dev,
                                 const double *lprior_dev, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                                 const float *hi_dev, float *z_cur_dev, float *x_cur_dev, double *lp_cur_dev, float *hist_z_dev,
                                 float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *acc_rows_dev, int constrained,
                                 double loglstar, void *stream) {
    return nnest_ensemble_rounds_moves_accept(work_dev, C, steps, D, i, half, step0, seed, q_dev, x_dev, ld_dev, logl_dev, lprior_dev,
                                              t_std_dev, t_mean_dev, lo_dev, hi_dev, z_cur_dev, x_cur_dev, lp_cur_dev, hist_z_dev,
                                              hist_x_dev, hist_lp_dev, n_accept_dev, acc_rows_dev, constrained, loglstar, stream, nullptr);
}

int nnest_mh_form_for(const nnest_nvp_t *h, int C, int flags) {
    if (!h || C < 1) return -1;
    return mh_form_for(h->s, C, flags, h->num_cu);
}

int nnest_mh_sync_words(int steps) { return steps < 0 ? -1 : (int)mh_sync_words(steps) + 1; }

int nnest_mh_num_groups(const nnest_nvp_t *h, int C) {
    (void)h;
    return mh_num_groups(C);
}

int nnest_mh_fill_noise(float *dz_dev, float *u_dev, int steps, int C, int D, uint64_t seed, uint64_t walker_offset,
                        void *stream) {
    if (!dz_dev) return fail(NNEST_E_ARG, "NULL dz_dev");
    HIP_TRY(launch_fill_noise(dz_dev, u_dev, steps, C, D, seed, walker_offset, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_nvp_train(nnest_nvp_t *h, const float *xtrain_dev, int n_train, const float *xvalid_dev, int n_valid,
                    const int *perm_dev, const float *noise_dev, uint64_t seed, float jitter, int batch,
                    int max_epochs, int patience, float lr, float weight_decay, int epoch_offset, int flags,
                    float *losses_dev, nnest_train_result_t *result_dev, void *stream) {
    if (!h) return fail(NNEST_E_ARG, "NULL handle");
    if (!xtrain_dev || !xvalid_dev || !perm_dev || !result_dev) return fail(NNEST_E_ARG, "NULL device buffer");
    if (n_train < 1 || n_valid < 1 || batch < 1 || max_epochs < 0)
        return fail(NNEST_E_ARG, "bad sizes n_train=%d n_valid=%d batch=%d max_epochs=%d", n_train, n_valid, batch, max_epochs);
    if (batch > 128) return fail(NNEST_E_UNSUPPORTED, "batch_size=%d > 128 (one workgroup holds a minibatch)", batch);
    if (h->s.kind == FLOW_KIND_MAF)
        return fail(NNEST_E_UNSUPPORTED, "maf: the epoch loop is driven from the host (nnest_nvp_loss_grad + nnest_nvp_adam_step per minibatch)");
    const int stage_rows = train_rows_per_launch(h->s);
    if (stage_rows <= 0)
        return fail(NNEST_E_UNSUPPORTED, "x_dim=%d hidden_dim=%d num_layers=%d: no training kernel is instantiated for this shape", h->s.D,
                    h->s.H, h->s.L);
    if ((batch < n_train ? batch : n_train) > stage_rows)
        return fail(NNEST_E_UNSUPPORTED, "hidden_dim=%d num_layers=%d: one workgroup stages at most %d rows of a minibatch, batch_size=%d "
                    "(drive the epoch loop from the host: nnest_nvp_loss_grad + nnest_nvp_adam_step per minibatch)", h->s.H, h->s.L,
                    stage_rows, batch);
    HIP_TRY(launch_train(h->w, h->adam_m, h->adam_v, h->best_w, h->img, h->adam_step, h->s, xtrain_dev, n_train, xvalid_dev,
                         n_valid, perm_dev, noise_dev, seed, jitter, batch, max_epochs, patience, lr, weight_decay,
                         epoch_offset, flags, losses_dev, result_dev, h->train_ws, h->fwd_pos, h->bwd_pos, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_nvp_train_form(const nnest_nvp_t *h, int batch, int flags, int *detail) {
    if (!h || batch < 1 || batch > 128 || h->s.kind == FLOW_KIND_MAF || batch > train_rows_per_launch(h->s)) return -1;
    return train_form_for(h->s, batch, flags, detail);
}

int nnest_nvp_loss_grad(nnest_nvp_t *h, const float *x_dev, int M, float *grad_dev, float *loss_dev, void *stream) {
    if (!h || !x_dev || !grad_dev || !loss_dev) return fail(NNEST_E_ARG, "NULL argument");
    if (M < 1 || M > 128) return fail(NNEST_E_UNSUPPORTED, "M=%d outside [1,128]", M);
    if (h->s.kind == FLOW_KIND_MAF) {
        if (h->s.L > 2) return fail(NNEST_E_UNSUPPORTED, "maf: num_layers=%d > 2 has no training kernel", h->s.L);
        HIP_TRY(launch_maf_loss_grad(h->s, h->img, h->img_bwd, h->gpos, x_dev, M, grad_dev, loss_dev, h->train_ws, (hipStream_t)stream));
        return NNEST_OK;
    }
    HIP_TRY(launch_loss_grad(h->w, h->s, x_dev, M, grad_dev, loss_dev, h->train_ws, h->img, h->fwd_pos, h->bwd_pos,
                             (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_nvp_vjp(nnest_nvp_t *h, const float *x_dev, const float *gz_dev, float gld, int M, float *grad_dev, float *gx_dev, void *stream) {
    if (!h || !x_dev || !gz_dev || !grad_dev || !gx_dev) return fail(NNEST_E_ARG, "NULL argument");
    if (M < 1 || M > 128) return fail(NNEST_E_UNSUPPORTED, "M=%d outside [1,128]", M);
    if (h->s.kind == FLOW_KIND_MAF) return fail(NNEST_E_UNSUPPORTED, "maf: no vector-Jacobian product (it is not a stage of a fast/slow hierarchy)");
    HIP_TRY(launch_vjp(h->w, h->s, x_dev, gz_dev, gld, M, grad_dev, gx_dev, h->train_ws, h->img, h->fwd_pos, h->bwd_pos, (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_nvp_adam_step(nnest_nvp_t *h, const float *grad_dev, float lr, float weight_decay, void *stream) {
    if (!h || !grad_dev) return fail(NNEST_E_ARG, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_adam_packed_dev(h->w, grad_dev, h->adam_m, h->adam_v, h->num_params, h->adam_step, lr, weight_decay, st));
    HIP_TRY(refresh_images(h, st));
    return NNEST_OK;
}

int nnest_maf_train_epoch(nnest_nvp_t *h, const float *rows_dev, int n_train, int batch, float lr, float weight_decay, float *loss_sum_dev,
                          void *stream) {
    if (!h || !rows_dev || !loss_sum_dev) return fail(NNEST_E_ARG, "NULL argument");
    if (h->s.kind != FLOW_KIND_MAF) return fail(NNEST_E_ARG, "not a MAF handle (nnest_maf_create)");
    if (n_train < 1 || batch < 1 || batch > 128) return fail(NNEST_E_UNSUPPORTED, "batch=%d outside [1,128]", batch);
    if (h->s.L > 2) return fail(NNEST_E_UNSUPPORTED, "maf: num_layers=%d > 2 has no training kernel", h->s.L);
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < n_train; b0 += batch) {   // Trainer._train's loop over the loader (trainer.py:387-403), queued back to back:
        const int M = n_train - b0 < batch ? n_train - b0 : batch;   // two launches per minibatch (gradient; reduce + Adam + images)
        HIP_TRY(launch_maf_train_minibatch(h->s, h->img, h->img_bwd, h->gpos, h->fwd_pos, h->bwd_pos, rows_dev + (size_t)b0 * h->s.D, M, h->w,
                                           h->adam_m, h->adam_v, h->adam_step, lr, weight_decay, loss_sum_dev, h->ticket, h->train_ws, st));
    }
    return NNEST_OK;
}

int nnest_training_jitter(const double *samples_dev, int N, int D, double *out_dev, void *stream) {
    if (!samples_dev || !out_dev || N < 2 || D < 1) return fail(NNEST_E_ARG, "bad arguments");
    HIP_TRY(launch_training_jitter(samples_dev, N, D, out_dev, (hipStream_t)stream));
    return NNEST_OK;
}

}  // extern "C"
