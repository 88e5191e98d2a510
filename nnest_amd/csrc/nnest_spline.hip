// nnest_spline.hip -- host side of the neural-spline flow (reference nnest/networks.py:393-715): the handle, the
// weight-image builder and the extern "C" entry points (include/nnest_hip.h, "spline" section).
//
// Image build (host, float64, once per weight update; x_dim <= 128 so the matrices are tiny): per block the ActNorm
// vectors (networks.py:661-705) and the 1x1 convolution W = P (tril(L,-1)+I) (triu(U,1)+diag(S)) (networks.py:640-645)
// are folded into one affine map per direction,
//     forward  z = x A_f + b_f,  A_f = diag(e^s) W,        b_f = t W
//     inverse  x = z A_b + b_b,  A_b = W^-1 diag(e^-s),     b_b = -t e^-s
// with log|det| = sum(s) + sum(log|S|) kept as a per-block constant, and every matrix is laid out as MFMA A-operand
// fragments in the slot numbering of spline_tile.h.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "ensemble_common.h"
#include "mcmc_walk.h"
#include "importance_walk.h"
#include "mcmc_mixed.h"
#include "mcmc_adapt.h"
#include "mcmc_gdata.h"
#include "glm_data.h"
#include "gauss_prior.h"
#include "importance_glm.h"
#include "slice_glm.h"
#include <limits.h>
#include "mh_glm.h"
#include "nnest_internal.h"
#include "mh_common.h"

using namespace nnest;

#include "spline_host.h"

static thread_local char g_serr[512] = "";
int nnest::spline_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_serr, sizeof(g_serr), fmt, ap);
    va_end(ap);
    nnest::set_last_error(g_serr);  // read back through nnest_hip_last_error()
    return code;
}


int nnest::spline_mlp_params(int nin, int nout, int H) { return H * nin + H + 2 * (H * H + H) + nout * H + nout; }

static SplineShape make_shape(int D, int H, int B, int K, float tail) {
    SplineShape s;
    memset(&s, 0, sizeof(s));
    s.D = D; s.H = H; s.B = B; s.K = K; s.tail = tail;
    s.nu = D / 2; s.nl = D - s.nu;
    s.NTh = (s.nl + 15) / 16;
    s.NH = H / 16;
    s.SL = (s.nl + 3) / 4; s.SU = (s.nu + 3) / 4;
    s.aff_floats = (2 * s.NTh) * (2 * s.NTh) * 256 + 2 * s.NTh * 16;
    s.f1_floats = spl_cond_floats(s.NTh, s.NH, s.SU);
    s.f2_floats = spl_cond_floats(s.NTh, s.NH, s.SL);
    s.blk_floats = 2 * s.aff_floats + s.f1_floats + s.f2_floats + 4;
    s.image_floats = B * s.blk_floats;
    const int P = 3 * K - 1;
    s.blk_params = 2 * D + (2 * D * D + D) + spline_mlp_params(s.nl, P * s.nu, H) + spline_mlp_params(s.nu, P * s.nl, H);
    s.num_params = B * s.blk_params;
    s.base_beta = 0.f;
    s.base_const = -0.91893853320467274f;
    return s;
}

// slot -> dimension of the full vector (or -1): half hf, tile t, k-step / register r, lane group g
static inline int slot_dim(const SplineShape &s, int hf, int t, int r, int g) {
    const int j = 16 * t + 4 * r + g, n = hf ? s.nu : s.nl;
    return j < n ? (hf ? s.nl : 0) + j : -1;
}

// out = in M + b: weights [to][ti][r][lane], bias [to][g][r]
static void build_affine(const SplineShape &s, const std::vector<double> &M, const std::vector<double> &b, float *img) {
    const int NTh = s.NTh, T2 = 2 * NTh, D = s.D;
    for (int to = 0; to < T2; ++to)
        for (int ti = 0; ti < T2; ++ti)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15;
                    const int di = slot_dim(s, ti / NTh, ti % NTh, r, g);
                    const int dout = slot_dim(s, to / NTh, to % NTh, i & 3, i >> 2);
                    img[(size_t)((to * T2 + ti) * 4 + r) * 64 + lane] = (di >= 0 && dout >= 0) ? (float)M[(size_t)di * D + dout] : 0.f;
                }
    float *bias = img + (size_t)T2 * T2 * 256;
    for (int to = 0; to < T2; ++to)
        for (int g = 0; g < 4; ++g)
            for (int r = 0; r < 4; ++r) {
                const int dout = slot_dim(s, to / NTh, to % NTh, r, g);
                bias[(to * 4 + g) * 4 + r] = dout >= 0 ? (float)b[dout] : 0.f;
            }
}

// conditioner MLP(nin -> H -> H -> H -> 23 nout)  (networks.py:393-409; NSF_CL :570-574)
static void build_cond(const SplineShape &s, const float *p, int nin, int nout, float *img) {
    const int H = s.H, NH = s.NH, NTh = s.NTh, S = (nout + 3) / 4, P = SPL_P;
    const float *W0 = p, *b0 = W0 + H * nin, *W1 = b0 + H, *b1 = W1 + H * H, *W2 = b1 + H, *b2 = W2 + H * H, *W3 = b2 + H,
                *b3 = W3 + (size_t)P * nout * H;
    float *L1 = img, *L2 = L1 + NH * NTh * 256, *L3 = L2 + NH * NH * 256, *bb = L3 + NH * NH * 256, *L4 = bb + 3 * 16 * NH,
          *B4 = L4 + (size_t)S * SPL_QT * NH * 256;
    for (int ht = 0; ht < NH; ++ht)
        for (int t = 0; t < NTh; ++t)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15, j = 16 * t + 4 * r + g;
                    L1[(size_t)((ht * NTh + t) * 4 + r) * 64 + lane] = j < nin ? W0[(16 * ht + i) * nin + j] : 0.f;
                }
    for (int l = 0; l < 2; ++l) {
        const float *W = l ? W2 : W1;
        float *Lw = l ? L3 : L2;
        for (int hto = 0; hto < NH; ++hto)
            for (int hti = 0; hti < NH; ++hti)
                for (int r = 0; r < 4; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int g = lane >> 4, i = lane & 15;
                        Lw[(size_t)((hto * NH + hti) * 4 + r) * 64 + lane] = W[(16 * hto + i) * H + 16 * hti + 4 * g + r];
                    }
    }
    for (int j = 0; j < H; ++j) { bb[j] = b0[j]; bb[H + j] = b1[j]; bb[2 * H + j] = b2[j]; }
    for (int sidx = 0; sidx < S; ++sidx)
        for (int q = 0; q < SPL_QT; ++q) {
            for (int hti = 0; hti < NH; ++hti)
                for (int r = 0; r < 4; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int g = lane >> 4, i = lane & 15;
                        const int jo = 4 * sidx + (i >> 2), pp = 4 * q + (i & 3);
                        const bool ok = jo < nout && pp < P;
                        L4[(size_t)(((sidx * SPL_QT + q) * NH + hti) * 4 + r) * 64 + lane] =
                            ok ? W3[(size_t)(jo * P + pp) * H + 16 * hti + 4 * g + r] : 0.f;
                    }
            for (int g = 0; g < 4; ++g)
                for (int r = 0; r < 4; ++r) {
                    const int jo = 4 * sidx + g, pp = 4 * q + r;
                    B4[((sidx * SPL_QT + q) * 4 + g) * 4 + r] = (jo < nout && pp < P) ? b3[jo * P + pp] : 0.f;
                }
        }
}

static bool invert(std::vector<double> &A, int D, std::vector<double> &Ai) {  // Gauss-Jordan, partial pivoting
    Ai.assign((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) Ai[(size_t)i * D + i] = 1.0;
    for (int c = 0; c < D; ++c) {
        int piv = c;
        for (int r = c + 1; r < D; ++r)
            if (fabs(A[(size_t)r * D + c]) > fabs(A[(size_t)piv * D + c])) piv = r;
        if (A[(size_t)piv * D + c] == 0.0) return false;
        if (piv != c)
            for (int j = 0; j < D; ++j) {
                std::swap(A[(size_t)c * D + j], A[(size_t)piv * D + j]);
                std::swap(Ai[(size_t)c * D + j], Ai[(size_t)piv * D + j]);
            }
        const double inv = 1.0 / A[(size_t)c * D + c];
        for (int j = 0; j < D; ++j) { A[(size_t)c * D + j] *= inv; Ai[(size_t)c * D + j] *= inv; }
        for (int r = 0; r < D; ++r) {
            if (r == c) continue;
            const double f = A[(size_t)r * D + c];
            if (f == 0.0) continue;
            for (int j = 0; j < D; ++j) { A[(size_t)r * D + j] -= f * A[(size_t)c * D + j]; Ai[(size_t)r * D + j] -= f * Ai[(size_t)c * D + j]; }
        }
    }
    return true;
}

int nnest::spline_build_image(nnest_spline *h) {
    const SplineShape &s = h->s;
    const int D = s.D;
    h->img_host.assign((size_t)s.image_floats, 0.f);
    std::vector<double> Lm((size_t)D * D), PL((size_t)D * D), W((size_t)D * D), Wc, Wi, M((size_t)D * D), bvec(D);
    for (int b = 0; b < s.B; ++b) {
        const float *pb = h->w.data() + (size_t)b * s.blk_params;
        const float *sv = pb, *tv = pb + D, *Lp = pb + 2 * D, *Sp = Lp + D * D, *Up = Sp + D, *f1 = Up + D * D;
        const float *f2 = f1 + spline_mlp_params(s.nl, SPL_P * s.nu, s.H);
        const float *Pm = h->perm.data() + (size_t)b * D * D;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) Lm[(size_t)i * D + j] = j < i ? (double)Lp[i * D + j] : (i == j ? 1.0 : 0.0);
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                double acc = 0;
                for (int k = 0; k < D; ++k) acc += (double)Pm[i * D + k] * Lm[(size_t)k * D + j];
                PL[(size_t)i * D + j] = acc;
            }
        double ldc = 0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                double acc = 0;
                for (int k = 0; k <= j; ++k) acc += PL[(size_t)i * D + k] * (k < j ? (double)Up[k * D + j] : (double)Sp[k]);
                W[(size_t)i * D + j] = acc;
            }
        for (int d = 0; d < D; ++d) ldc += (double)sv[d] + log(fabs((double)Sp[d]));
        Wc = W;
        if (!invert(Wc, D, Wi)) return spline_fail(NNEST_E_ARG, "block %d: the 1x1 convolution matrix is singular", b);
        float *blk = h->img_host.data() + (size_t)b * s.blk_floats;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) M[(size_t)i * D + j] = exp((double)sv[i]) * W[(size_t)i * D + j];
        for (int j = 0; j < D; ++j) {
            double acc = 0;
            for (int i = 0; i < D; ++i) acc += (double)tv[i] * W[(size_t)i * D + j];
            bvec[j] = acc;
        }
        build_affine(s, M, bvec, blk);
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) M[(size_t)i * D + j] = Wi[(size_t)i * D + j] * exp(-(double)sv[j]);
        for (int j = 0; j < D; ++j) bvec[j] = -(double)tv[j] * exp(-(double)sv[j]);
        build_affine(s, M, bvec, blk + s.aff_floats);
        build_cond(s, f1, s.nl, s.nu, blk + 2 * s.aff_floats);
        build_cond(s, f2, s.nu, s.nl, blk + 2 * s.aff_floats + s.f1_floats);
        blk[2 * s.aff_floats + s.f1_floats + s.f2_floats] = (float)ldc;
    }
    return NNEST_OK;
}

extern "C" {

int nnest_spline_create(int D, int H, int B, int K, float tail_bound, nnest_spline_t **out) {
    if (!out) return spline_fail(NNEST_E_ARG, "out is NULL");
    *out = nullptr;
    if (D < 2 || H < 1 || B < 1 || K < 1 || !(tail_bound > 0)) return spline_fail(NNEST_E_ARG, "bad shape D=%d H=%d B=%d K=%d", D, H, B, K);
    if (H % 16 != 0) return spline_fail(NNEST_E_UNSUPPORTED, "hidden_dim=%d: the gfx950 kernels tile the hidden layers by 16", H);
    SplineShape s = make_shape(D, H, B, K, tail_bound);
    if (!spline_shape_supported(s))
        return spline_fail(NNEST_E_UNSUPPORTED, "spline flow: x_dim=%d hidden_dim=%d num_bins=%d not instantiated (num_bins 8; x_dim <= 128 at "
                     "hidden_dim 16, <= 64 at 32)", D, H, K);
    nnest_spline *h = new nnest_spline();
    h->s = s;
    h->img = nullptr;
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return spline_fail(NNEST_E_HIP, "hipGetDevice failed (no GPU?)"); }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, h->device) != hipSuccess) { delete h; return spline_fail(NNEST_E_HIP, "hipGetDeviceProperties failed"); }
    h->num_cu = p.multiProcessorCount;
    h->w.assign((size_t)s.num_params, 0.f);
    h->perm.assign((size_t)B * D * D, 0.f);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < D; ++i) h->perm[((size_t)b * D + i) * D + i] = 1.f;
    if (hipMalloc((void **)&h->img, (size_t)s.image_floats * sizeof(float)) != hipSuccess) {
        delete h;
        return spline_fail(NNEST_E_HIP, "device allocation failed");
    }
    *out = h;
    return NNEST_OK;
}

int nnest_spline_destroy(nnest_spline_t *h) {
    if (!h) return NNEST_OK;
    (void)hipFree(h->img);
    (void)hipFree(h->w_dev); (void)hipFree(h->adam_m); (void)hipFree(h->adam_v); (void)hipFree(h->best_w); (void)hipFree(h->pi_dev); (void)hipFree(h->pos_dev);
    (void)hipFree(h->wmat); (void)hipFree(h->timg); (void)hipFree(h->partial); (void)hipFree(h->grad); (void)hipFree(h->gwsum);
    (void)hipFree(h->stash); (void)hipFree(h->gbuf); (void)hipFree(h->hbuf); (void)hipFree(h->keep); (void)hipFree(h->losses_dev); (void)hipFree(h->ctl_dev); (void)hipFree(h->epoch_losses_dev);
    if (h->ctl_host) (void)hipHostFree(h->ctl_host);
    spline_rows_free(h);
    delete h;
    return NNEST_OK;
}

int nnest_spline_num_params(const nnest_spline_t *h) { return h ? h->s.num_params : -1; }

int nnest_spline_set_base(nnest_spline_t *h, float beta) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (!(beta >= 0.f)) return spline_fail(NNEST_E_ARG, "beta=%g: 0 selects N(0, I), beta > 0 GeneralisedNormal(0, 1, beta)", (double)beta);
    h->s.base_beta = beta;
    h->s.base_const = beta == 0.f ? -0.91893853320467274f : (float)(log((double)beta) - log(2.0) - lgamma(1.0 / (double)beta));
    return NNEST_OK;
}

int nnest_spline_load_weights(nnest_spline_t *h, const float *packed_host, const float *perm_host, void *stream) {
    if (!h || !packed_host) return spline_fail(NNEST_E_ARG, "NULL argument");
    memcpy(h->w.data(), packed_host, h->w.size() * sizeof(float));
    if (perm_host) memcpy(h->perm.data(), perm_host, h->perm.size() * sizeof(float));
    h->w_dev_current = false;  // the training copy on the device is refreshed on its next use
    int rc = spline_build_image(h);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    SHIP_TRY(hipMemcpyAsync(h->img, h->img_host.data(), h->img_host.size() * sizeof(float), hipMemcpyHostToDevice, st));
    SHIP_TRY(hipStreamSynchronize(st));
    return NNEST_OK;
}

int nnest_spline_store_weights(nnest_spline_t *h, float *packed_host, float *perm_host, void *stream) {
    (void)stream;
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (packed_host) memcpy(packed_host, h->w.data(), h->w.size() * sizeof(float));
    if (perm_host) memcpy(perm_host, h->perm.data(), h->perm.size() * sizeof(float));
    return NNEST_OK;
}

static int scheck_rows(const nnest_spline_t *h, const void *a, const void *b, int N) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (N < 0) return spline_fail(NNEST_E_ARG, "N=%d < 0", N);
    if (N > 0 && (!a || !b)) return spline_fail(NNEST_E_ARG, "NULL device buffer");
    return NNEST_OK;
}

static int scheck_like(const nnest_like_t *like, int D, LikeSpec *out) {
    if (!like) return spline_fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    if (like->id == NNEST_LIKE_EGGBOX && D != 2) return spline_fail(NNEST_E_ARG, "Eggbox is defined for x_dim = 2 (likelihoods.py:97-102)");
    if (like->id == NNEST_LIKE_GAUSSMIX && D < 2) return spline_fail(NNEST_E_ARG, "GaussianMix needs x_dim >= 2");
    out->id = like->id;
    out->scale = like->scale;
    for (int i = 0; i < 6; ++i) out->p[i] = like->params[i];
    return NNEST_OK;
}

int nnest_spline_forward(nnest_spline_t *h, const float *x_dev, float *z_dev, float *logdet_dev, int N, void *stream) {
    int rc = scheck_rows(h, x_dev, z_dev, N);
    if (rc) return rc;
    SHIP_TRY(launch_spline_pass(h->img, h->s, PASS_FORWARD, x_dev, z_dev, logdet_dev, nullptr, nullptr, N, LikeSpec(), h->num_cu,
                                (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_spline_inverse(nnest_spline_t *h, const float *z_dev, float *x_dev, float *logdet_dev, int N, void *stream) {
    int rc = scheck_rows(h, z_dev, x_dev, N);
    if (rc) return rc;
    SHIP_TRY(launch_spline_pass(h->img, h->s, PASS_INVERSE, z_dev, x_dev, logdet_dev, nullptr, nullptr, N, LikeSpec(), h->num_cu,
                                (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_spline_log_probs(nnest_spline_t *h, const float *x_dev, float *logp_dev, int N, void *stream) {
    int rc = scheck_rows(h, x_dev, logp_dev, N);
    if (rc) return rc;
    SHIP_TRY(launch_spline_pass(h->img, h->s, PASS_LOGPROB, x_dev, logp_dev, nullptr, nullptr, nullptr, N, LikeSpec(), h->num_cu,
                                (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_spline_inverse_loglike(nnest_spline_t *h, const nnest_like_t *like, const float *z_dev, float *x_dev,
                                 float *logdet_dev, double *logl_dev, int *inbox_dev, int N, void *stream) {
    int rc = scheck_rows(h, z_dev, logl_dev, N);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = scheck_like(like, h->s.D, &lk))) return rc;
    SHIP_TRY(launch_spline_pass(h->img, h->s, PASS_INVERSE_LOGLIKE, z_dev, x_dev, logdet_dev, logl_dev, inbox_dev, N, lk, h->num_cu,
                                (hipStream_t)stream));
    return NNEST_OK;
}

int nnest_spline_mh_form_for(const nnest_spline_t *h, int C, int flags) {
    if (!h || C <= 0) return -1;
    return spline_mh_form(h->s, C, flags, h->num_cu);
}

int nnest_spline_mh_constrained_steps(nnest_spline_t *h, const nnest_like_t *like, float *z_dev, float *x_dev, double *logl_dev,
                                      double loglstar, float step_size, int steps, int C, int flags, const float *noise_dz_dev,
                                      const float *noise_u_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev,
                                      double *hist_logl_dev, int *n_accept_dev, int *n_call_dev, float *scale_out_dev,
                                      void *sync_dev, void *stream) {
    int rc = scheck_rows(h, z_dev, logl_dev, C);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = scheck_like(like, h->s.D, &lk))) return rc;
    if (steps < 0) return spline_fail(NNEST_E_ARG, "steps=%d < 0", steps);
    if ((noise_dz_dev == nullptr) != (noise_u_dev == nullptr))
        return spline_fail(NNEST_E_ARG, "noise_dz_dev and noise_u_dev must both be given or both be NULL");
    if ((flags & NNEST_MH_DYNAMIC_BATCH) && !sync_dev) return spline_fail(NNEST_E_ARG, "NNEST_MH_DYNAMIC_BATCH needs sync_dev");
    hipError_t e = launch_spline_mh(h->img, h->s, lk, z_dev, x_dev, logl_dev, loglstar, step_size, steps, C, flags, noise_dz_dev,
                                    noise_u_dev, seed, walker_offset, hist_x_dev, hist_logl_dev, n_accept_dev, n_call_dev,
                                    scale_out_dev, (unsigned long long *)sync_dev, h->num_cu, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "batch-wide step rule: C=%d walkers do not fit a resident grid", C);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mh: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_spline_slice_form_for(const nnest_spline_t *h, int C, int flags) {
    if (!h || C <= 0 || (flags & ~15)) return -1;
    return spline_slice_form(h->s, C, flags, h->num_cu);
}

int nnest_spline_slice_steps(nnest_spline_t *h, const nnest_like_t *like, float *z_dev, float *x_dev, double *logl_dev, double loglstar,
                             float width, int steps, int C, int max_stepout, int max_shrink, int flags, const float *noise_dz_dev,
                             uint64_t seed, uint64_t walker_offset, float *hist_x_dev, int *n_call_dev, int *n_move_dev, int *n_eval_dev,
                             void *stream) {
    int rc = scheck_rows(h, z_dev, logl_dev, C);
    if (rc) return rc;
    LikeSpec lk;
    if ((rc = scheck_like(like, h->s.D, &lk))) return rc;
    if (!slice_params_ok(steps, max_stepout, max_shrink, width))
        return spline_fail(NNEST_E_ARG, "steps=%d max_stepout=%d (0..2^24) max_shrink=%d (1..60) width=%g", steps, max_stepout, max_shrink, (double)width);
    if (flags & ~15) return spline_fail(NNEST_E_ARG, "flags=0x%x: bits 0..3 only (NNEST_SPLINE_SLICE_FORM)", flags);
    if (C > 0 && spline_slice_form(h->s, C, flags, h->num_cu) < 0)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline slice proposal: form %d pinned, x_dim=%d (the pair form needs x_dim > 32)", (flags & 15) - 1, h->s.D);
    const SliceArgs a = {z_dev, x_dev, logl_dev, loglstar, width, steps, C, max_stepout, max_shrink, lk, seed, walker_offset, noise_dz_dev,
                         hist_x_dev, nullptr, n_call_dev, n_move_dev, n_eval_dev};
    hipError_t e = launch_spline_slice(SplArgs{h->img, h->s}, a, flags, h->num_cu, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return spline_fail(NNEST_E_UNSUPPORTED, "spline slice proposal: x_dim=%d hidden_dim=%d not instantiated", h->s.D, h->s.H);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_slice: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_spline_ensemble_max_walkers(nnest_spline_t *h, int like_id) {
    if (!h || like_id < 0 || like_id >= NNEST_LIKE_COUNT) return -1;
    int n = 0;
    if (spline_ensemble_max_walkers(SplArgs{h->img, h->s}, h->num_cu, &n) != hipSuccess) return -1;
    return n;
}

// (the checks that need no handle come first: they answer on a machine without a GPU, where no handle can exist)
int nnest_spline_ensemble_steps(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, float *z_out_dev,
                                float *x_out_dev, double *lp_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_lp_dev,
                                int *n_accept_dev, int *work_dev, int C, int steps, uint64_t step0, uint64_t seed, int constrained,
                                double loglstar, void *stream) {
    if (!like) return spline_fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    int rc = ensemble_sizes(C, steps);
    if (rc) return rc;
    if (!t_std_dev || !t_mean_dev || !z_in_dev || !z_out_dev || !x_out_dev || !lp_out_dev || !work_dev ||
        (steps > 0 && (!hist_z_dev || !hist_x_dev || !hist_lp_dev)))
        return spline_fail(NNEST_E_ARG, "NULL device buffer");
    if (!lo_dev != !hi_dev) return spline_fail(NNEST_E_ARG, "lo_dev and hi_dev: both or neither");
    if ((const void *)z_in_dev == (const void *)z_out_dev)
        return spline_fail(NNEST_E_ARG, "z_in_dev must not be z_out_dev (partners read it during the launch)");
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = scheck_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    a.t_std = t_std_dev; a.t_mean = t_mean_dev; a.lo = lo_dev; a.hi = hi_dev;
    a.z_in = z_in_dev; a.lp_in = lp_in_dev; a.z_out = z_out_dev; a.x_out = x_out_dev; a.lp_out = lp_out_dev;
    a.hist_z = hist_z_dev; a.hist_x = hist_x_dev; a.hist_lp = hist_lp_dev; a.n_accept = n_accept_dev; a.work = work_dev;
    a.C = C; a.S = steps; a.constrained = constrained ? 1 : 0; a.step0 = (uint32_t)step0; a.seed = seed; a.loglstar = loglstar;
    char msg[400];
    msg[0] = 0;
    rc = launch_spline_ensemble(SplArgs{h->img, h->s}, a, h->num_cu, (hipStream_t)stream, msg, sizeof(msg));
    if (rc) return spline_fail(rc, "%s", msg);
    return NNEST_OK;
}

// the random-walk Metropolis run through the spline flow (nnest_spline_mcmc.hip); the argument checks of nnest_mcmc_steps.
// beta NULL: nnest_spline_mcmc_steps; else nnest_spline_mcmc_tempered_steps at *beta
static int spline_mcmc_steps_entry(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                   const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                   const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                   float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                   float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, const double *beta,
                                   void *stream) {
    if (!like) return spline_fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
    int rc;
    if (beta && (rc = mcmc_beta_ok(*beta))) return rc;
    McmcTemperedArgs a;
    memset(&a, 0, sizeof(a));
    a.beta = beta ? *beta : 1.0;
    rc = mcmc_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev, lp_out_dev,
                   logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0, seed, walker_offset);
    if (rc) return rc;
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if ((rc = scheck_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    const hipError_t e = beta ? launch_spline_mcmc_tempered(SplArgs{h->img, h->s}, a, (hipStream_t)stream)
                              : launch_spline_mcmc(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mcmc: x_dim=%d hidden_dim=%d not instantiated", h->s.D, h->s.H);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mcmc: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_spline_mcmc_steps(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                            const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                            const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                            float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                            float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, void *stream) {
    return spline_mcmc_steps_entry(h, like, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev,
                                   lp_out_dev, logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0,
                                   seed, walker_offset, nullptr, stream);
}

int nnest_spline_mcmc_tempered_steps(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                     const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                     const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev,
                                     double *logl_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev,
                                     int C, int steps, float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta,
                                     void *stream) {
    return spline_mcmc_steps_entry(h, like, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_in_dev, lp_in_dev, logl_in_dev, z_out_dev, x_out_dev,
                                   lp_out_dev, logl_out_dev, hist_z_dev, hist_x_dev, hist_logl_dev, n_accept_dev, C, steps, step_size, step0,
                                   seed, walker_offset, &beta, stream);
}

// what nnest_spline_mcmc_mixed_steps takes, asked before a launch (and by the entry itself): the refusals name their reason -- the
// base's in the words of nnest_spline_importance_check
int nnest_spline_mcmc_mixed_check(nnest_spline_t *h, int like_id) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_UNSUPPORTED, "mcmc mixed: unknown likelihood id %d", like_id);
    if (h->s.base_beta != 0.f)
        return spline_fail(NNEST_E_UNSUPPORTED, "mcmc mixed: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only",
                           (double)h->s.base_beta);
    McmcMixedArgs probe;
    memset(&probe, 0, sizeof(probe));   // (C = 0: the shape's verdict, nothing is launched)
    if (launch_spline_mcmc_mixed(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mcmc mixed: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D,
                           h->s.H);
    return NNEST_OK;
}

// the mixed walk through the spline flow (nnest_spline_mcmc_mixed.hip); the argument checks of nnest_mcmc_mixed_steps
int nnest_spline_mcmc_mixed_steps(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, void *stream) {
    if (!like) return spline_fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
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
    if ((rc = nnest_spline_mcmc_mixed_check(h, like->id))) return rc;
    if ((rc = scheck_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    const hipError_t e = launch_spline_mcmc_mixed(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mcmc_mixed: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_mcmc_adapt_steps takes, asked before a launch (and by the entry itself): as nnest_spline_mcmc_mixed_check answers
int nnest_spline_mcmc_adapt_check(nnest_spline_t *h, int like_id) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_UNSUPPORTED, "mcmc adapt: unknown likelihood id %d", like_id);
    if (h->s.base_beta != 0.f)
        return spline_fail(NNEST_E_UNSUPPORTED, "mcmc adapt: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only",
                           (double)h->s.base_beta);
    McmcAdaptArgs probe;
    memset(&probe, 0, sizeof(probe));   // (C = 0: the shape's verdict, nothing is launched)
    if (launch_spline_mcmc_adapt(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mcmc adapt: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D,
                           h->s.H);
    return NNEST_OK;
}

// the adaptive walk through the spline flow (nnest_spline_mcmc_adapt.hip); the argument checks of nnest_mcmc_adapt_steps
int nnest_spline_mcmc_adapt_steps(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev, double *hist_step_dev,
                                  uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream) {
    if (!like) return spline_fail(NNEST_E_ARG, "like is NULL");
    if (like->id < 0 || like->id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_ARG, "unknown likelihood id %d", like->id);
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
    if ((rc = nnest_spline_mcmc_adapt_check(h, like->id))) return rc;
    if ((rc = scheck_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    const hipError_t e = launch_spline_mcmc_adapt(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mcmc_adapt: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_mcmc_gdata_steps takes, asked before a launch (and by the entry itself): the shapes and the base of
// nnest_spline_mcmc_adapt_check, and a descriptor of the flow's x_dim
int nnest_spline_mcmc_gdata_check(nnest_spline_t *h, int D) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (h->s.base_beta != 0.f)
        return spline_fail(NNEST_E_UNSUPPORTED, "mcmc gdata: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only",
                           (double)h->s.base_beta);
    McmcGdataArgs probe;
    memset(&probe, 0, sizeof(probe));   // (C = 0: the shape's verdict, nothing is launched)
    if (launch_spline_mcmc_gdata(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mcmc gdata: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D,
                           h->s.H);
    if (D != h->s.D) return spline_fail(NNEST_E_ARG, "mcmc gdata: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// the adaptive walk through the spline flow on the Gaussian likelihood from user data (nnest_spline_mcmc_gdata.hip); the argument
// checks of nnest_mcmc_gdata_steps
int nnest_spline_mcmc_gdata_steps(nnest_spline_t *h, const nnest_gdata_t *gdata, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev, double *hist_step_dev,
                                  uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream) {
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
    if ((rc = nnest_spline_mcmc_gdata_check(h, a.gd.D))) return rc;
    a.like.scale = 1.0f;
    const hipError_t e = launch_spline_mcmc_gdata(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mcmc_gdata: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_mcmc_glm_steps takes, asked before a launch (and by the entry itself): the shapes and the base of
// nnest_spline_mcmc_adapt_check, and a descriptor of the flow's x_dim
int nnest_spline_mcmc_glm_check(nnest_spline_t *h, int D) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (h->s.base_beta != 0.f)
        return spline_fail(NNEST_E_UNSUPPORTED, "mcmc glm: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only",
                           (double)h->s.base_beta);
    McmcGlmArgs probe;
    memset(&probe, 0, sizeof(probe));   // (C = 0: the shape's verdict, nothing is launched)
    if (launch_spline_mcmc_glm(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mcmc glm: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D,
                           h->s.H);
    if (D != h->s.D) return spline_fail(NNEST_E_ARG, "mcmc glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// the adaptive walk through the spline flow on the regression likelihoods of the user's data (nnest_spline_mcmc_glm.hip); the argument
// checks of nnest_mcmc_glm_steps
int nnest_spline_mcmc_glm_steps(nnest_spline_t *h, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev, double *hist_step_dev,
                                  uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream) {
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
    if ((rc = nnest_spline_mcmc_glm_check(h, a.gl.D))) return rc;
    a.like.scale = 1.0f;
    const hipError_t e = launch_spline_mcmc_glm(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mcmc_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_slice_glm_steps takes, asked before a launch (and by the entry itself): the team tile's shapes, and a descriptor
// of the flow's x_dim
int nnest_spline_slice_glm_check(nnest_spline_t *h, int D) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    SliceGlmArgs probe;
    memset(&probe, 0, sizeof(probe));   // (C = 0: the shape's verdict, nothing is launched)
    if (launch_spline_slice_glm(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline slice glm: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D,
                           h->s.H);
    if (D != h->s.D) return spline_fail(NNEST_E_ARG, "slice glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// the slice proposal through the spline flow on the regression likelihoods of the user's data (nnest_spline_slice_glm.hip); the
// argument checks of nnest_slice_glm_steps
int nnest_spline_slice_glm_steps(nnest_spline_t *h, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev,
                                 float *z_dev, float *x_dev, double *logl_dev, double loglstar, float width, int steps, int C,
                                 int max_stepout, int max_shrink, const float *noise_dz_dev, uint64_t seed, uint64_t walker_offset,
                                 float *hist_x_dev, int *n_call_dev, int *n_move_dev, int *n_eval_dev, void *stream) {
    SliceGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if (!t_std_dev != !t_mean_dev) return spline_fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (!slice_params_ok(steps, max_stepout, max_shrink, width))
        return spline_fail(NNEST_E_ARG, "steps=%d max_stepout=%d (0..2^24) max_shrink=%d (1..60) width=%g", steps, max_stepout, max_shrink, (double)width);
    if ((rc = scheck_rows(h, z_dev, logl_dev, C))) return rc;
    if ((rc = nnest_spline_slice_glm_check(h, a.gl.D))) return rc;
    a.z = z_dev; a.x = x_dev; a.logl = logl_dev; a.loglstar = loglstar; a.width = width; a.steps = steps; a.C = C;
    a.max_out = max_stepout; a.max_shrink = max_shrink; a.like.scale = 1.0f; a.seed = seed; a.walker_offset = walker_offset;
    a.noise_dz = noise_dz_dev; a.hist_x = hist_x_dev; a.n_call = n_call_dev; a.n_move = n_move_dev; a.n_eval = n_eval_dev;
    a.t_std = t_std_dev; a.t_mean = t_mean_dev;
    const hipError_t e = launch_spline_slice_glm(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_slice_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_mh_glm_steps takes, asked before a launch (and by the entry itself): the flags' three settings, the team tile's
// shapes, a descriptor of the flow's x_dim, and -- under the batch rule -- a grid that is proven resident
int nnest_spline_mh_glm_check(nnest_spline_t *h, int D, int C, int flags) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (!mh_glm_flags_ok(flags, true))
        return spline_fail(NNEST_E_ARG, "spline mh glm: flags 0x%x: 0 (fixed step), NNEST_MH_DYNAMIC_STEP (the rule per 16-walker tile) or "
                           "NNEST_MH_DYNAMIC_BATCH | NNEST_MH_LAG(0..15); the unconstrained walk is nnest_spline_mcmc_glm_steps, and there are "
                           "no forms, warm-up steps or sync halves", flags);
    int cap = INT_MAX;
    for (int fam : {GLM_LOGISTIC, GLM_POISSON}) {   // (the smaller of the two families' grids: the verdict holds for either)
        MhGlmArgs probe;
        memset(&probe, 0, sizeof(probe));
        probe.gl.family = fam;
        int c = 0;
        hipError_t e = launch_spline_mh_glm(SplArgs{h->img, h->s}, probe, h->num_cu, &c, nullptr);
        if (e == hipErrorInvalidConfiguration)
            return spline_fail(NNEST_E_UNSUPPORTED, "spline mh glm: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D, h->s.H);
        if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "spline mh glm: occupancy query: %s", hipGetErrorString(e));
        cap = c < cap ? c : cap;
    }
    if (D != h->s.D) return spline_fail(NNEST_E_ARG, "mh glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    if (C < 0) return spline_fail(NNEST_E_ARG, "mh glm: C=%d < 0", C);
    if ((flags & NNEST_MH_DYNAMIC_BATCH) && (C + 15) / 16 > cap)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mh glm: the batch-wide step rule needs every workgroup resident: C=%d walkers are %d "
                           "workgroups, %d fit this device", C, (C + 15) / 16, cap);
    return NNEST_OK;
}

// the constrained Metropolis proposal through the spline flow on the regression likelihoods of the user's data
// (nnest_spline_mh_glm.hip); the argument checks of nnest_mh_glm_steps
int nnest_spline_mh_glm_steps(nnest_spline_t *h, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, float *z_dev,
                              float *x_dev, double *logl_dev, double loglstar, float step_size, int steps, int C, int flags,
                              const float *noise_dz_dev, const float *noise_u_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev,
                              double *hist_logl_dev, int *n_accept_dev, int *n_call_dev, float *scale_out_dev, void *sync_dev, void *stream) {
    MhGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if (!t_std_dev != !t_mean_dev) return spline_fail(NNEST_E_ARG, "t_std_dev and t_mean_dev: both or neither");
    if (steps < 0) return spline_fail(NNEST_E_ARG, "steps=%d < 0", steps);
    if ((noise_dz_dev == nullptr) != (noise_u_dev == nullptr))
        return spline_fail(NNEST_E_ARG, "noise_dz_dev and noise_u_dev must both be given or both be NULL");
    if ((rc = scheck_rows(h, z_dev, logl_dev, C))) return rc;
    if ((rc = nnest_spline_mh_glm_check(h, a.gl.D, C, flags))) return rc;
    if ((flags & NNEST_MH_DYNAMIC_BATCH) && !sync_dev) return spline_fail(NNEST_E_ARG, "NNEST_MH_DYNAMIC_BATCH needs sync_dev");
    a.z = z_dev; a.x = x_dev; a.logl = logl_dev; a.loglstar = loglstar; a.step_size = step_size; a.steps = steps; a.C = C; a.flags = flags;
    a.like.scale = 1.0f; a.noise_dz = noise_dz_dev; a.noise_u = noise_u_dev; a.seed = seed; a.walker_offset = walker_offset;
    a.hist_x = hist_x_dev; a.hist_logl = hist_logl_dev; a.n_accept = n_accept_dev; a.n_call = n_call_dev; a.scale_out = scale_out_dev;
    a.sync = (flags & NNEST_MH_DYNAMIC_BATCH) ? (unsigned long long *)sync_dev : nullptr;
    a.sync_err = a.sync ? reinterpret_cast<int *>(a.sync + mh_sync_words(steps)) : nullptr;   // the word behind the counters
    a.t_std = t_std_dev; a.t_mean = t_mean_dev;
    const hipError_t e = launch_spline_mh_glm(SplArgs{h->img, h->s}, a, h->num_cu, nullptr, (hipStream_t)stream);
    if (e == hipErrorLaunchOutOfResources)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mh glm: the batch-wide step rule needs every workgroup resident: C=%d walkers do not fit "
                           "this device", C);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mh_glm: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_mcmc_glm_prior_steps takes, asked before a launch (and by the entry itself): nnest_spline_mcmc_glm_check's
// verdict -- the kernel is that kernel's with a prior term, and the team tile's shapes are the same
int nnest_spline_mcmc_glm_prior_check(nnest_spline_t *h, int D) {
    int rc;
    if ((rc = nnest_spline_mcmc_glm_check(h, D))) return rc;
    McmcGlmPriorArgs probe;
    memset(&probe, 0, sizeof(probe));   // (C = 0: the shape's verdict, nothing is launched)
    if (launch_spline_mcmc_glm_prior(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline mcmc glm prior: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)",
                           h->s.D, h->s.H);
    return NNEST_OK;
}

// the same walk under the normal priors of gauss_prior.h (nnest_spline_mcmc_glm_prior.hip); the argument checks of
// nnest_mcmc_glm_prior_steps
int nnest_spline_mcmc_glm_prior_steps(nnest_spline_t *h, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior,
                                      const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                                      const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                                      float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                                      double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0,
                                      uint64_t seed, uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev,
                                      const double *step_in_dev, double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps,
                                      double adapt_rate, double target_accept, void *stream) {
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
    if ((rc = nnest_spline_mcmc_glm_prior_check(h, a.gl.D))) return rc;
    a.like.scale = 1.0f;
    const hipError_t e = launch_spline_mcmc_glm_prior(SplArgs{h->img, h->s}, a, (hipStream_t)stream);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_mcmc_glm_prior: %s", hipGetErrorString(e));
    return NNEST_OK;
}

// what nnest_spline_importance_evidence takes, asked before a launch (and by the entry itself): the refusals name their reason
int nnest_spline_importance_check(nnest_spline_t *h, int like_id) {
    if (!h) return spline_fail(NNEST_E_ARG, "NULL handle");
    if (like_id < 0 || like_id >= NNEST_LIKE_COUNT) return spline_fail(NNEST_E_UNSUPPORTED, "importance: unknown likelihood id %d", like_id);
    if (h->s.base_beta != 0.f)
        return spline_fail(NNEST_E_UNSUPPORTED, "importance: GeneralisedNormal base (beta=%g): the kernel draws from N(0, I) only",
                           (double)h->s.base_beta);
    ImpArgs probe;
    memset(&probe, 0, sizeof(probe));   // (M = 0: the shape's verdict, nothing is launched)
    if (launch_spline_importance(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline importance: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)", h->s.D,
                           h->s.H);
    return NNEST_OK;
}

// the importance-sampled evidence through the spline flow (nnest_spline_importance.hip); the argument checks of
// nnest_importance_evidence
int nnest_spline_importance_evidence(nnest_spline_t *h, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                     const float *lo_dev, const float *hi_dev, float *z_out_dev, float *x_out_dev, double *logl_out_dev,
                                     double *logw_out_dev, double *partials_dev, double *sums_dev, int M, uint64_t seed,
                                     uint64_t sample_offset, void *stream) {
    if (!like) return spline_fail(NNEST_E_ARG, "like is NULL");
    ImpArgs a;
    memset(&a, 0, sizeof(a));
    int rc = importance_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_out_dev, x_out_dev, logl_out_dev, logw_out_dev, partials_dev,
                             sums_dev, M, seed, sample_offset);
    if (rc) return rc;
    if ((rc = nnest_spline_importance_check(h, like->id))) return rc;
    if ((rc = scheck_like(like, h->s.D, &a.like))) return rc;
    a.like.scale = 1.0f;
    a.groups = importance_groups(M, IMP_SPLINE_TILE, h->num_cu);
    const hipStream_t st = (hipStream_t)stream;
    SHIP_TRY(launch_importance_begin(sums_dev, st));
    hipError_t e = launch_spline_importance(SplArgs{h->img, h->s}, a, st);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_importance: %s", hipGetErrorString(e));
    SHIP_TRY(launch_importance_combine(partials_dev, sums_dev, a.groups, st));
    return NNEST_OK;
}

// what nnest_spline_importance_glm_evidence takes, asked before a launch (and by the entry itself): nnest_spline_importance_check's
// verdict on the base and the team tile's shapes -- the kernel is that kernel's on another target --, and a descriptor of the
// flow's x_dim
int nnest_spline_importance_glm_check(nnest_spline_t *h, int D) {
    int rc;
    if ((rc = nnest_spline_importance_check(h, NNEST_LIKE_GAUSSIAN))) return rc;
    ImpGlmArgs probe;
    memset(&probe, 0, sizeof(probe));   // (M = 0: the shape's verdict, nothing is launched)
    if (launch_spline_importance_glm(SplArgs{h->img, h->s}, probe, nullptr) == hipErrorInvalidConfiguration)
        return spline_fail(NNEST_E_UNSUPPORTED, "spline importance glm: x_dim=%d hidden_dim=%d not instantiated (the team tile's shapes)",
                           h->s.D, h->s.H);
    if (D != h->s.D) return spline_fail(NNEST_E_ARG, "importance glm: the likelihood's D=%d is not the flow's x_dim=%d", D, h->s.D);
    return NNEST_OK;
}

// the importance-sampled evidence of a regression through the spline flow (nnest_spline_importance_glm.hip); the argument checks of
// nnest_importance_glm_evidence
int nnest_spline_importance_glm_evidence(nnest_spline_t *h, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior,
                                         const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                                         float *z_out_dev, float *x_out_dev, double *logl_out_dev, double *logw_out_dev,
                                         double *partials_dev, double *sums_dev, int M, uint64_t seed, uint64_t sample_offset,
                                         void *stream) {
    ImpGlmArgs a;
    memset(&a, 0, sizeof(a));
    int rc = importance_args(&a, t_std_dev, t_mean_dev, lo_dev, hi_dev, z_out_dev, x_out_dev, logl_out_dev, logw_out_dev, partials_dev,
                             sums_dev, M, seed, sample_offset);
    if (rc) return rc;
    if ((rc = glm_ok(glm, glm ? glm->D : 0, &a.gl))) return rc;
    if (prior) {
        if ((rc = gauss_prior_ok(prior, h ? h->s.D : prior->D, &a.pr))) return rc;   // (no handle: refused below)
        if (lo_dev) return spline_fail(NNEST_E_ARG, "importance glm: a prior together with the box lo_dev / hi_dev (one or the other)");
        a.prior = 1;
    }
    if ((rc = nnest_spline_importance_glm_check(h, a.gl.D))) return rc;
    a.like.scale = 1.0f;
    a.groups = importance_groups(M, IMP_SPLINE_TILE, h->num_cu);
    const hipStream_t st = (hipStream_t)stream;
    SHIP_TRY(launch_importance_begin(sums_dev, st));
    hipError_t e = launch_spline_importance_glm(SplArgs{h->img, h->s}, a, st);
    if (e != hipSuccess) return spline_fail(NNEST_E_HIP, "launch_spline_importance_glm: %s", hipGetErrorString(e));
    SHIP_TRY(launch_importance_combine(partials_dev, sums_dev, a.groups, st));
    return NNEST_OK;
}

}  // extern "C"
