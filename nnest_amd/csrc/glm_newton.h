// glm_newton.h -- the GRADIENT AND CURVATURE of the regression likelihoods of glm_data.h at one theta, and the NEWTON STEP under the
// normal priors of gauss_prior.h (include/nnest_hip.h nnest_glm_curv, nnest_glm_newton_solve; nnest_glm_newton.hip):
// the row terms in float64, the layout of the partials, the tile schedule of the matrix cores and the launchers' declarations.
// Everything here is float64; the float32 descriptor is read as it is and converted exactly.
//   eta_i = o_i + sum_c A[i, c] theta_c      float64, fused multiply-adds, in the kernel's own fixed order
//   l_i                                      glm_term's definition from the double eta_i (NaN where eta_i is not finite)
//   logistic: mu_i = 1 / (1 + e^-eta_i), w_i = mu_i (1 - mu_i), both from t = e^-|eta_i| (no overflow at either end; 1 - mu_i is
//             t / (1 + t) or 1 / (1 + t), never a difference);   poisson: mu_i = w_i = e^eta_i
//   out[0] = logl0 + sum l_i (glm_finish's safe rule),  out[1 + c] = sum_i (y_i - mu_i) A[i, c],
//   out[1 + D + c D + d] = sum_i w_i A[i, c] A[i, d]    (the negative Hessian of log L, a full matrix, the lower triangle a bit copy)
#pragma once
#include "gauss_prior.h"

namespace nnest {

constexpr int GLMNW_ROWS = 64;          // data rows a workgroup stages at a time: one per lane
constexpr int GLMNW_MAX_GROUPS = 256;   // row groups at most: one workgroup a CU of the largest part, whatever the device is
constexpr int GLMNW_STRIDE = 68;        // floats between two columns of the staged block: lane (m, k) reads bank 4 m + k, all 64 distinct
constexpr int GLMNW_SOLVE_THREADS = 128;

// doubles a row group writes: the sum of the terms, the gradient, the packed upper triangle of the negative Hessian (row-major)
__host__ __device__ constexpr int glm_curv_slots(int D) { return 1 + D + D * (D + 1) / 2; }
__host__ __device__ constexpr int glm_curv_packed(int D, int r, int c) { return 1 + D + r * D - r * (r - 1) / 2 + (c - r); }   // (r <= c)
// bytes of LDS the solve takes: L [D][D + 1] (the pad keeps a column walk off one bank), y, delta and g [D] each
__host__ __device__ constexpr size_t glm_newton_solve_lds(int D) { return sizeof(double) * ((size_t)D * (D + 1) + 3 * (size_t)D); }

// THE TILE SCHEDULE.  NT = ceil(D / 16) column tiles; the NH = NT (NT + 1) / 2 tiles on and above the diagonal of the Hessian, row by
// row, then NT gradient tiles (the residuals as a sixteenth of an operand against the same columns); tile q goes to wave q % 4
template <int NT>
struct CurvTiles {
    static constexpr int NH = NT * (NT + 1) / 2;
    static constexpr int NQ = NH + NT;
    static constexpr int PER = (NQ + 3) / 4;   // accumulators a wave holds (D = 128: 11, 88 registers)
    static constexpr int tr(int q) {
        int r = 0;
        while (q >= NT - r) { q -= NT - r; ++r; }
        return r;
    }
    static constexpr int tc(int q) {
        int r = 0;
        while (q >= NT - r) { q -= NT - r; ++r; }
        return r + q;
    }
};

#pragma clang fp contract(off)
// one row at the double eta: its term l, the residual y - mu and the weight w
template <int FAM>
__device__ __forceinline__ void glm_curv_row(double eta, double y, double &l, double &resid, double &w) {
    if (!(fabs(eta) <= 1.79769313486231570e308)) {
        l = resid = w = __builtin_nan("");
        return;
    }
    if constexpr (FAM == GLM_LOGISTIC) {
        const double s = (1.0 - 2.0 * y) * eta;   // (exact for y in {0, 1})
        l = -(fmax(s, 0.0) + log1p(exp(-fabs(s))));
        const double t = exp(-fabs(eta));
        const double big = 1.0 / (1.0 + t), small = t / (1.0 + t);   // (mu and 1 - mu, the larger first)
        resid = y - (eta >= 0.0 ? big : small);
        w = big * small;
    } else {
        const double m = exp(eta);
        l = y * eta - m;
        resid = y - m;
        w = m;
    }
}
#pragma clang fp contract(fast)

// nnest_glm_newton.hip.  G, the row groups of n rows: one per block of 64 rows up to GLMNW_MAX_GROUPS.  A function of (n, D) alone
// -- not of the device: the same call gives the same bits on any part
int glm_curv_groups(int n, int D);
// out [1 + D + D D], partials [G][glm_curv_slots(D)]
hipError_t launch_glm_curv(const GlmSpec &gl, const double *theta, double *out, double *partials, hipStream_t st);
// prior NULL: none.  step [D], chol [D D], info [4]
hipError_t launch_glm_newton_solve(const double *curv, const GaussPriorSpec *prior, const double *theta, double *step, double *chol,
                                   double *info, int D, hipStream_t st);

}  // namespace nnest
