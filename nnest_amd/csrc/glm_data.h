// glm_data.h -- the GENERALISED LINEAR MODEL LIKELIHOODS of the fused Metropolis runs (include/nnest_hip.h nnest_mcmc_glm_steps;
// nnest_mcmc_glm.hip: the NVP's one-walker-per-wave kernel and the likelihood alone; nnest_spline_mcmc_glm.hip: the spline flow's
// tile kernel): the adaptive walk (mcmc_adapt.h, unchanged) with the log-likelihood of a regression on the user's data,
//   logL(t) = logl0 + sum_{i < n} l_i,   eta_i = o_i + sum_c A[i, c] t_c,
//   logistic: l_i = -softplus((1 - 2 y_i) eta_i), y_i in {0, 1};   poisson: l_i = y_i eta_i - exp(eta_i), y_i >= 0,
// in place of the analytic likelihoods.  Here are the likelihood in both layouts, the arguments and the launchers' declarations.
// The arithmetic, with t = T(x) the float32 row:
//   eta_i = o_i + sum_c A[i, c] t_c    float32, fused multiply-adds, in the layout's own order
//   l_i                                float64 from (double)eta_i; softplus(s) = max(s, 0) + log1p(exp(-|s|)); NaN where eta_i is
//                                      not finite (so a non-finite coordinate of t poisons the sum whatever the signs)
//   logL = logl0 + sum_i l_i           float64, in a fixed order per entry; -1e100 where that is not finite (gdata_finish's rule)
// Rows i >= n are MASKED (softplus(0) = log 2: padding alone would count them), whatever the padded arrays hold there.
// The data are read from global memory through the caches: at [D, ld] = A^T, rows along the fast axis, ld = n rounded up to a
// multiple of 64, so that a wave's 64 rows of one column, and a tile's 16, are one run; y [ld], o [ld].  The family is a template
// parameter of every kernel.
#pragma once
#include "mcmc_adapt.h"
#include "solo_tile.h"

namespace nnest {

constexpr int GLM_LOGISTIC = 0, GLM_POISSON = 1;   // nnest_glm_t.family
constexpr int GLM_MAX_ROWS = 65536;

// the descriptor on the device side (nnest_glm_t, checked)
struct GlmSpec {
    const float *at;   // [D, ld]: A^T
    const float *y;    // [ld]
    const float *o;    // [ld]
    double logl0;
    int n, ld, D, family;
};

// the arguments of a launch: the adaptive launch's (its `like` unused), the descriptor beside them.  A type of its own: the
// adaptive kernels keep the arguments -- and with them the code -- they had
struct McmcGlmArgs : McmcAdaptArgs {
    GlmSpec gl;
};

#pragma clang fp contract(off)
// one row's term, float64 from the float32 linear predictor
template <int FAM>
__device__ __forceinline__ double glm_term(float eta, float y) {
    if (!(fabsf(eta) <= 3.40282346638528860e38f)) return __builtin_nan("");
    const double e = (double)eta;
    if constexpr (FAM == GLM_LOGISTIC) {
        const double s = (1.0 - 2.0 * (double)y) * e;   // (exact for y in {0, 1})
        return -(fmax(s, 0.0) + log1p(exp(-fabs(s))));
    } else {
        return (double)y * e - exp(e);
    }
}
// logL from the sum: the safe rule of solo_loglike / loglike_tile
__device__ __forceinline__ double glm_finish(double logl0, double sum) {
    double acc = logl0 + sum;
    if (!(fabs(acc) <= 1.79769313486231570e308)) acc = -1e100;
    return acc;
}
#pragma clang fp contract(fast)

// ---- the solo layout (solo_tile.h): lane = 16 g + p holds dims 2U p + 2u + c of the walker's row; the four 16-lane rows g hold
// copies.  ROWS OVER LANES: lane l of pass P owns data row 64 P + l, so the 64 lanes evaluate 64 distinct float64 terms (the four
// copies sharing rows, as the Gaussian sibling does, would compute each term 16 times).  t_c reaches the wave by v_readlane_b32
// from the lane (position c / 2U of copy 0) and register (c % 2U) that hold it -- the position is a loop counter in an SGPR, the
// register an unrolled index: no LDS, no barrier --, and one broadcast serves GLM_PASSES passes, whose loads at[c, 64 P + l] are
// independent coalesced runs.  Each lane adds its rows' terms in float64 in the order of P; a float64 butterfly over the 64 lanes
// (xor 1 .. 32) follows: addition commutes, so every lane of the wave ends with the same bits. ----
constexpr int GLM_PASSES = 4;
template <int U, int FAM>
__device__ __forceinline__ double glm_solo_loglike(const GlmSpec &gl, int lane, const float (&tx)[2][U]) {
    const int D = gl.D, n = gl.n;
    const size_t ld = (size_t)gl.ld;
    const int npass = (n + 63) >> 6;   // (64 npass <= ld: no read past the arrays)
    double sum = 0.0;
    // The loop over the columns has NO branch but its own: a pass past the last one reads the last one's rows again (cache hits;
    // its result is dropped), a column past D - 1 reads column D - 1 with t = 0 (x + 0 a = x) -- with a branch per pass hipcc waits
    // for every load before it issues the next, and the evaluation is one global-memory latency per product.
    for (int p0 = 0; p0 < npass; p0 += GLM_PASSES) {
        int off[GLM_PASSES];   // (the pass's first row relative to the group's, clamped to the last pass)
#pragma unroll
        for (int j = 0; j < GLM_PASSES; ++j) off[j] = 64 * (min(p0 + j, npass - 1) - p0);
        const int i0 = 64 * p0 + lane;
        float acc[GLM_PASSES];
#pragma unroll
        for (int j = 0; j < GLM_PASSES; ++j) acc[j] = gl.o[i0 + off[j]];
        const float *col = gl.at + i0;
        for (int pos = 0; 2 * U * pos < D; ++pos) {   // (uniform; at most 16 trips: 32 U >= D)
#pragma unroll
            for (int k = 0; k < 2 * U; ++k) {
                const int c = 2 * U * pos + k;
                const float tc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tx[k & 1][k >> 1]), pos));
                const float t = c < D ? tc : 0.f;
                const float *a = col + (size_t)min(c, D - 1) * ld;
#pragma unroll
                for (int j = 0; j < GLM_PASSES; ++j) acc[j] = fmaf(a[off[j]], t, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < GLM_PASSES; ++j) {
            const int i = i0 + 64 * j;
            const double l = glm_term<FAM>(acc[j], gl.y[i0 + off[j]]);
            sum += (p0 + j < npass && i < n) ? l : 0.0;   // (masked, not padded)
        }
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    sum += __shfl_xor(sum, 8);
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    return glm_finish(gl.logl0, sum);
}

// ---- the team tile (flow_tile.h, spline_latent.h): lane = 16 g + m holds, of walker m, the dims 32 tau + 8 g + j (j = 0 .. 7;
// class c = j & 1, component j >> 1 of tx[c][tau]).  eta^T = A t^T is an [n x D] [D x 16] product on the matrix cores, 16 rows of A
// to an accumulator, v_mfma_f32_16x16x4f32 (mfma4): K-step (tau, j) takes the four columns 32 tau + 8 k + j (k = 0 .. 3) -- lane
// (m, g) gives A[16 rb + m, 32 tau + 8 g + j] (from at: the 16 lanes m read one run) and t of walker m at that column, which it
// holds --, the accumulator starts from the offsets, and lane (m, g) ends with eta of rows 16 rb + 4 g + v (v = 0 .. 3) of walker
// m: four distinct (row, walker) pairs a lane, no float64 term twice in a wave.
// THE FOUR WAVES SHARE THE ROWS: wave w takes the row blocks rb = w, w + 4, ... (n >> D: the product and the terms would otherwise
// be done four times over), adds its terms in float64 in the order (rb, v), over its lane groups by group_sum, and writes one
// double per walker to part[w][m] in LDS; behind ONE __syncthreads() every wave adds the four partials in wave order, so the four
// waves hold the same bits.  `part`: [4][16] doubles; the caller alternates two such arrays between consecutive evaluations (see
// nnest_spline_mcmc_glm.hip for why that is enough).  Called by all 256 threads of the workgroup. ----
template <int NT, int FAM>
__device__ __forceinline__ double glm_tile_loglike(const GlmSpec &gl, int lane, int wv, const f32x4 (&tx)[2][NT], double *part) {
    const int D = gl.D, n = gl.n, m = lane & 15, g = lane >> 4;
    const size_t ld = (size_t)gl.ld;
    float b[NT][8];
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        b[tau][0] = tx[0][tau].x; b[tau][1] = tx[1][tau].x; b[tau][2] = tx[0][tau].y; b[tau][3] = tx[1][tau].y;
        b[tau][4] = tx[0][tau].z; b[tau][5] = tx[1][tau].z; b[tau][6] = tx[0][tau].w; b[tau][7] = tx[1][tau].w;
    }
    double s = 0.0;
    const int nrb = (n + 15) >> 4;   // (16 nrb <= ld: no read past the arrays)
    // RB of the wave's row blocks at a time (rb, rb + 4, ...: independent accumulators, their loads in flight together).  Two in
    // the narrowest tile only: measured between two builds, at x_dim 20 two are 2-3 % of the launch faster than one, at x_dim 50 (NT = 2)
    // 20 to 60 % slower -- the second set of operands goes to AGPRs and back.  The loads carry no branch: a column past D - 1 reads column D - 1 and is zeroed behind
    // the load, a row block past the last reads the wave's current one again and is dropped -- with a branch per load hipcc
    // waits for each column block's loads before it issues the next.
    constexpr int RB = NT == 1 ? 2 : 1;
    for (int rb = wv; rb < nrb; rb += 4 * RB) {   // (uniform: wv is the wave's number)
        f32x4 acc[RB];
        int i0[RB];
        bool live[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            live[q] = rb + 4 * q < nrb;   // (uniform)
            i0[q] = 16 * (live[q] ? rb + 4 * q : rb) + 4 * g;
            acc[q] = *reinterpret_cast<const f32x4 *>(gl.o + i0[q]);
        }
        float a[RB][NT][8];
#pragma unroll
        for (int q = 0; q < RB; ++q)
#pragma unroll
            for (int tau = 0; tau < NT; ++tau)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 32 * tau + 8 * g + j;
                    const float v = gl.at[(size_t)min(c, D - 1) * ld + (i0[q] - 4 * g) + m];   // (no read past [D, ld])
                    a[q][tau][j] = c < D ? v : 0.f;
                }
#pragma unroll
        for (int tau = 0; tau < NT; ++tau)
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int q = 0; q < RB; ++q) acc[q] = mfma4(a[q][tau][j], b[tau][j], acc[q]);
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const f32x4 yv = *reinterpret_cast<const f32x4 *>(gl.y + i0[q]);
            const double l0 = glm_term<FAM>(acc[q].x, yv.x), l1 = glm_term<FAM>(acc[q].y, yv.y);
            const double l2 = glm_term<FAM>(acc[q].z, yv.z), l3 = glm_term<FAM>(acc[q].w, yv.w);
            s += live[q] && i0[q] < n ? l0 : 0.0;   // (masked, not padded)
            s += live[q] && i0[q] + 1 < n ? l1 : 0.0;
            s += live[q] && i0[q] + 2 < n ? l2 : 0.0;
            s += live[q] && i0[q] + 3 < n ? l3 : 0.0;
        }
    }
    s = group_sum(s);
    if (lane < 16) part[16 * wv + m] = s;
    __syncthreads();
    const double tot = ((part[m] + part[16 + m]) + part[32 + m]) + part[48 + m];
    return glm_finish(gl.logl0, tot);
}

hipError_t launch_loglike_glm(const GlmSpec &gl, const float *t, double *logl, int N, hipStream_t st);
hipError_t launch_mcmc_glm(const FlowShape &s, const float *packed, const McmcGlmArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.C <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_mcmc_glm(const SplArgs &q, const McmcGlmArgs &a, hipStream_t st);
// nnest_abi.hip: the check of a descriptor against the flow's x_dim (sets the error string), and the descriptor checked
int glm_ok(const nnest_glm_t *glm, int D, GlmSpec *out);

}  // namespace nnest
