// gauss_prior.h -- INDEPENDENT NORMAL PRIORS beside the regression likelihoods of glm_data.h in the fused Metropolis runs
// (include/nnest_hip.h nnest_mcmc_glm_prior_steps; nnest_mcmc_glm_prior.hip: the NVP's one-walker-per-wave kernel and the prior
// alone; nnest_spline_mcmc_glm_prior.hip: the spline flow's tile kernel): the adaptive walk of nnest_mcmc_glm_steps with
//   log pi(t) = logc - 1/2 sum_c ((t_c - m_c) r_c)^2,   r_c = 1 / sigma_c,   logc = -sum_c log sigma_c - (D / 2) log 2 pi,
// in the place of mcmc_target_tempered's 0.0.  Here are the descriptor, the prior term in both layouts, the arguments and the
// launchers' declarations.  The arithmetic, with t = T(x) the float32 row the likelihood sees:
//   u_c = (t_c - m_c) * r_c            float32, each operation rounded (contract off)
//   ss = sum_c (double)u_c (double)u_c float64, in the layout's own fixed order: the order of solo_row_zz / tile_row_zz
//   log pi = logc - 0.5 ss             float64; -inf where ss is not finite (a non-finite coordinate is refused, never NaN)
//   lp_beta = ((beta logL) + log|det|) + log pi    each operation rounded; -inf outside the box lo / hi, as in every sibling
// Padded dimensions carry m = 0, r = 0 under t = 0: u = 0.  glm_data.h is included, not edited.
#pragma once
#include "glm_data.h"

namespace nnest {

// the descriptor on the device side (nnest_gauss_prior_t, checked)
struct GaussPriorSpec {
    const float *m;   // [D]
    const float *r;   // [D]: float32(1 / sigma)
    double logc;
    int D;
};

// the arguments of a launch: the glm launch's, the prior's descriptor beside them.  A type of its own: the glm kernels keep the
// arguments -- and with them the code -- they had
struct McmcGlmPriorArgs : McmcGlmArgs {
    GaussPriorSpec pr;
};

#pragma clang fp contract(off)
__device__ __forceinline__ float gauss_prior_u(float t, float m, float r) { return (t - m) * r; }
// log pi from the sum of squares
__device__ __forceinline__ double gauss_prior_finish(double logc, double ss) {
    return fabs(ss) <= 1.79769313486231570e308 ? logc - 0.5 * ss : -INFINITY;
}
// mcmc_target_tempered (mcmc_walk.h) with log pi in place of its 0.0
__device__ __forceinline__ double mcmc_target_tempered_prior(double logl, float ld, bool in_box, double logpi, double beta) {
    const double prior = in_box ? logpi : -INFINITY;
    return ((beta * logl) + (double)ld) + prior;
}
#pragma clang fp contract(fast)

// ---- the solo layout (solo_tile.h): lane = 16 g + p holds dims 2U p + 2u + c of the row, and of m and r (pm, pr: loaded once a
// launch); the lane's 2U products in the order (u, c), then the four-step xor butterfly over the 16 positions: solo_row_zz's order ----
template <int U>
__device__ __forceinline__ double gauss_prior_solo(const float (&tx)[2][U], const float (&pm)[2][U], const float (&pr)[2][U], double logc) {
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float v = gauss_prior_u(tx[c][u], pm[c][u], pr[c][u]);
            ss += (double)v * (double)v;   // (the product of two float32 is exact in float64)
        }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    ss += __shfl_xor(ss, 4);
    ss += __shfl_xor(ss, 8);
    return gauss_prior_finish(logc, ss);
}
// m and r of the lane's dims (padded dims: 0, 0)
template <int U>
__device__ __forceinline__ void gauss_prior_solo_load(const GaussPriorSpec &p, int pos, float (&pm)[2][U], float (&pr)[2][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = 2 * U * pos + 2 * u + c;
            const bool v = d < p.D;
            pm[c][u] = v ? p.m[d] : 0.f;
            pr[c][u] = v ? p.r[d] : 0.f;
        }
}

// ---- the team tile (spline_latent.h): lane = 16 g + w holds, of walker w, the dims 32 tau + 8 g + j; ppar: [2][32 NT] floats in
// LDS -- m, r, padded dims 0 --, read as tpar is.  Every wave sums its own copy of the tile in full (group_sum over the walker's four
// lane groups), in tile_row_zz's order: the four waves hold the same bits without an exchange ----
// (class c of the lane's eight consecutive values: spline_latent.h's tile_class, restated -- this header serves the solo unit too)
__device__ __forceinline__ f32x4 gauss_prior_class(const f32x4 &v0, const f32x4 &v1, int c) {
    return c ? (f32x4){v0.y, v0.w, v1.y, v1.w} : (f32x4){v0.x, v0.z, v1.x, v1.z};
}
template <int NT>
__device__ __forceinline__ double gauss_prior_tile(const f32x4 (&tx)[2][NT], const float *ppar, int g, double logc) {
    double ss = 0.0;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(ppar + 32 * tau + 8 * g);
        constexpr int PW = 8 * NT;   // f32x4 per parameter
        const f32x4 m0 = p[0], m1 = p[1], r0 = p[PW], r1 = p[PW + 1];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 mu = gauss_prior_class(m0, m1, c), rr = gauss_prior_class(r0, r1, c), t = tx[c][tau];
            const float ux = gauss_prior_u(t.x, mu.x, rr.x), uy = gauss_prior_u(t.y, mu.y, rr.y);
            const float uz = gauss_prior_u(t.z, mu.z, rr.z), uw = gauss_prior_u(t.w, mu.w, rr.w);
            ss += (double)ux * (double)ux + (double)uy * (double)uy + (double)uz * (double)uz + (double)uw * (double)uw;
        }
    }
    return gauss_prior_finish(logc, group_sum(ss));
}

hipError_t launch_logprior_gauss(const GaussPriorSpec &p, const float *t, double *logp, int N, hipStream_t st);
hipError_t launch_mcmc_glm_prior(const FlowShape &s, const float *packed, const McmcGlmPriorArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.C <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_mcmc_glm_prior(const SplArgs &q, const McmcGlmPriorArgs &a, hipStream_t st);
// nnest_abi.hip: the check of a descriptor against D, `what` D is in the refusal (sets the error string), and the descriptor checked
int gauss_prior_ok(const nnest_gauss_prior_t *prior, int D, GaussPriorSpec *out, const char *what = "the flow's x_dim");

}  // namespace nnest
