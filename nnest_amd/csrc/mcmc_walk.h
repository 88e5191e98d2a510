// mcmc_walk.h -- what the two kernels of the fused random-walk Metropolis run share (include/nnest_hip.h nnest_mcmc_steps;
// nnest_mcmc.hip: the NVP's one-walker-per-wave kernel and the draws' export; nnest_spline_mcmc.hip: the spline flow's tile kernel): the
// draws, the arguments and the launchers' declarations.  The target's pieces -- ens_T, ens_target, ens_accept_factor -- are the
// ensemble sampler's (ensemble_common.h): lp(z) here IS nnest_ensemble_steps's target at constrained = 0.  One definition of each
// draw: a run is a function of (seed, global walker index, global step), not of its layout, because both kernels and the export
// compute with these.
#pragma once
#include "ensemble_common.h"
#include "flow_tile.h"
#include "nnest_internal.h"

namespace nnest {

enum { NOISE_STREAM_MCMC = 5, NOISE_STREAM_MCMC_U = 6 };

// the four normals of dims 4g .. 4g+3 of (walker, step): noise_normal4 on the run's own stream
__device__ __forceinline__ f32x4 mcmc_normal4(uint64_t seed, uint64_t walker, uint32_t t, uint32_t g) {
    return noise_normal4(seed, walker, t, g, (uint32_t)NOISE_STREAM_MCMC);
}

// the accept draw of (walker, step): noise_uniform's sibling on stream NOISE_STREAM_MCMC_U (24 bits: exact in float32)
__device__ __forceinline__ float mcmc_uniform(uint64_t seed, uint64_t walker, uint32_t t) {
    u32x4 c;
    c.x = 0;
    c.y = (uint32_t)walker;
    c.z = t;
    c.w = ((uint32_t)(walker >> 32) & 0x0fffffffu) | ((uint32_t)NOISE_STREAM_MCMC_U << 28);
    const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(r.x >> 8) * 5.9604644775390625e-08f;
}

#pragma clang fp contract(off)
// q = z + step * eps, each operation rounded (as ens_propose is written)
__device__ __forceinline__ float mcmc_propose(float z, float step, float eps) { return z + step * eps; }
// the TEMPERED target (nnest_mcmc_tempered_steps): ens_target at constrained = 0 with the likelihood to the power beta,
// lp_beta = ((beta * logL) + log|det|) + prior, each operation rounded; beta = 1 is ens_target bit for bit (1.0 * logL is exact)
__device__ __forceinline__ double mcmc_target_tempered(double logl, float ld, bool in_prior, double beta) {
    const double prior = in_prior ? 0.0 : -INFINITY;
    return ((beta * logl) + (double)ld) + prior;
}
#pragma clang fp contract(fast)

// the arguments of a launch (nnest_mcmc_steps, nnest_spline_mcmc_steps).  The flow goes with them: FlowShape + packed weights for
// the NVP, SplArgs for the spline
struct McmcArgs {
    LikeSpec like;                  // scale 1: the likelihood sees T(x)
    const float *t_std, *t_mean;    // [D], or NULL: T = identity (x * 1 + 0 in float32)
    const float *lo, *hi;           // the prior box on T(x) [D], or NULL (no prior)
    const float *z_in;              // [C][D]
    const double *lp_in, *logl_in;  // [C], or NULL: evaluated
    float *z_out, *x_out;           // [C][D]
    double *lp_out, *logl_out;      // [C]
    float *hist_z, *hist_x;         // [C][S][D], or NULL: the ends only
    double *hist_logl;              // [C][S]
    int *n_accept;                  // [C] or NULL
    int C, S;
    float step;
    uint32_t step0;
    uint64_t seed, walker_offset;
};
// ... of a tempered launch (nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps): the likelihood's power beside them.  A type
// of its own, so that the untempered kernels keep the arguments -- and with them the code -- they had
struct McmcTemperedArgs : McmcArgs {
    double beta;                    // finite, >= 0 (0: the prior and the Jacobian alone)
};
// the arguments of an instantiation: TP selects the tempered target at compile time
template <bool TP> struct McmcArgsOf { typedef McmcArgs type; };
template <> struct McmcArgsOf<true> { typedef McmcTemperedArgs type; };

// nnest_abi.hip: the argument checks both entries share (sets the error string); fills `a` (a.like is the caller's, after its own
// likelihood check)
int mcmc_args(McmcArgs *a, const float *t_std, const float *t_mean, const float *lo, const float *hi, const float *z_in, const double *lp_in,
              const double *logl_in, float *z_out, float *x_out, double *lp_out, double *logl_out, float *hist_z, float *hist_x,
              double *hist_logl, int *n_accept, int C, int steps, float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset);
hipError_t launch_mcmc_fill_noise(float *dz, float *u, int S, int C, int D, uint32_t step0, uint64_t seed, uint64_t walker_offset,
                                  hipStream_t st);
hipError_t launch_mcmc(const FlowShape &s, const float *packed, const McmcArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for
hipError_t launch_spline_mcmc(const SplArgs &q, const McmcArgs &a, hipStream_t st);
// the tempered instantiations of the same two kernels (a.beta as the entry checked it: nnest_abi.hip mcmc_beta_ok)
hipError_t launch_mcmc_tempered(const FlowShape &s, const float *packed, const McmcTemperedArgs &a, hipStream_t st);
hipError_t launch_spline_mcmc_tempered(const SplArgs &q, const McmcTemperedArgs &a, hipStream_t st);
// nnest_abi.hip: the check of a tempered entry's beta (sets the error string)
int mcmc_beta_ok(double beta);

}  // namespace nnest
