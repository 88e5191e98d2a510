// importance_walk.h -- what the two kernels of the importance-sampled evidence share (include/nnest_hip.h nnest_importance_evidence;
// nnest_importance.hip: the NVP's one-sample-per-wave kernel, the draws' export and the second reduction stage;
// nnest_spline_importance.hip: the spline flow's tile kernel): the draws, the base density, the running sums and their merge, the
// arguments and the launchers' declarations.  The target's pieces -- ens_T, ens_target -- are the ensemble sampler's
// (ensemble_common.h): lp(z) here IS nnest_mcmc_steps's target.  One definition of each: a sample is a function of (seed, global
// sample index), not of its layout, because both kernels and the export compute with these.
#pragma once
#include "ensemble_common.h"
#include "flow_tile.h"
#include "nnest_internal.h"

namespace nnest {

enum { NOISE_STREAM_IMPORTANCE = 7 };
constexpr int IMP_NVP_TILE = 4, IMP_SPLINE_TILE = 16;   // samples per workgroup and pass of the persistent loop
constexpr int IMP_NVP_GROUPS_PER_CU = 4, IMP_SPLINE_GROUPS_PER_CU = 2;

// the four normals of dims 4g .. 4g+3 of sample m (step 0 of the stream): the Box-Muller arithmetic of mcmc_normal4
__device__ __forceinline__ f32x4 importance_normal4(uint64_t seed, uint64_t m, uint32_t g) {
    return noise_normal4(seed, m, 0u, g, (uint32_t)NOISE_STREAM_IMPORTANCE);
}

#pragma clang fp contract(off)
// the base's log density from sum z_d^2 (float64 of the float32 z): N(0, I)
__device__ __forceinline__ double importance_logb(double zz, int D) { return -0.5 * zz - (double)D * 0.91893853320467274178; }

// a running (a, S1, S2, n): a = max logw of the live samples, S1 = sum e^(logw - a), S2 = sum e^(2 (logw - a))
struct ImpSums { double a, s1, s2, n; };
__device__ __forceinline__ ImpSums importance_empty() { return ImpSums{-INFINITY, 0.0, 0.0, 0.0}; }
// one sample more (`counted`: a row of the launch; a dead sample -- logw NaN or -inf -- has weight 0)
__device__ __forceinline__ void importance_add(ImpSums &r, double logw, bool counted) {
    const bool live = counted && !(logw != logw) && logw != -INFINITY;
    if (!live) return;
    if (logw > r.a) {
        const double e = exp(r.a - logw);   // (a = -inf: 0)
        r.s1 = r.s1 * e + 1.0;
        r.s2 = r.s2 * (e * e) + 1.0;
        r.a = logw;
    } else {
        const double e = exp(logw - r.a);
        r.s1 += e;
        r.s2 += e * e;
    }
    r.n += 1.0;
}
// the sums of two sets of samples.  Symmetric in its arguments, operation by operation: both sides of an exchange hold the same bits
__device__ __forceinline__ ImpSums importance_merge(const ImpSums &p, const ImpSums &q) {
    ImpSums r;
    r.a = p.a > q.a ? p.a : q.a;
    const double ep = p.a == r.a ? 1.0 : exp(p.a - r.a), eq = q.a == r.a ? 1.0 : exp(q.a - r.a);   // (-inf beside -inf: 1, on sums of 0)
    r.s1 = p.s1 * ep + q.s1 * eq;
    r.s2 = p.s2 * (ep * ep) + q.s2 * (eq * eq);
    r.n = p.n + q.n;
    return r;
}
#pragma clang fp contract(fast)

// a workgroup's sums leave through here, called by ONE thread: the triple into its slot of partials, the count onto the launch's
// integer counter (sums[3] holds an integer until importance_combine_kernel has read it: integer addition has no order)
__device__ __forceinline__ void importance_publish(double *partials, double *sums, int group, const ImpSums &r) {
    partials[3 * group] = r.a;
    partials[3 * group + 1] = r.s1;
    partials[3 * group + 2] = r.s2;
    if (r.n != 0.0) atomicAdd(reinterpret_cast<unsigned long long *>(sums + 3), (unsigned long long)r.n);
}

// the arguments of a launch (nnest_importance_evidence, nnest_spline_importance_evidence).  The flow goes with them: FlowShape +
// packed weights for the NVP, SplArgs for the spline
struct ImpArgs {
    LikeSpec like;                  // scale 1: the likelihood sees T(x)
    const float *t_std, *t_mean;    // [D], or NULL: T = identity (x * 1 + 0 in float32)
    const float *lo, *hi;           // the prior box on T(x) [D], or NULL (no prior)
    float *z_out, *x_out;           // [M][D], or NULL: the sums only
    double *logl_out, *logw_out;    // [M]
    double *partials;               // [3 groups]
    double *sums;                   // [4]
    int M, groups;
    uint64_t seed, sample_offset;
};

// nnest_abi.hip: the argument checks both entries share (sets the error string); fills `a` but a.like and a.groups
int importance_args(ImpArgs *a, const float *t_std, const float *t_mean, const float *lo, const float *hi, float *z_out, float *x_out,
                    double *logl_out, double *logw_out, double *partials, double *sums, int M, uint64_t seed, uint64_t sample_offset);
int importance_groups(int M, int tile, int num_cu);   // nnest_importance.hip
hipError_t launch_importance_fill_noise(float *z, int M, int D, uint64_t seed, uint64_t sample_offset, hipStream_t st);
// zeroes the counter in front of the first stage / combines the partials in index order behind it (groups = 0: the empty sums)
hipError_t launch_importance_begin(double *sums, hipStream_t st);
hipError_t launch_importance_combine(const double *partials, double *sums, int groups, hipStream_t st);
hipError_t launch_importance(const FlowShape &s, const float *packed, const ImpArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for
hipError_t launch_spline_importance(const SplArgs &q, const ImpArgs &a, hipStream_t st);

}  // namespace nnest
