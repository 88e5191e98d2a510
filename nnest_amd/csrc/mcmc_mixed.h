// mcmc_mixed.h -- what the two kernels of the MIXED walk share (include/nnest_hip.h nnest_mcmc_mixed_steps; nnest_mcmc_mixed.hip: the
// NVP's one-walker-per-wave kernel; nnest_spline_mcmc_mixed.hip: the spline flow's tile kernel): random-walk Metropolis steps
// (mcmc_walk.h's, unchanged) with a flow-INDEPENDENCE ("global") step at every global_every-th step of the run -- the proposal is a
// draw of the flow's base, accepted on the ratio of importance weights.  The draws are mcmc_walk.h's (a draw at (walker, step) is
// used by exactly one kind of step), the tempered target is mcmc_target_tempered, the base density is importance_walk.h's: here are
// the schedule, the weight, the arguments and the launchers' declarations.  DESIGN.md 3.13.
#pragma once
#include "importance_walk.h"
#include "mcmc_walk.h"

namespace nnest {

// The schedule: step t (global index) is a global step iff k = global_every > 0 and (t + 1) % k == 0.  Kept as the phase t % k,
// advanced by one per step: no division in the step loop.  Uniform over the launch: every walker takes the same kind of step.
struct MixedPhase {
    uint32_t k, ph;   // ph = t % k of the step about to be taken (k = 0: never global)
    __device__ __forceinline__ void init(uint32_t step0, int global_every) {
        k = global_every > 0 ? (uint32_t)global_every : 0u;
        ph = k ? step0 % k : 0u;
    }
    // the kind of the step about to be taken; moves on to the next step
    __device__ __forceinline__ bool next_is_global() {
        if (k == 0u) return false;
        const bool g = ph + 1u == k;
        ph = g ? 0u : ph + 1u;
        return g;
    }
};

#pragma clang fp contract(off)
// the log importance weight of a row from its lp and its float64 sum of squares: lw = lp - logb(zz), one rounded subtraction
__device__ __forceinline__ double mixed_logw(double lp, double zz, int D) { return lp - importance_logb(zz, D); }
#pragma clang fp contract(fast)

// the arguments of a mixed launch: the tempered launch's, the schedule and the global steps' counter beside them.  A type of its
// own: the kernels of nnest_mcmc_steps and nnest_mcmc_tempered_steps keep the arguments -- and with them the code -- they had
struct McmcMixedArgs : McmcTemperedArgs {
    int global_every;               // k >= 0 (0: every step local)
    int *n_accept_global;           // [C] or NULL: the accepted global steps (n_accept counts both kinds)
};

hipError_t launch_mcmc_mixed(const FlowShape &s, const float *packed, const McmcMixedArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.C <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_mcmc_mixed(const SplArgs &q, const McmcMixedArgs &a, hipStream_t st);
// nnest_abi.hip: the check of a mixed entry's schedule (sets the error string)
int mcmc_mixed_every_ok(int global_every);

}  // namespace nnest
