// mcmc_adapt.h -- what the two kernels of the ADAPTIVE walk share (include/nnest_hip.h nnest_mcmc_adapt_steps; nnest_mcmc_adapt.hip:
// the NVP's one-walker-per-wave kernel; nnest_spline_mcmc_adapt.hip: the spline flow's tile kernel): the mixed walk (mcmc_mixed.h,
// unchanged) with the step of the local proposal a float64 `sigma` PER WALKER, moved by a Robbins-Monro rule on the walker's own
// binary decisions over the first adapt_steps steps of the run and frozen from there on.  The draws, the target, the schedule and
// the accept rule are the mixed walk's: here are the rule, the arguments and the launchers' declarations.  DESIGN.md 3.14.
#pragma once
#include "mcmc_mixed.h"

namespace nnest {

#pragma clang fp contract(off)
// the guards: sigma = min(max(sigma, MIN), MAX), written so that a NaN loads as MIN (NaN > MIN is false)
__device__ __forceinline__ double adapt_clamp(double sigma) {
    const double lo = sigma > NNEST_ADAPT_STEP_MIN ? sigma : NNEST_ADAPT_STEP_MIN;
    return lo < NNEST_ADAPT_STEP_MAX ? lo : NNEST_ADAPT_STEP_MAX;
}
// the update after the decision `acc` of the LOCAL step t < adapt_steps (the caller's conditions): float64, each operation rounded;
// the binary decision, no transcendental -- a numpy restatement gives the same bits
__device__ __forceinline__ double adapt_update(double sigma, uint32_t t, bool acc, double rate, double target) {
    const double g = rate / sqrt((double)t + 1.0);
    const double s = sigma * (1.0 + g * ((acc ? 1.0 : 0.0) - target));
    return adapt_clamp(s);
}
#pragma clang fp contract(fast)

// the arguments of an adaptive launch: the mixed launch's, the walkers' steps and the rule's parameters beside them.  A type of its
// own: the mixed kernels keep the arguments -- and with them the code -- they had
struct McmcAdaptArgs : McmcMixedArgs {
    const double *step_in;          // [C] or NULL: every walker starts at (double)step
    double *step_out;               // [C] or NULL (written iff S > 0)
    double *hist_step;              // [C][S] or NULL: sigma after each step
    uint32_t adapt_steps;           // steps t < adapt_steps adapt; the rest are frozen
    double adapt_rate;              // in [0, 1]
    double target_accept;           // in (0, 1)
};

hipError_t launch_mcmc_adapt(const FlowShape &s, const float *packed, const McmcAdaptArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.C <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_mcmc_adapt(const SplArgs &q, const McmcAdaptArgs &a, hipStream_t st);
// nnest_abi.hip: the check of an adaptive entry's rule (sets the error string)
int mcmc_adapt_rule_ok(double adapt_rate, double target_accept);

}  // namespace nnest
