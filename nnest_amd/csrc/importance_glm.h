// importance_glm.h -- what the two kernels of the IMPORTANCE-SAMPLED EVIDENCE OF A REGRESSION share (include/nnest_hip.h
// nnest_importance_glm_evidence; nnest_importance_glm.hip: the NVP's one-sample-per-wave kernel; nnest_spline_importance_glm.hip: the
// spline flow's tile kernel): the arguments of a launch and the launchers' declarations.  Everything else is included, not edited:
// the draws, the base density, the running sums, their merge and the second stage are importance_walk.h's, the likelihood is
// glm_data.h's, the prior gauss_prior.h's.  A sample is nnest_importance_evidence's in every respect but the target:
//   logw_m = lp(z_m) - logb(z_m),   lp = (logL(T(x)) + log|det|) + prior     float64, each operation rounded
//   prior: PRIOR = false: 0 inside the box lo / hi on T(x), -inf outside (ens_target);
//          PRIOR = true:  log pi(T(x)) of gauss_prior.h, no box (mcmc_target_tempered_prior at beta = 1: 1.0 * logL is exact).
#pragma once
#include "gauss_prior.h"
#include "importance_walk.h"

namespace nnest {

// the arguments of a launch: the importance launch's (its `like` unused), the descriptors beside them.  A type of its own: the
// importance kernels keep the arguments -- and with them the code -- they had
struct ImpGlmArgs : ImpArgs {
    GlmSpec gl;
    GaussPriorSpec pr;   // read by the PRIOR = true kernels only
    int prior;           // 0: the box (or nothing); 1: pr
};

hipError_t launch_importance_glm(const FlowShape &s, const float *packed, const ImpGlmArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.M <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_importance_glm(const SplArgs &q, const ImpGlmArgs &a, hipStream_t st);

}  // namespace nnest
