// slice_glm.h -- the SLICE proposal in latent space on a GENERALISED LINEAR MODEL of the user's data (include/nnest_hip.h
// nnest_slice_glm_steps, nnest_spline_slice_glm_steps): the arguments and the launchers' declarations of
// nnest_slice_glm.hip (the NVP's one-walker-per-wave kernel) and nnest_spline_slice_glm.hip (the spline flow's team tile).
// The definition is nnest_slice_steps's (nnest_solo.hip; slice_walk.h has the bracket rule) with logL(x) = GLM(T(x)): T as
// SoloBox::map / spl_tile_map compute it, the likelihood glm_data.h's.  The box stays on x.
#pragma once
#include "glm_data.h"
#include "mh_common.h"
#include "nnest_internal.h"

namespace nnest {

// the slice launch's arguments (their `like` unused) with the descriptor and T beside them.  lo / hi: always NULL -- SoloBox::init
// and spl_tile_setup read them, and the box of this proposal is on x, not on T(x)
struct SliceGlmArgs : SliceArgs {
    GlmSpec gl;
    const float *t_std, *t_mean;   // [D] or both NULL: T = identity
    const float *lo, *hi;
};

hipError_t launch_slice_glm(const FlowShape &s, const float *packed, const SliceGlmArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.C <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_slice_glm(const SplArgs &q, const SliceGlmArgs &a, hipStream_t st);

}  // namespace nnest
