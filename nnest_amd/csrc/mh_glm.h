// mh_glm.h -- the constrained METROPOLIS proposal (K4's hard-constraint step, mh_body.h; reference sampler.py:229-463) in latent space on
// a GENERALISED LINEAR MODEL of the user's data (include/nnest_hip.h nnest_mh_glm_steps, nnest_spline_mh_glm_steps):
// the arguments and the launchers' declarations of nnest_mh_glm.hip (the NVP's one-walker-per-wave kernel) and
// nnest_spline_mh_glm.hip (the spline flow's team tile).  The step is mh_body's with logL(x) = GLM(T(x)): T as SoloBox::map /
// spl_tile_map compute it, the likelihood glm_data.h's.  The box stays on x.
#pragma once
#include "glm_data.h"
#include "mh_common.h"
#include "nnest_internal.h"

namespace nnest {

// the K4 launch's fields that apply, with the descriptor and T beside them.  lo / hi: always NULL -- SoloBox::init and
// spl_tile_setup read them, and the box of this proposal is on x, not on T(x)
struct MhGlmArgs {
    float *z, *x;
    double *logl;
    double loglstar;
    float step_size;
    int steps, C, flags;
    LikeSpec like;              // (unused: SoloBox::init reads its scale)
    const float *noise_dz;      // recorded draws [steps][C][D] / [steps][C] (tests), both or neither
    const float *noise_u;
    uint64_t seed, walker_offset;
    float *hist_x;              // [C][steps + 1][D] or NULL
    double *hist_logl;          // [C][steps + 1] or NULL
    int *n_accept, *n_call;
    float *scale_out;           // one float per workgroup, or NULL
    float *x0;                  // the spline tile: the chains' first x (mh_first_x_buffer), for launch_mh_all_moved behind the launch
    unsigned long long *sync;   // the batch rule: mh_common.h's counters, zero at the launch
    int *sync_err;              // the word behind them: set where a bounded wait ran out
    GlmSpec gl;
    const float *t_std, *t_mean;   // [D] or both NULL: T = identity
    const float *lo, *hi;
};

// the three settings the flags word takes (everything else is an argument error): 0, the batch rule with a lag, and -- on the
// spline entry, `tile_rule` -- the rule per 16-walker tile
inline bool mh_glm_flags_ok(int flags, bool tile_rule) {
    if (flags == 0) return true;
    if ((flags & ~NNEST_MH_LAG(15)) == NNEST_MH_DYNAMIC_BATCH) return true;
    return tile_rule && flags == NNEST_MH_DYNAMIC_STEP;
}

// what the kernels do with a step's count: sampler.py:422-431, in double as mh_body does it
struct MhGlmVotes {
    int accept = 0, reject = 0;
    __device__ __forceinline__ void vote(double &scale, int num_accepted, int num_total) {
        if (2 * num_accepted > num_total) accept += 1; else reject += 1;
        if (accept > reject) scale *= exp(1.0 / (1 + accept));
        if (accept < reject) scale /= exp(1.0 / (1 + reject));
    }
};

// `max_grid` (both): where not NULL, nothing is launched and the grid the batch rule may span comes back -- the occupancy of the
// instantiation for this shape and family, with its dynamic LDS, times num_cu.  A launch under the batch rule whose grid is larger
// returns hipErrorLaunchOutOfResources and launches nothing.  hipErrorInvalidConfiguration: a shape that is not instantiated.
hipError_t launch_mh_glm(const FlowShape &s, const float *packed, const MhGlmArgs &a, int num_cu, int *max_grid, hipStream_t st);
hipError_t launch_spline_mh_glm(const SplArgs &q, const MhGlmArgs &a, int num_cu, int *max_grid, hipStream_t st);

}  // namespace nnest
