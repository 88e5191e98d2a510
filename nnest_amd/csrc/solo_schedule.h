// solo_schedule.h -- the barrier schedule of mh_kernel_solo (nnest_solo.hip), stated once.
//
// A workgroup of the solo form is three roles around ONE workgroup barrier: the net waves (a walker each), the noise wave and the
// relay wave.  A role that takes one barrier more or fewer than the others hangs its workgroup, so the step ranges of the three
// loops and the number of barriers each role takes are functions of (S, warm, dynamic, exact_all) here, the loops take their bounds
// from them, and a host program (tests/test_solo_schedule.py) holds the counts against each other before anything is launched.
//
// The order of barriers, the same for every role that takes part:
//   P0                            buffer 0 (the noise and scale of step 1) is published
//   P1                            buffer 1 (S >= 1)
//   A_k, P_{k+1}, B_k             k = 1 .. warm: an exact step (the batch rule's warm-up; every step but the last under lag 0)
//   P_k                           k = first lagged fetch .. S: a lagged (or fixed-step) step fetches buffer k
//   F                             exact_all (lag 0) only: the relay reads the LAST step's accepts behind it
// A wave that has ended no longer counts at s_barrier: the noise wave ends in front of F, and without the batch rule the relay wave
// ends in front of P0.  Plain C++ (no device types): the host program includes this file as it is.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SOLO_SCHED_FN __host__ __device__ constexpr
#else
#define SOLO_SCHED_FN constexpr
#endif

namespace nnest {

// the exact steps of a launch: flag_warm is the caller's NNEST_MH_WARM; lag 0 makes every step exact; at most S - 1 (step S has no
// successor to evaluate twice), none without the batch rule
SOLO_SCHED_FN int solo_warm_steps(int S, int flag_warm, bool dynamic, bool exact_all) {
    return dynamic ? ((exact_all ? S : flag_warm) < S - 1 ? (exact_all ? S : flag_warm) : S - 1) : 0;
}
// Steps 1 .. warm are exact steps.  Step warm + 1 (warm > 0) takes the candidate chosen at B_warm: it has neither a proposal nor a
// fetch of its own.  The steps that propose, fetch, finish and apply straight through (the lagged loop) start here:
SOLO_SCHED_FN int solo_first_straight_step(int warm) { return warm > 0 ? warm + 2 : 1; }
// ... and the first of them whose fetch is a barrier of the P_k row above (step 1's fetch is P1)
SOLO_SCHED_FN int solo_first_lagged_fetch(int warm) { return warm > 0 ? warm + 2 : 2; }
SOLO_SCHED_FN int solo_lagged_fetches(int S, int warm) { return S >= solo_first_lagged_fetch(warm) ? S - solo_first_lagged_fetch(warm) + 1 : 0; }
// the relay's first iteration of its lagged loop (an iteration = one barrier): without a warm-up its iterations 0 and 1 are P0, P1
SOLO_SCHED_FN int solo_relay_first_iteration(int warm) { return warm > 0 ? warm + 2 : 0; }

// ---- barriers per role, each written from that role's own loops ----
// net wave: the first fetch; then with a warm-up step 1's fetch, three per exact step and one per straight step -- without one a
// fetch per step; F
SOLO_SCHED_FN int solo_net_barriers(int S, int warm, bool dynamic, bool exact_all) {
    int n = 1;
    if (warm > 0) n += 1 + 3 * warm;
    const int first = solo_first_straight_step(warm);
    n += S >= first ? S - first + 1 : 0;
    return n + (exact_all ? 1 : 0);
}
// noise wave: P0, P1, three per exact step, the lagged fetches; ends in front of F
SOLO_SCHED_FN int solo_noise_barriers(int S, int warm, bool dynamic, bool exact_all) {
    int n = 1;
    if (S >= 1) n += 1 + 3 * warm + solo_lagged_fetches(S, warm);
    return n;
}
// relay wave (batch rule only): with a warm-up P0, P1 and three per exact step; an iteration of its lagged loop per barrier; F
SOLO_SCHED_FN int solo_relay_barriers(int S, int warm, bool dynamic, bool exact_all) {
    if (!dynamic) return 0;
    int n = warm > 0 ? 2 + 3 * warm : 0;
    const int k0 = solo_relay_first_iteration(warm);
    n += S >= k0 ? S - k0 + 1 : 0;
    return n + (exact_all ? 1 : 0);
}
// what a role's count must be for the workgroup to get through: the net waves' count, less the barriers behind the role's end
SOLO_SCHED_FN int solo_noise_barriers_due(int S, int warm, bool dynamic, bool exact_all) {
    return solo_net_barriers(S, warm, dynamic, exact_all) - (exact_all ? 1 : 0);
}
SOLO_SCHED_FN int solo_relay_barriers_due(int S, int warm, bool dynamic, bool exact_all) {
    return dynamic ? solo_net_barriers(S, warm, dynamic, exact_all) : 0;
}

}  // namespace nnest
