// slice_walk.h -- the bracket rule of ONE update of the slice proposal in latent space, stated once for every kernel that runs it
// (nnest_spline_slice.hip slice_body, nnest_slice_rounds.hip; nnest_solo.hip slice_kernel_solo restates it as nested loops).
// BUILD-DEFINED, parity unpinned: the reference proposes random-walk Metropolis moves only (nnest/sampler.py:310-316); the tests hold
// this to a CPU restatement that is a loop form on purpose (tests/test_slice_walk.py).
//
// Along a direction the candidates are z + t * width * eps; inside(t) is the caller's (box, slice level, likelihood).  With the
// uniforms u_k = draw(k) of the update (the kernels: noise_uniform(seed, walker, 64 it + k)):
//   bracket [t_l, t_r] = [-u_0, 1 - u_0];  stepping out (Neal 2003, sec. 4.1) within a budget of B = 2 max_out expansions: while
//   inside(t_l): t_l -= 1, then while inside(t_r): t_r += 1 -- the full step-out.  If it takes more than B expansions, the bracket
//   restarts at [-u_0, 1 - u_0] and the budget is split at random by u_63: at most J = slice_split_left(u_63) steps to the left, then
//   at most B - J to the right.  Either way the bracket is found from the new point with the probability it had from the old, so the
//   update is reversible (separate caps per side were not, once they bound).  max_out = 0: no stepping out.
//   shrinkage: t = t_l + (t_r - t_l) u_k (k = 2, 3, ...); inside(t) -> the walker moves there; else the bracket's end on t's side
//   becomes t; after max_shrink draws the walker stays.
// As a state machine: one evaluation of inside(tc) per advance(), so walkers that share a wave need not stay in step.
//
// Plain C++17: no HIP header is needed, so the rule runs on the host too (tests/test_slice_walk.py).  Every floating-point
// expression is part of the definition (the outputs are compared bit for bit): none may be reassociated or contracted differently.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SLICE_WALK_FN __host__ __device__ __forceinline__
#else
#define SLICE_WALK_FN inline
#endif

namespace nnest {

// the split of the stepping-out budget B = 2 max_out from v = u_63: at most J = min(B, floor(v (B + 1))) expansions to the left and
// B - J to the right.  v is a 24-bit fraction m / 2^24, so J = (m (B + 1)) >> 24 exactly, in integers (a float32 product could round
// up to B + 1).
SLICE_WALK_FN int slice_split_left(float v, int max_out) {
    const uint64_t m = (uint64_t)(v * 16777216.0f);
    const int B = 2 * max_out, J = (int)((m * (uint64_t)(B + 1)) >> 24);
    return J < B ? J : B;
}

// the range of the rule's parameters at every entry point (max_shrink: the uniforms 2 .. 61 of an update; max_stepout: the split's
// integer product)
SLICE_WALK_FN bool slice_params_ok(int steps, int max_stepout, int max_shrink, float width) {
    return steps >= 0 && max_stepout >= 0 && max_stepout <= (1 << 24) && max_shrink >= 1 && max_shrink <= 60 && width > 0.f;
}

struct SliceWalk {
    int it;           // update (1-based; 0: none begun)
    int phase, k;     // phase 0 / 1: stepping out to the left / right (k steps taken); 2: shrinkage (k draws taken)
    int nl;           // < 0: the full step-out (at most 2 max_out expansions in all, k counts them over both sides);
                      // else the split step-out: at most nl steps left, 2 max_out - nl right
    float t0;         // -u_0: the bracket's start
    float tl, tr, tc; // bracket, the candidate to evaluate next

    template <class Draw>
    SLICE_WALK_FN float shrink_candidate(Draw &draw) const {
        const float uk = draw(2 + k);
        return __builtin_fmaf(tr - tl, uk, tl);
    }

    // the next update: bracket and first candidate (draw sees the new `it`)
    template <class Draw>
    SLICE_WALK_FN void begin(Draw draw, int max_out) {
        it += 1;
        const float u0 = draw(0);
        t0 = -u0;
        tl = t0;
        tr = 1.0f - u0;
        k = 0;
        nl = -1;
        phase = max_out > 0 ? 0 : 2;
        tc = phase == 0 ? tl : shrink_candidate(draw);
    }

    // the full step-out took more than 2 max_out expansions: restart from [-u_0, 1 - u_0] with the budget split at random
    template <class Draw>
    SLICE_WALK_FN void split_stepout(Draw &draw, int max_out) {
        tl = t0;
        tr = 1.0f + t0;
        k = 0;
        nl = slice_split_left(draw(63), max_out);
        phase = nl > 0 ? 0 : (nl < 2 * max_out ? 1 : 2);
        tc = phase == 0 ? tl : phase == 1 ? tr : shrink_candidate(draw);
    }

    // ins = inside(tc).  Returns true when the update has ended: the walker moved to tc if `ins`, else it stays; otherwise tc is
    // the next candidate.
    template <class Draw>
    SLICE_WALK_FN bool advance(bool ins, Draw draw, int max_out, int max_shrink) {
        if (phase == 0 && nl < 0) {          // full: while inside(t_l): t_l -= 1 (more than 2 max_out expansions: split)
            if (ins) { tl -= 1.0f; k += 1; }
            if (!ins) { phase = 1; tc = tr; }
            else if (k <= 2 * max_out) tc = tl;
            else split_stepout(draw, max_out);
        } else if (phase == 1 && nl < 0) {   // full: the same to the right, k counting on
            if (ins) { tr += 1.0f; k += 1; }
            if (!ins) { phase = 2; k = 0; tc = shrink_candidate(draw); }
            else if (k <= 2 * max_out) tc = tr;
            else split_stepout(draw, max_out);
        } else if (phase == 0) {             // split: for j < nl: if !inside(t_l) break; t_l -= 1
            if (ins) { tl -= 1.0f; k += 1; }
            if (ins && k < nl) tc = tl;
            else if (nl < 2 * max_out) { phase = 1; k = 0; tc = tr; }
            else { phase = 2; k = 0; tc = shrink_candidate(draw); }
        } else if (phase == 1) {             // split: for j < 2 max_out - nl: the same to the right
            if (ins) { tr += 1.0f; k += 1; }
            if (ins && k < 2 * max_out - nl) tc = tr;
            else { phase = 2; k = 0; tc = shrink_candidate(draw); }
        } else if (ins) {                    // shrinkage: the walker moves to the candidate
            return true;
        } else {                             // the bracket's end on the candidate's side becomes the candidate
            if (tc < 0.f) tl = tc; else tr = tc;
            k += 1;
            if (k < max_shrink) tc = shrink_candidate(draw);
            else return true;                // after max_shrink draws the walker stays
        }
        return false;
    }
};

}  // namespace nnest
