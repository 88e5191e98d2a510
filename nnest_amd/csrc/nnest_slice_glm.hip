// nnest_slice_glm.hip -- the SLICE proposal in latent space of the trained NVP on a GENERALISED LINEAR MODEL of the user's data
// (logistic or Poisson regression): nnest_slice_steps's update (nnest_solo.hip slice_kernel_solo has the definition: directions,
// Philox uniforms, slice level, bracket rule -- slice_walk.h --, counters, NNEST_MH_ALL_MOVED) with
//   logL(x) := GLM(T(x)),  T(x)_d = ens_T(x_d, t_std[d], t_mean[d])  (SoloBox::map; NULL t_std / t_mean: the identity)
// and the likelihood of glm_data.h (float32 eta in the solo layout's order, float64 terms, rows >= n masked, the safe rule -1e100) in
// place of the analytic likelihoods.  include/nnest_hip.h nnest_slice_glm_steps; DESIGN.md 3.22.  BUILD-DEFINED.
// The box is on x (!(x < -1 || x > 1), a NaN coordinate inside), as in slice_kernel_solo -- NOT on T(x): the map gets no lo / hi.
//
// Layout: mcmc_glm_kernel's, the solo layout, one walker per wave, four walkers per workgroup; the flow half is solo_latent.h's
// SoloFlow, T is SoloBox::map, in front of glm_solo_loglike (data rows over the wave's 64 lanes).  One walker per wave and no step-size
// rule: no wave waits for another behind the staging barrier, any C is a legal grid.
//
// THE LIKELIHOOD IS SKIPPED where no decision depends on it: a candidate with pre == false (outside the box, or below the slice
// level) cannot lie in the slice, and its logL is never read -- not by the bracket rule (inside = pre && logL > L*), not by the
// move (only a candidate inside the slice is moved to), not by a counter (n_eval counts every candidate, n_call those with pre).
// `pre` is the same on all 64 lanes: the box's verdict is a ballot over the wave, and the log-det is the wave's total, read from
// lane 0 into a scalar register -- every lane of the wave holds that same total (solo_logdet_total), the readfirstlane only tells
// the compiler so.  So the skip is a scalar branch around glm_solo_loglike, whose readlanes and butterfly always see the whole wave.
// The update loop is slice_kernel_solo's nested loops, not the state machine of slice_walk.h: one walker per wave needs none, and
// the state machine's registers are the likelihood's here (profiles/slice_glm/resources.txt).
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "glm_data.h"
#include "nnest_internal.h"
#include "slice_glm.h"
#include "solo_latent.h"

namespace nnest {

template <int U, int FAM>
__global__ void __launch_bounds__(256) slice_glm_kernel(FlowShape s, const float *__restrict__ packed, SliceGlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    __shared__ __attribute__((aligned(16))) float x0buf[4][16][2 * U];   // the chains' first x (the usable-chain test at the end)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, S = a.steps, C = a.C;
    SoloFlow<U>::stage(wlds, s, packed, lane, wave);
    __syncthreads();
    const int pos = lane & 15;
    const bool writer_lane = lane < 16;
    const int row = blockIdx.x * 4 + wave;
    if (row >= C) return;   // (no barrier behind this point)
    SoloFlow<U> flow;
    flow.init(wlds, s, lane);
    SoloBox<U, NNEST_LIKE_GAUSSIAN> box;   // (T alone: lo / hi are NULL, its likelihood is not called)
    box.init(a, D, lane, pos);
    const double loglstar = a.loglstar;
    // x <- f^-1(x) in place; the walker's log-det as a scalar (the same bits on every lane: see the top)
    auto inverse = [&](float (&xs)[2][U]) -> float {
        const float ld = solo_logdet_total(flow.inverse(xs));
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ld)));
    };
    auto store_row = [&](float *base, size_t r, const float (&v)[2][U]) { solo_store_row<U>(base + r * D, D, pos, v); };

    float z[2][U], x[2][U];
    solo_load_row<U>(a.z + (size_t)row * D, D, pos, z);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c][u] = z[c][u];
    float ld = inverse(x);
    double logl = a.logl[row];
    if (writer_lane && a.x) {   // the chain's first x waits in LDS (usable-chain test at the end, nested.py:432; a lane reads back its own)
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) x0buf[wave][pos][2 * u + c] = x[c][u];
    }
    if (writer_lane && a.hist_x) store_row(a.hist_x, (size_t)row * (S + 1), x);
    const uint64_t walker = a.walker_offset + (uint64_t)row;
    int n_call = 0, n_move = 0, n_eval = 0;
    float zc[2][U], xc[2][U], ldc = 0.f;
    double lc = 0.0;
#pragma unroll 1
    for (int it = 1; it <= S; ++it) {
        float e[2][U];
        if (a.noise_dz) {
            solo_load_row<U>(a.noise_dz + ((size_t)(it - 1) * C + row) * D, D, pos, e);
        } else {
            solo_lane_normals<U>(pos, [&](uint32_t g) { return noise_normal4(a.seed, walker, (uint32_t)it, g, NOISE_STREAM_DZ); }, e);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) e[c][u] = box.live[c][u] ? e[c][u] : 0.f;   // (padded dims stay 0)
        }
        const float u0 = noise_uniform(a.seed, walker, 64u * (uint32_t)it + 0u), u1 = noise_uniform(a.seed, walker, 64u * (uint32_t)it + 1u);
        const float logy = ld + __logf(u1);   // (u1 = 0: -inf, the whole feasible line is the slice)
        // one evaluation: candidate t -> (zc, xc, ldc, lc); true if it lies in the slice
        auto inside = [&](float t) -> bool {
            const float tw = t * a.width;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) { zc[c][u] = __builtin_fmaf(e[c][u], tw, z[c][u]); xc[c][u] = zc[c][u]; }
            ldc = inverse(xc);
            int okl = 1;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int u = 0; u < U; ++u) okl &= !(xc[c][u] < -1.f || xc[c][u] > 1.f);   // UniformPrior(D, -1, 1): priors.py:39-43
            const bool inb = __ballot(okl != 0) == ~0ull;
            const bool pre = inb && (ldc > logy);   // (scalar: a ballot and two scalar floats)
            n_eval += 1;
            n_call += pre ? 1 : 0;
            if (!pre) return false;   // the likelihood is skipped: its value decides nothing (see the top)
            float tx[2][U];
            box.map(xc, tx);
            lc = glm_solo_loglike<U, FAM>(a.gl, lane, tx);
            return lc > loglstar;
        };
        // (slice_walk.h's rule as nested loops, as slice_kernel_solo restates it)
        float tl = -u0, tr = 1.0f - u0;
        if (a.max_out > 0) {
            const int B = 2 * a.max_out;
            int n = 0;   // expansions of the full step-out; more than B: the split step-out instead
            while (n <= B && inside(tl)) { tl -= 1.0f; n += 1; }
            while (n <= B && inside(tr)) { tr += 1.0f; n += 1; }
            if (n > B) {
                tl = -u0;
                tr = 1.0f - u0;
                const int nl = slice_stepout_left(a.seed, walker, (uint32_t)it, a.max_out);
                for (int j = 0; j < nl; ++j) { if (!inside(tl)) break; tl -= 1.0f; }
                for (int j = 0; j < B - nl; ++j) { if (!inside(tr)) break; tr += 1.0f; }
            }
        }
        bool moved = false;
        for (int k = 0; k < a.max_shrink; ++k) {
            const float uk = noise_uniform(a.seed, walker, 64u * (uint32_t)it + 2u + (uint32_t)k);
            const float t = __builtin_fmaf(tr - tl, uk, tl);
            if (inside(t)) { moved = true; break; }
            if (t < 0.f) tl = t; else tr = t;
        }
        if (moved) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int u = 0; u < U; ++u) { z[c][u] = zc[c][u]; x[c][u] = xc[c][u]; }
            ld = ldc; logl = lc; n_move += 1;
        }
        if (writer_lane && a.hist_x) store_row(a.hist_x, (size_t)row * (S + 1) + it, x);
    }
    bool all_moved = n_move > 0;
    if (a.x) {
        bool mine = true;
        if (writer_lane) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int d = 2 * U * pos + 2 * u + c;
                    const float x0 = x0buf[wave][pos][2 * u + c];
                    mine = mine && (d >= D || x[c][u] != x0);
                }
        }
        all_moved = (__ballot(mine) & 0xffffull) == 0xffffull;
    }
    if (writer_lane) {
        store_row(a.z, (size_t)row, z);
        if (a.x) store_row(a.x, (size_t)row, x);
        if (pos == 0) {
            a.logl[row] = logl;
            if (a.n_call) a.n_call[row] = n_call;
            if (a.n_move) a.n_move[row] = n_move | (all_moved ? NNEST_MH_ALL_MOVED : 0);
            if (a.n_eval) a.n_eval[row] = n_eval;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
template <int U, int FAM>
static hipError_t slice_glm_launch_k(const FlowShape &s, const float *packed, const SliceGlmArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((slice_glm_kernel<U, FAM>), dim3((a.C + 3) / 4), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

template <int FAM>
static hipError_t slice_glm_launch_f(const FlowShape &s, const float *packed, const SliceGlmArgs &a, hipStream_t st) {
    return solo_for_U(s.NT, [&](auto sh) { return slice_glm_launch_k<decltype(sh)::U, FAM>(s, packed, a, st); });
}

hipError_t launch_slice_glm(const FlowShape &s, const float *packed, const SliceGlmArgs &a, hipStream_t st) {
    if (!slice_form_eligible(s)) return hipErrorInvalidConfiguration;
    if (a.C <= 0) return hipSuccess;
    switch (a.gl.family) {
        case GLM_LOGISTIC: return slice_glm_launch_f<GLM_LOGISTIC>(s, packed, a, st);
        case GLM_POISSON: return slice_glm_launch_f<GLM_POISSON>(s, packed, a, st);
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
