// nnest_importance_glm.hip -- IMPORTANCE-SAMPLED EVIDENCE of a GENERALISED LINEAR MODEL of the user's data from the trained flow:
// nnest_importance_evidence's estimate (nnest_importance.hip has the definition: draws, base density, weight, sums) with the
// regression likelihood of glm_data.h in place of the analytic ones and, optionally, the normal priors of gauss_prior.h in place of
// the box (include/nnest_hip.h nnest_importance_glm_evidence).  BUILD-DEFINED.
//
// Layout: importance_kernel's, the solo layout, one sample per wave, four waves a workgroup, a PERSISTENT grid: wave `wg` of the
// grid's `nw` takes samples wg, wg + nw, ...  That unit stays what it is: its body is restated here on the two halves of
// solo_latent.h, as nnest_mcmc_glm_prior.hip restates its sibling's.  The likelihood spreads the data rows over the wave's 64 lanes
// (glm_solo_loglike: v_readlane_b32 broadcasts, no LDS, no barrier); m and r of the prior sit in registers, loaded once a launch.
// There is no barrier inside the per-wave loop, so the waves of a workgroup may run different trip counts.
//
// Reduction: importance_kernel's -- a running (a, S1, S2, n) per wave, the four waves merged in wave order by one thread, which
// publishes the workgroup's partial; importance_combine_kernel merges the partials in index order.  No floating-point atomics.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "importance_glm.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

template <int U, int FAM, bool PRIOR>
__global__ void __launch_bounds__(256) importance_glm_kernel(FlowShape s, const float *__restrict__ packed, ImpGlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, M = a.M;
    SoloFlow<U>::stage(wlds, s, packed, lane, wave);
    __syncthreads();
    const int pos = lane & 15;
    SoloFlow<U> flow;
    flow.init(wlds, s, lane);
    SoloBox<U, NNEST_LIKE_GAUSSIAN> box;   // (T and the box; its likelihood is not called)
    box.init(a, D, lane, pos);
    float pm[2][U], pr[2][U];   // the prior's m and r of the lane's dims
    double logc = 0.0;
    if constexpr (PRIOR) {
        gauss_prior_solo_load<U>(a.pr, pos, pm, pr);
        logc = a.pr.logc;
    }
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](float (&xs)[2][U], double &logl) -> double {
        const float ld = solo_logdet_total(flow.inverse(xs));
        float tx[2][U];
        int ok = 1;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                tx[c][u] = ens_T(xs[c][u], box.sd[c][u], box.mu[c][u]);
                ok &= !(tx[c][u] < box.blo[c][u] || tx[c][u] > box.bhi[c][u]);   // (NaN counts as inside: UniformPrior, priors.py)
            }
        if constexpr (PRIOR) {
            const double logpi = gauss_prior_solo<U>(tx, pm, pr, logc);
            logl = glm_solo_loglike<U, FAM>(a.gl, lane, tx);
            return mcmc_target_tempered_prior(logl, ld, true, logpi, 1.0);   // (no box beside the prior: the entry refuses one)
        } else {
            const bool in_box = __ballot(ok != 0) == ~0ull;
            logl = glm_solo_loglike<U, FAM>(a.gl, lane, tx);
            return ens_target(logl, ld, in_box, 0, 0.0);
        }
    };

    const bool writer_lane = lane < 16;
    auto store_row = [&](float *base, const float (&v)[2][U]) { solo_store_row<U>(base, D, pos, v); };
    const bool outs = a.z_out != nullptr;
    const int nw = (int)gridDim.x * 4, wg = (int)blockIdx.x * 4 + wave;

    ImpSums run = importance_empty();
#pragma unroll 1
    for (int k = wg; k < M; k += nw) {   // (M <= 2^30: k + nw stays inside int)
        const uint64_t m = a.sample_offset + (uint64_t)k;
        float e[2][U], z[2][U], x[2][U];
        solo_lane_normals<U>(pos, [&](uint32_t g) { return importance_normal4(a.seed, m, g); }, e);
        double zz = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                z[c][u] = box.live[c][u] ? e[c][u] : 0.f;   // (padded dims stay 0)
                x[c][u] = z[c][u];
                zz += (double)z[c][u] * (double)z[c][u];
            }
        // over the row's 16 positions; the four rows hold copies
        zz += __shfl_xor(zz, 1);
        zz += __shfl_xor(zz, 2);
        zz += __shfl_xor(zz, 4);
        zz += __shfl_xor(zz, 8);
        double logl;
        const double lp = target(x, logl);
        const double logw = lp - importance_logb(zz, D);
        importance_add(run, logw, true);
        if (outs && writer_lane) {
            store_row(a.z_out + (size_t)k * D, z);
            store_row(a.x_out + (size_t)k * D, x);
            if (pos == 0) {
                a.logl_out[k] = logl;
                a.logw_out[k] = logw;
            }
        }
    }
    if (lane == 0) {
        red[wave][0] = run.a; red[wave][1] = run.s1; red[wave][2] = run.s2; red[wave][3] = run.n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ImpSums r = importance_empty();
        for (int w = 0; w < 4; ++w) r = importance_merge(r, ImpSums{red[w][0], red[w][1], red[w][2], red[w][3]});
        importance_publish(a.partials, a.sums, (int)blockIdx.x, r);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
template <int U, int FAM, bool PRIOR>
static hipError_t importance_glm_launch_k(const FlowShape &s, const float *packed, const ImpGlmArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((importance_glm_kernel<U, FAM, PRIOR>), dim3(a.groups), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

template <int FAM, bool PRIOR>
static hipError_t importance_glm_launch_f(const FlowShape &s, const float *packed, const ImpGlmArgs &a, hipStream_t st) {
    switch (s.NT) {
        case 1: return importance_glm_launch_k<1, FAM, PRIOR>(s, packed, a, st);
        case 2: return importance_glm_launch_k<2, FAM, PRIOR>(s, packed, a, st);
        case 3: return importance_glm_launch_k<3, FAM, PRIOR>(s, packed, a, st);
        case 4: return importance_glm_launch_k<4, FAM, PRIOR>(s, packed, a, st);
    }
    return hipErrorInvalidConfiguration;
}

hipError_t launch_importance_glm(const FlowShape &s, const float *packed, const ImpGlmArgs &a, hipStream_t st) {
    if (a.M <= 0 || a.groups <= 0) return hipSuccess;
    switch (a.gl.family) {
        case GLM_LOGISTIC:
            return a.prior ? importance_glm_launch_f<GLM_LOGISTIC, true>(s, packed, a, st)
                           : importance_glm_launch_f<GLM_LOGISTIC, false>(s, packed, a, st);
        case GLM_POISSON:
            return a.prior ? importance_glm_launch_f<GLM_POISSON, true>(s, packed, a, st)
                           : importance_glm_launch_f<GLM_POISSON, false>(s, packed, a, st);
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
