// nnest_mcmc_glm.hip -- the ADAPTIVE WALK in the latent space of the trained flow on a GENERALISED LINEAR MODEL of the user's data
// (logistic or Poisson regression): nnest_mcmc_adapt_steps's run (nnest_mcmc_adapt.hip has the definition: draws, schedule, weight,
// accept rule, step rule, beta, the state handed between launches) with the likelihood of glm_data.h compiled in, in a kernel of its
// own; and the likelihood alone on rows that are already T(x) (nnest_loglike_glm).  include/nnest_hip.h nnest_mcmc_glm_steps;
// DESIGN.md 3.16.  BUILD-DEFINED.  The adaptive walk is a superset -- adapt_steps = 0 without step_in is the mixed walk,
// global_every = 0 the random walk, beta the tempering --, so one kernel per family serves every fused Metropolis route.
//
// Layout: mcmc_gdata_kernel's, the solo layout, one walker per wave; the flow half is solo_latent.h's SoloFlow, T and the box are
// SoloBox::map, in front of the likelihood of glm_data.h (data rows over the wave's 64 lanes).
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "glm_data.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

template <int U, int FAM>
__global__ void __launch_bounds__(256) mcmc_glm_kernel(FlowShape s, const float *__restrict__ packed, McmcGlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, C = a.C, S = a.S;
    SoloFlow<U>::stage(wlds, s, packed, lane, wave);
    __syncthreads();
    const int pos = lane & 15;
    const int row = blockIdx.x * 4 + wave;
    if (row >= C) return;   // (no barrier behind this point)
    SoloFlow<U> flow;
    flow.init(wlds, s, lane);
    SoloBox<U, NNEST_LIKE_GAUSSIAN> box;   // (T and the box; its likelihood is not called)
    box.init(a, D, lane, pos);
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl` (solo_latent_eval, with the likelihood of glm_data.h)
    auto target = [&](float (&xs)[2][U], double &logl) -> double {
        const float ld = solo_logdet_total(flow.inverse(xs));
        float tx[2][U];
        const bool in_prior = box.map(xs, tx);
        logl = glm_solo_loglike<U, FAM>(a.gl, lane, tx);
        return mcmc_target_tempered(logl, ld, in_prior, a.beta);
    };

    const bool writer_lane = lane < 16;
    auto store_row = [&](float *base, const float (&v)[2][U]) { solo_store_row<U>(base, D, pos, v); };
    const uint64_t w = a.walker_offset + (uint64_t)row;
    // the walker's step: float64 between the steps, rounded to float32 where the proposal uses it
    double sigma = a.step_in ? adapt_clamp(a.step_in[row]) : (double)a.step;
    MixedPhase phase;
    phase.init(a.step0, a.global_every);

    float z[2][U], x[2][U];
    solo_load_row<U>(a.z_in + (size_t)row * D, D, pos, z);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c][u] = z[c][u];
    double lp = 0.0, logl = 0.0;
    int n_acc = 0, n_acc_g = 0;
    const bool hist = a.hist_z != nullptr;
#pragma unroll 1
    for (int i = -1; i < S; ++i) {
        const bool init = i < 0;
        const uint32_t t = a.step0 + (uint32_t)i;
        const bool glob = !init && phase.next_is_global();
        float q[2][U], xq[2][U];
        float uacc = 1.f;
        if (!init) {
            float e[2][U];
            solo_lane_normals<U>(pos, [&](uint32_t g) { return mcmc_normal4(a.seed, w, t, g); }, e);
            const float step = (float)sigma;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) {   // (padded dims stay 0)
                    const float ql = mcmc_propose(z[c][u], step, e[c][u]);
                    q[c][u] = box.live[c][u] ? (glob ? e[c][u] : ql) : 0.f;
                }
            uacc = mcmc_uniform(a.seed, w, t);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) q[c][u] = z[c][u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) xq[c][u] = q[c][u];
        double loglq;
        const double lpq = target(xq, loglq);
        // the two sides of the accept rule: lp on a local step, the log importance weight on a global one
        double lnew = lpq, lold = lp;
        if (glob) {
            lnew = mixed_logw(lpq, solo_row_zz<U>(q), D);
            lold = mixed_logw(lp, solo_row_zz<U>(z), D);
        }
        const bool acc = !init && ens_accept_factor(lnew, lold, 0.0, uacc);
        if (acc || init) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) { z[c][u] = q[c][u]; x[c][u] = xq[c][u]; }
            lp = lpq;
            logl = loglq;
        }
        if (init && a.lp_in) { lp = a.lp_in[row]; logl = a.logl_in[row]; }
        n_acc += acc ? 1 : 0;
        n_acc_g += acc && glob ? 1 : 0;
        if (!init && !glob && t < a.adapt_steps) sigma = adapt_update(sigma, t, acc, a.adapt_rate, a.target_accept);
        if (!init && hist && writer_lane) {
            const size_t hr = (size_t)row * S + i;
            store_row(a.hist_z + hr * D, z);
            store_row(a.hist_x + hr * D, x);
            if (pos == 0) a.hist_logl[hr] = logl;
        }
        if (!init && a.hist_step && lane == 0) a.hist_step[(size_t)row * S + i] = sigma;
    }
    if (writer_lane) {
        if (S > 0) store_row(a.z_out + (size_t)row * D, z);   // (steps = 0 evaluates the start: x, lp and logL only)
        store_row(a.x_out + (size_t)row * D, x);
        if (pos == 0) {
            a.lp_out[row] = lp;
            a.logl_out[row] = logl;
            if (S > 0 && a.n_accept) a.n_accept[row] = n_acc;
            if (S > 0 && a.n_accept_global) a.n_accept_global[row] = n_acc_g;
            if (S > 0 && a.step_out) a.step_out[row] = sigma;
        }
    }
}

// the likelihood alone: row n of t [N, D] on wave n of the launch (four rows a workgroup), in the layout of the walk's kernel
template <int U, int FAM>
__global__ void __launch_bounds__(256) loglike_glm_kernel(GlmSpec gl, const float *__restrict__ t, double *__restrict__ logl, int N) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pos = lane & 15;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= N) return;
    float tx[2][U];
    solo_load_row<U>(t + (size_t)row * gl.D, gl.D, pos, tx);
    const double l = glm_solo_loglike<U, FAM>(gl, lane, tx);
    if (lane == 0) logl[row] = l;
}

// ------------------------------------------------------------------------------------------------
// host side
template <int U, int FAM>
static hipError_t mcmc_glm_launch_k(const FlowShape &s, const float *packed, const McmcGlmArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((mcmc_glm_kernel<U, FAM>), dim3((a.C + 3) / 4), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

template <int FAM>
static hipError_t mcmc_glm_launch_f(const FlowShape &s, const float *packed, const McmcGlmArgs &a, hipStream_t st) {
    return solo_for_U(s.NT, [&](auto sh) { return mcmc_glm_launch_k<decltype(sh)::U, FAM>(s, packed, a, st); });
}

hipError_t launch_mcmc_glm(const FlowShape &s, const float *packed, const McmcGlmArgs &a, hipStream_t st) {
    if (a.C <= 0) return hipSuccess;
    switch (a.gl.family) {
        case GLM_LOGISTIC: return mcmc_glm_launch_f<GLM_LOGISTIC>(s, packed, a, st);
        case GLM_POISSON: return mcmc_glm_launch_f<GLM_POISSON>(s, packed, a, st);
    }
    return hipErrorInvalidConfiguration;
}

template <int U, int FAM>
static hipError_t loglike_glm_launch_k(const GlmSpec &gl, const float *t, double *logl, int N, hipStream_t st) {
    hipLaunchKernelGGL((loglike_glm_kernel<U, FAM>), dim3((N + 3) / 4), dim3(256), 0, st, gl, t, logl, N);
    return hipGetLastError();
}

template <int FAM>
static hipError_t loglike_glm_launch_f(const GlmSpec &gl, const float *t, double *logl, int N, hipStream_t st) {
    // (U: the lane's 2U dims, 32 U >= D)
    return solo_for_U((gl.D + 31) / 32, [&](auto sh) { return loglike_glm_launch_k<decltype(sh)::U, FAM>(gl, t, logl, N, st); });
}

hipError_t launch_loglike_glm(const GlmSpec &gl, const float *t, double *logl, int N, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    switch (gl.family) {
        case GLM_LOGISTIC: return loglike_glm_launch_f<GLM_LOGISTIC>(gl, t, logl, N, st);
        case GLM_POISSON: return loglike_glm_launch_f<GLM_POISSON>(gl, t, logl, N, st);
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
