// nnest_mcmc_glm_prior.hip -- the ADAPTIVE WALK in the latent space of the trained flow on a GENERALISED LINEAR MODEL of the user's data
// UNDER INDEPENDENT NORMAL PRIORS on the coefficients: nnest_mcmc_glm_steps's run (nnest_mcmc_glm.hip; nnest_mcmc_adapt.hip has the
// definition: draws, schedule, weight, accept rule, step rule, beta, the state handed between launches) with log pi of gauss_prior.h
// in the target where that kernel adds 0.0, in a kernel of its own; and the prior alone on rows that are already T(x)
// (nnest_logprior_gauss).  include/nnest_hip.h nnest_mcmc_glm_prior_steps; DESIGN.md 3.17.  BUILD-DEFINED.
//
// Layout: mcmc_glm_kernel's, the solo layout, one walker per wave.  m and r of the lane's 2U dims sit in registers beside SoloBox's
// fields, loaded once a launch (padded dims: r = 0); the sum of squares takes the lane's 2U products and the four-step xor butterfly
// over the 16 positions -- no LDS, no barrier.  nnest_mcmc_glm.hip stays what it is: its body is restated here.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "gauss_prior.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

template <int U, int FAM>
__global__ void __launch_bounds__(256) mcmc_glm_prior_kernel(FlowShape s, const float *__restrict__ packed, McmcGlmPriorArgs a) {
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
    float pm[2][U], pr[2][U];   // the prior's m and r of the lane's dims
    gauss_prior_solo_load<U>(a.pr, pos, pm, pr);
    const double logc = a.pr.logc;
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](float (&xs)[2][U], double &logl) -> double {
        const float ld = solo_logdet_total(flow.inverse(xs));
        float tx[2][U];
        const bool in_box = box.map(xs, tx);
        const double logpi = gauss_prior_solo<U>(tx, pm, pr, logc);
        logl = glm_solo_loglike<U, FAM>(a.gl, lane, tx);
        return mcmc_target_tempered_prior(logl, ld, in_box, logpi, a.beta);
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

// the prior alone: row n of t [N, D] on wave n of the launch (four rows a workgroup), in the layout of the walk's kernel
template <int U>
__global__ void __launch_bounds__(256) logprior_gauss_kernel(GaussPriorSpec p, const float *__restrict__ t, double *__restrict__ logp, int N) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pos = lane & 15;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= N) return;
    float tx[2][U], pm[2][U], pr[2][U];
    solo_load_row<U>(t + (size_t)row * p.D, p.D, pos, tx);
    gauss_prior_solo_load<U>(p, pos, pm, pr);
    const double l = gauss_prior_solo<U>(tx, pm, pr, p.logc);
    if (lane == 0) logp[row] = l;
}

// ------------------------------------------------------------------------------------------------
// host side
template <int U, int FAM>
static hipError_t mcmc_glm_prior_launch_k(const FlowShape &s, const float *packed, const McmcGlmPriorArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((mcmc_glm_prior_kernel<U, FAM>), dim3((a.C + 3) / 4), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

template <int FAM>
static hipError_t mcmc_glm_prior_launch_f(const FlowShape &s, const float *packed, const McmcGlmPriorArgs &a, hipStream_t st) {
    return solo_for_U(s.NT, [&](auto sh) { return mcmc_glm_prior_launch_k<decltype(sh)::U, FAM>(s, packed, a, st); });
}

hipError_t launch_mcmc_glm_prior(const FlowShape &s, const float *packed, const McmcGlmPriorArgs &a, hipStream_t st) {
    if (a.C <= 0) return hipSuccess;
    switch (a.gl.family) {
        case GLM_LOGISTIC: return mcmc_glm_prior_launch_f<GLM_LOGISTIC>(s, packed, a, st);
        case GLM_POISSON: return mcmc_glm_prior_launch_f<GLM_POISSON>(s, packed, a, st);
    }
    return hipErrorInvalidConfiguration;
}

template <int U>
static hipError_t logprior_gauss_launch_k(const GaussPriorSpec &p, const float *t, double *logp, int N, hipStream_t st) {
    hipLaunchKernelGGL((logprior_gauss_kernel<U>), dim3((N + 3) / 4), dim3(256), 0, st, p, t, logp, N);
    return hipGetLastError();
}

hipError_t launch_logprior_gauss(const GaussPriorSpec &p, const float *t, double *logp, int N, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    // (U: the lane's 2U dims, 32 U >= D)
    return solo_for_U((p.D + 31) / 32, [&](auto sh) { return logprior_gauss_launch_k<decltype(sh)::U>(p, t, logp, N, st); });
}

}  // namespace nnest
