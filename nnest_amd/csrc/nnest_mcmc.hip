// nnest_mcmc.hip -- RANDOM-WALK METROPOLIS in the latent space of the trained flow with the likelihood, the prior and the Jacobian in
// the ratio: MCMCSampler's run (nnest/mcmc.py:79-126: Sampler._mcmc_sample with loglstar = None, nnest/sampler.py:372-416), every step
// of a launch inside the kernel.  BUILD-DEFINED STREAM, THE REFERENCE'S MOVE: the draws are Philox4x32-10 words of this library, so
// parity with torch's stream is statistical.
//
// Definition (include/nnest_hip.h nnest_mcmc_steps has it in full).  Walker k of the launch is walker
// w = walker_offset + k of the run; step t is a global index:
//   eps[4g .. 4g+3] = noise_normal4(seed, w, t, g, stream 5);  u = mcmc_uniform(seed, w, t) (stream 6);
//   q = z + step_size * eps (float32, no contraction);  the walker moves to q iff lp(q) - lp(z) > log u (float64: ens_accept_factor
//   with no factor, the DE step's rule);  lp is the latent target of solo_latent.h -- the inverse, ens_T, the box test with the
//   NaN-inside rule, solo_loglike at scale 1 -- combined by ens_target at constrained = 0 (ensemble_kernel's lp), and the walker
//   carries logL(T(x)) beside it.
//
// Layout: the solo layout (solo_latent.h): one walker per wave, four walkers per workgroup; the weights in registers (x_dim <= 64)
// or in LDS.  Walkers are independent: no hand-off, no residency limit, no work buffer, and a partial last workgroup simply has
// idle waves.  The lane's normals: solo_lane_normals.
//
// ONE loop runs the launch's evaluations -- i = -1 is the start, where nobody moves -- so the inverse is inlined once and the start
// of a launch is evaluated by the code that evaluated it as a proposal in the launch before: a run cut into launches is the same
// run, bit for bit.
//
// The TEMPERED run (nnest_mcmc_tempered_steps) is the same kernel with the likelihood to the power beta in lp
// (mcmc_target_tempered), a compile-time variant: the walker still carries and logs the untempered logL.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "mcmc_walk.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

// the draws, exported for the checker through the kernels' own functions: dz [S][C][D], u [S][C]
__global__ void mcmc_fill_noise_kernel(float *__restrict__ dz, float *__restrict__ u, int S, int C, int D, uint32_t step0, uint64_t seed,
                                       uint64_t walker_offset) {
    const int G = (D + 3) / 4;
    const long n = (long)S * C * G;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int g = (int)(e % G);
        const long r = e / G;   // i C + k
        const int k = (int)(r % C), i = (int)(r / C);
        const uint64_t w = walker_offset + (uint64_t)k;
        const uint32_t t = step0 + (uint32_t)i;
        if (dz) {
            const f32x4 v = mcmc_normal4(seed, w, t, (uint32_t)g);
            const float vv[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 4; ++j)
                if (4 * g + j < D) dz[r * D + 4 * g + j] = vv[j];
        }
        if (u && g == 0) u[r] = mcmc_uniform(seed, w, t);
    }
}

// TP: the tempered target (mcmc_target_tempered at a.beta), a compile-time variant: the TP = false instantiations are the kernels
// of nnest_mcmc_steps
template <int U, int LK, bool TP>
__global__ void __launch_bounds__(256) mcmc_kernel(FlowShape s, const float *__restrict__ packed, typename McmcArgsOf<TP>::type a) {
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
    SoloBox<U, LK> box;
    box.init(a, D, lane, pos);
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](float (&xs)[2][U], double &logl) -> double {
        return solo_latent_eval(flow, box, xs, [&](double l, float ld, bool in_prior) {
            logl = l;
            if constexpr (TP) return mcmc_target_tempered(l, ld, in_prior, a.beta);
            else return ens_target(l, ld, in_prior, 0, 0.0);
        });
    };

    const bool writer_lane = lane < 16;
    auto store_row = [&](float *base, const float (&v)[2][U]) { solo_store_row<U>(base, D, pos, v); };
    const uint64_t w = a.walker_offset + (uint64_t)row;
    const float step = a.step;

    float z[2][U], x[2][U];
    solo_load_row<U>(a.z_in + (size_t)row * D, D, pos, z);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c][u] = z[c][u];
    double lp = 0.0, logl = 0.0;
    int n_acc = 0;
    const bool hist = a.hist_z != nullptr;
#pragma unroll 1
    for (int i = -1; i < S; ++i) {
        const bool init = i < 0;
        const uint32_t t = a.step0 + (uint32_t)i;
        float q[2][U], xq[2][U];
        float uacc = 1.f;
        if (!init) {
            float e[2][U];
            solo_lane_normals<U>(pos, [&](uint32_t g) { return mcmc_normal4(a.seed, w, t, g); }, e);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) q[c][u] = box.live[c][u] ? mcmc_propose(z[c][u], step, e[c][u]) : 0.f;   // (padded dims stay 0)
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
        const bool acc = !init && ens_accept_factor(lpq, lp, 0.0, uacc);
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
        if (!init && hist && writer_lane) {
            const size_t hr = (size_t)row * S + i;
            store_row(a.hist_z + hr * D, z);
            store_row(a.hist_x + hr * D, x);
            if (pos == 0) a.hist_logl[hr] = logl;
        }
    }
    if (writer_lane) {
        if (S > 0) store_row(a.z_out + (size_t)row * D, z);   // (steps = 0 evaluates the start: x, lp and logL only)
        store_row(a.x_out + (size_t)row * D, x);
        if (pos == 0) {
            a.lp_out[row] = lp;
            a.logl_out[row] = logl;
            if (S > 0 && a.n_accept) a.n_accept[row] = n_acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
hipError_t launch_mcmc_fill_noise(float *dz, float *u, int S, int C, int D, uint32_t step0, uint64_t seed, uint64_t walker_offset,
                                  hipStream_t st) {
    if (S <= 0 || C <= 0 || (!dz && !u)) return hipSuccess;
    hipLaunchKernelGGL(mcmc_fill_noise_kernel, dim3(256), dim3(256), 0, st, dz, u, S, C, D, step0, seed, walker_offset);
    return hipGetLastError();
}

template <int U, int LK, bool TP>
static hipError_t mcmc_launch_k(const FlowShape &s, const float *packed, const typename McmcArgsOf<TP>::type &a, hipStream_t st) {
    hipLaunchKernelGGL((mcmc_kernel<U, LK, TP>), dim3((a.C + 3) / 4), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

template <bool TP>
static hipError_t mcmc_dispatch(const FlowShape &s, const float *packed, const typename McmcArgsOf<TP>::type &a, hipStream_t st) {
    if (a.C <= 0) return hipSuccess;
    return solo_for_shape(s.NT, a.like.id, [&](auto sh) { return mcmc_launch_k<decltype(sh)::U, decltype(sh)::LK, TP>(s, packed, a, st); });
}

hipError_t launch_mcmc(const FlowShape &s, const float *packed, const McmcArgs &a, hipStream_t st) {
    return mcmc_dispatch<false>(s, packed, a, st);
}
hipError_t launch_mcmc_tempered(const FlowShape &s, const float *packed, const McmcTemperedArgs &a, hipStream_t st) {
    return mcmc_dispatch<true>(s, packed, a, st);
}

}  // namespace nnest
