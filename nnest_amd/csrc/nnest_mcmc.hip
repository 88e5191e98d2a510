// nnest_mcmc.hip -- RANDOM-WALK METROPOLIS in the latent space of the trained flow with the likelihood, the prior and the Jacobian in
// the ratio: MCMCSampler's run (nnest/mcmc.py:79-126: Sampler._mcmc_sample with loglstar = None, nnest/sampler.py:372-416), every step
// of a launch inside the kernel.  BUILD-DEFINED STREAM, THE REFERENCE'S MOVE: the draws are Philox4x32-10 words of this library, so
// parity with torch's stream is statistical.
//
// Definition (include/nnest_hip.h nnest_mcmc_steps has it in full).  Walker k of the launch is walker
// w = walker_offset + k of the run; step t is a global index:
//   eps[4g .. 4g+3] = noise_normal4(seed, w, t, g, stream 5);  u = mcmc_uniform(seed, w, t) (stream 6);
//   q = z + step_size * eps (float32, no contraction);  the walker moves to q iff lp(q) - lp(z) > log u (float64: ens_accept_factor
//   with no factor, the DE step's rule);  lp is the target of ensemble_kernel (nnest_ensemble.hip) at constrained = 0 -- the same
//   inverse, ens_T, box test, NaN-inside rule, solo_loglike at scale 1 and ens_target -- and the walker carries logL(T(x)) beside it.
//
// Layout: ensemble_kernel's (the solo layout of nnest_solo.hip): one walker per wave, lane = 32 n + 16 h + p holds dims
// 2U p + 2u + c, the four (n, h) rows hold copies; four walkers per workgroup; the weights in registers (x_dim <= 64) or in LDS.
// Walkers are independent: no hand-off, no residency limit, no work buffer, and a partial last workgroup simply has idle waves.
// A lane's 2U consecutive dims lie in one Philox block (U = 1: half of one; U = 2: exactly one) or in two (U = 3, 4); every (n, h)
// row draws the same block, so the copies stay copies.
//
// The target is written out here rather than shared with ensemble_kernel: that kernel's instantiations are sensitive to how its
// target is wrapped (see the comments there), and this one returns logL beside lp.  ONE loop runs the launch's evaluations -- i = -1
// is the start, where nobody moves -- so the inverse is inlined once and the start of a launch is evaluated by the code that
// evaluated it as a proposal in the launch before: a run cut into launches is the same run, bit for bit.
//
// The TEMPERED run (nnest_mcmc_tempered_steps) is the same kernel with the likelihood to the power beta in lp
// (mcmc_target_tempered), a compile-time variant: the walker still carries and logs the untempered logL.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "mcmc_walk.h"
#include "nnest_internal.h"
#include "solo_loglike.h"
#include "solo_tile.h"

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
// of nnest_mcmc_steps as they were, instruction for instruction
template <int U, int LK, bool TP>
__global__ void __launch_bounds__(256) mcmc_kernel(FlowShape s, const float *__restrict__ packed, typename McmcArgsOf<TP>::type a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, C = a.C, S = a.S;
    constexpr bool LDSW = U >= 3;   // (solo_lds_weights<U, 4>: x_dim > 64 keeps the weights in LDS)
    {
        if constexpr (!LDSW) {
            const int n = s.nets_params();
            for (int i = threadIdx.x; i < n; i += blockDim.x) wlds[i] = packed[i];
        } else if (wave < 3) {
            SoloNet<U> nb;
            solo_gather<U>(nb, packed + (size_t)(wave * 2 + (lane >= 32 ? 1 : 0)) * s.net_params, D, (wave + 1) & 1, wave & 1, lane);
            solo4_store<U>(wlds, wave, nb, lane);
        }
    }
    __syncthreads();
    const int pos = lane & 15;
    const bool translate_half = lane >= 32;
    const int row = blockIdx.x * 4 + wave;
    if (row >= C) return;   // (no barrier behind this point)
    SoloNet<U> net[LDSW ? 1 : 3];
    if constexpr (!LDSW) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
            solo_gather<U>(net[b], wlds + (size_t)(b * 2 + (translate_half ? 1 : 0)) * s.net_params, D, (b + 1) & 1, b & 1, lane);
    }
    const unsigned sel = translate_half ? 0xffffffffu : 0u;
    const bool h1 = (lane & 16) != 0;
    auto inverse = [&](float (&xs)[2][U]) {   // NormalizingFlow.inverse (networks.py:34-42), blocks 2, 1, 0
        if constexpr (LDSW) {
            float ld = solo_coupling_inverse4<U>(Solo4Lds{wlds + (size_t)2 * SOLO4_NF * 64, lane}, sel, h1, xs[1], xs[0]);
            ld += solo_coupling_inverse4<U>(Solo4Lds{wlds + (size_t)1 * SOLO4_NF * 64, lane}, sel, h1, xs[0], xs[1]);
            ld += solo_coupling_inverse4<U>(Solo4Lds{wlds, lane}, sel, h1, xs[1], xs[0]);
            return ld;
        } else {
            float ld;
            solo_coupling_inverse<U, true>(net[2], sel, h1, xs[1], xs[0], ld);
            solo_coupling_inverse<U, false>(net[1], sel, h1, xs[0], xs[1], ld);
            solo_coupling_inverse<U, false>(net[0], sel, h1, xs[1], xs[0], ld);
            return ld;
        }
    };
    // this lane's dims: T (NULL: x * 1 + 0), the box
    float sd[2][U], mu[2][U], blo[2][U], bhi[2][U];
    bool live[2][U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = 2 * U * pos + 2 * u + c;
            const bool v = d < D;
            live[c][u] = v;
            sd[c][u] = v ? (a.t_std ? a.t_std[d] : 1.f) : 0.f;
            mu[c][u] = v && a.t_mean ? a.t_mean[d] : 0.f;
            blo[c][u] = v && a.lo ? a.lo[d] : -INFINITY;
            bhi[c][u] = v && a.hi ? a.hi[d] : INFINITY;
        }
    LikeSpec like = a.like;
    like.scale = 1.0f;
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](float (&xs)[2][U], double &logl) -> double {
        const float ld = solo_logdet_total(inverse(xs));
        float tx[2][U];
        int ok = 1;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                tx[c][u] = ens_T(xs[c][u], sd[c][u], mu[c][u]);
                ok &= !(tx[c][u] < blo[c][u] || tx[c][u] > bhi[c][u]);   // (NaN counts as inside: UniformPrior, priors.py)
            }
        const bool in_prior = __ballot(ok != 0) == ~0ull;
        logl = solo_loglike<U, LK>(like, D, lane, tx);
        if constexpr (TP) return mcmc_target_tempered(logl, ld, in_prior, a.beta);
        else return ens_target(logl, ld, in_prior, 0, 0.0);
    };

    const bool writer_lane = lane < 16;
    auto store_row = [&](float *base, const float (&v)[2][U]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int d = 2 * U * pos + 2 * u + c;
                if (d < D) base[d] = v[c][u];
            }
    };
    // the lane's 2U dims start at dim 2U pos: component `off` (0 or 2) of Philox block g0
    constexpr int NB = U <= 2 ? 1 : 2;
    const uint32_t g0 = (uint32_t)(2 * U * pos) >> 2;
    const uint32_t offm = ((2 * U * pos) & 3) != 0 ? 0xffffffffu : 0u;
    const uint64_t w = a.walker_offset + (uint64_t)row;
    const float step = a.step;

    float z[2][U], x[2][U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = 2 * U * pos + 2 * u + c;
            z[c][u] = d < D ? a.z_in[(size_t)row * D + d] : 0.f;
            x[c][u] = z[c][u];
        }
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
            float n[4 * NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const f32x4 v = mcmc_normal4(a.seed, w, t, g0 + (uint32_t)b);
                n[4 * b] = v.x; n[4 * b + 1] = v.y; n[4 * b + 2] = v.z; n[4 * b + 3] = v.w;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int k = 2 * u + c;
                    float e = n[k];
                    // (a lane whose dims start at component 2; a mask, as the coupling code selects: as `off2 ? n[k + 2] : n[k]` the
                    // compiler selects the address and keeps n in scratch)
                    if constexpr ((U & 1) != 0)
                        e = __uint_as_float((__float_as_uint(n[k]) & ~offm) | (__float_as_uint(n[k + 2]) & offm));
                    q[c][u] = live[c][u] ? mcmc_propose(z[c][u], step, e) : 0.f;   // (padded dims stay 0)
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
    // (ensemble_kernel's LDS: the packed nets, or the three blocks' gathered fields at x_dim > 64)
    const size_t lds = U >= 3 ? (size_t)3 * SOLO4_NF * 64 * sizeof(float) : (size_t)s.nets_params() * sizeof(float);
    hipLaunchKernelGGL((mcmc_kernel<U, LK, TP>), dim3((a.C + 3) / 4), dim3(256), lds, st, s, packed, a);
    return hipGetLastError();
}

template <bool TP>
static hipError_t mcmc_dispatch(const FlowShape &s, const float *packed, const typename McmcArgsOf<TP>::type &a, hipStream_t st) {
    if (a.C <= 0) return hipSuccess;
    const bool rosen = a.like.id == NNEST_LIKE_ROSENBROCK;
    switch (s.NT) {
        case 1: return rosen ? mcmc_launch_k<1, NNEST_LIKE_ROSENBROCK, TP>(s, packed, a, st) : mcmc_launch_k<1, -1, TP>(s, packed, a, st);
        case 2: return rosen ? mcmc_launch_k<2, NNEST_LIKE_ROSENBROCK, TP>(s, packed, a, st) : mcmc_launch_k<2, -1, TP>(s, packed, a, st);
        case 3: return rosen ? mcmc_launch_k<3, NNEST_LIKE_ROSENBROCK, TP>(s, packed, a, st) : mcmc_launch_k<3, -1, TP>(s, packed, a, st);
        case 4: return rosen ? mcmc_launch_k<4, NNEST_LIKE_ROSENBROCK, TP>(s, packed, a, st) : mcmc_launch_k<4, -1, TP>(s, packed, a, st);
    }
    return hipErrorInvalidConfiguration;
}

hipError_t launch_mcmc(const FlowShape &s, const float *packed, const McmcArgs &a, hipStream_t st) {
    return mcmc_dispatch<false>(s, packed, a, st);
}
hipError_t launch_mcmc_tempered(const FlowShape &s, const float *packed, const McmcTemperedArgs &a, hipStream_t st) {
    return mcmc_dispatch<true>(s, packed, a, st);
}

}  // namespace nnest
