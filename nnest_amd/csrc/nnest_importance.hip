// nnest_importance.hip -- IMPORTANCE-SAMPLED EVIDENCE from the trained flow: Z = E_q[L(T(x)) pi(T(x)) / q(x)] with the flow as the
// proposal q, drawn, evaluated and reduced inside one kernel (include/nnest_hip.h nnest_importance_evidence has the definition in
// full).  BUILD-DEFINED: the reference has no such estimator.  Sample k of the launch is sample
// m = sample_offset + k of the run:
//   z_m[4g .. 4g+3] = noise_normal4(seed, m, 0, g, stream 7);  lp(z_m) = nnest_mcmc_steps's target (solo_latent.h's latent target
//   combined by ens_target);  logw_m = lp(z_m) - logb(z_m) in float64, logb the N(0, I) density.
//
// Layout: the solo layout (solo_latent.h, which states the target and the lane's normals; this kernel keeps a written-out copy of
// both, for a measured reason: see the comment above it): one sample per wave; the weights in registers (x_dim <= 64) or in LDS.
// The grid is PERSISTENT: a workgroup loads the weights once, then wave `wg` of the grid's `nw` takes samples wg, wg + nw, ...  A
// lane's dims map to Philox blocks as mcmc_kernel's eps do.  sum z^2 is reduced over a row's 16 positions in float64 (a butterfly:
// every lane of the wave ends with the same bits).
//
// Reduction, deterministic, no floating-point atomics: each wave keeps a running (a, S1, S2, n) (importance_walk.h), the four waves
// of a workgroup are merged in wave order by one thread, which writes the workgroup's partial; importance_combine_kernel, one
// workgroup, merges the partials in index order.  The live count travels as an integer (importance_publish).
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "importance_walk.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

// the draws, exported for the checker through the kernels' own function: z [M][D]
__global__ void importance_fill_noise_kernel(float *__restrict__ z, int M, int D, uint64_t seed, uint64_t sample_offset) {
    const int G = (D + 3) / 4;
    const long n = (long)M * G;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int g = (int)(e % G);
        const long k = e / G;
        const f32x4 v = importance_normal4(seed, sample_offset + (uint64_t)k, (uint32_t)g);
        const float vv[4] = {v.x, v.y, v.z, v.w};
        for (int j = 0; j < 4; ++j)
            if (4 * g + j < D) z[k * D + 4 * g + j] = vv[j];
    }
}

// sums[3] is the launch's integer live count from here to importance_combine_kernel
__global__ void importance_begin_kernel(double *sums) { *reinterpret_cast<unsigned long long *>(sums + 3) = 0ull; }

// the second stage: ONE workgroup, one thread merges the partials in index order (groups is a few thousand at most)
__global__ void importance_combine_kernel(const double *__restrict__ partials, double *__restrict__ sums, int groups) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ImpSums r = importance_empty();
    for (int g = 0; g < groups; ++g) r = importance_merge(r, ImpSums{partials[3 * g], partials[3 * g + 1], partials[3 * g + 2], 0.0});
    const unsigned long long n = *reinterpret_cast<const unsigned long long *>(sums + 3);
    sums[0] = r.a;
    sums[1] = r.s1;
    sums[2] = r.s2;
    sums[3] = (double)n;
}

// This kernel keeps its target WRITTEN OUT (the text solo_latent.h states for mcmc_kernel and ensemble_x_kernel).  On the shared
// header importance_kernel<1, -1> measured above the parent by more than the parent's spread in every run: x_dim 20 GaussianMix,
// 2^22 samples, 4.324 -> 4.365 ms, spread 0.017 (profiles/latent_target/timing.txt, section 3); T and the box were then loaded through
// nested branches instead of predicated loads, 3073 instructions for 3051.  As written here every instantiation is the parent's,
// instruction for instruction.
template <int U, int LK>
__global__ void __launch_bounds__(256) importance_kernel(FlowShape s, const float *__restrict__ packed, ImpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, M = a.M;
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
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl` (solo_latent.h's target, combined by ens_target)
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
        return ens_target(logl, ld, in_prior, 0, 0.0);
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
    // the lane's 2U dims start at dim 2U pos: component `off` (0 or 2) of Philox block g0 (solo_lane_normals, written out)
    constexpr int NB = U <= 2 ? 1 : 2;
    const uint32_t g0 = (uint32_t)(2 * U * pos) >> 2;
    const uint32_t offm = ((2 * U * pos) & 3) != 0 ? 0xffffffffu : 0u;
    const bool outs = a.z_out != nullptr;
    const int nw = (int)gridDim.x * 4, wg = (int)blockIdx.x * 4 + wave;

    ImpSums run = importance_empty();
#pragma unroll 1
    for (int k = wg; k < M; k += nw) {   // (M <= 2^30: k + nw stays inside int)
        const uint64_t m = a.sample_offset + (uint64_t)k;
        float n[4 * NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4 v = importance_normal4(a.seed, m, g0 + (uint32_t)b);
            n[4 * b] = v.x; n[4 * b + 1] = v.y; n[4 * b + 2] = v.z; n[4 * b + 3] = v.w;
        }
        float z[2][U], x[2][U];
        double zz = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = 2 * u + c;
                float e = n[j];
                // (a lane whose dims start at component 2; a mask: solo_lane_normals)
                if constexpr ((U & 1) != 0)
                    e = __uint_as_float((__float_as_uint(n[j]) & ~offm) | (__float_as_uint(n[j + 2]) & offm));
                z[c][u] = live[c][u] ? e : 0.f;   // (padded dims stay 0)
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
int importance_groups(int M, int tile, int num_cu) {
    if (M <= 0) return 0;
    const long need = ((long)M + tile - 1) / tile;
    const long cap = (long)num_cu * (tile == IMP_NVP_TILE ? IMP_NVP_GROUPS_PER_CU : IMP_SPLINE_GROUPS_PER_CU);
    return (int)(need < cap ? need : cap);
}

hipError_t launch_importance_fill_noise(float *z, int M, int D, uint64_t seed, uint64_t sample_offset, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(importance_fill_noise_kernel, dim3(256), dim3(256), 0, st, z, M, D, seed, sample_offset);
    return hipGetLastError();
}

hipError_t launch_importance_begin(double *sums, hipStream_t st) {
    hipLaunchKernelGGL(importance_begin_kernel, dim3(1), dim3(1), 0, st, sums);
    return hipGetLastError();
}

hipError_t launch_importance_combine(const double *partials, double *sums, int groups, hipStream_t st) {
    hipLaunchKernelGGL(importance_combine_kernel, dim3(1), dim3(64), 0, st, partials, sums, groups);
    return hipGetLastError();
}

template <int U, int LK>
static hipError_t importance_launch_k(const FlowShape &s, const float *packed, const ImpArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((importance_kernel<U, LK>), dim3(a.groups), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

hipError_t launch_importance(const FlowShape &s, const float *packed, const ImpArgs &a, hipStream_t st) {
    if (a.M <= 0 || a.groups <= 0) return hipSuccess;
    return solo_for_shape(s.NT, a.like.id, [&](auto sh) { return importance_launch_k<decltype(sh)::U, decltype(sh)::LK>(s, packed, a, st); });
}

}  // namespace nnest
