// nnest_spline_importance.hip -- IMPORTANCE-SAMPLED EVIDENCE from the trained neural-spline flow (include/nnest_hip.h
// nnest_spline_importance_evidence).  BUILD-DEFINED.  The definition is nnest_importance_evidence's (nnest_importance.hip has it), with
// the same draws, base density, sums and merge (importance_walk.h): only the flow differs -- the spline's inverse (spline_inverse.h)
// replaces the coupling stack -- and with it the layout.
//
// Layout: the TEAM tile of nnest_spline_mcmc.hip: 16 samples per workgroup and pass, four waves per tile.  Every wave carries the
// same 16 samples in the parity-class tiles of flow_tile.h; only the spline evaluations of the inverse are divided between the waves
// (SplineInverseTeam).  The grid is PERSISTENT: workgroup b takes tiles b, b + groups, ...; T's scale and offset and the box are put
// in LDS once.  A lane's eight dims of tile column tau are the Philox blocks 8 tau + 2 g and 8 tau + 2 g + 1 of its sample, as
// mcmc_tile_walk draws its eps.  Rows >= M of the last tile evaluate their point (the sample one past the launch's) and are neither
// counted nor written.  Every wave runs every tile of its workgroup, so the team's barriers inside the inverse always meet.
//
// Reduction: lane (g, r) keeps the running sums of the samples that came through row r; log-det and likelihood are bit-identical on
// the four lane groups and on the four waves (nnest_spline_mcmc.hip), so the four waves hold identical sums.  At the end a butterfly
// over the 16 rows with the symmetric merge leaves every lane with the same bits, and wave 0 publishes.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mcmc.hip is: a loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "importance_walk.h"
#include "mh_common.h"
#include "nnest_internal.h"
#include "spline_train_tile.h"

namespace nnest {

#include "spline_inverse.h"

// class c of the lane's eight consecutive values v0 (dims 0..3 of its block pair) and v1 (4..7): load_tile's layout
__device__ __forceinline__ f32x4 imp_class(const f32x4 &v0, const f32x4 &v1, int c) {
    return c ? (f32x4){v0.y, v0.w, v1.y, v1.w} : (f32x4){v0.x, v0.z, v1.x, v1.z};
}

__device__ __forceinline__ double imp_shfl_xor(double v, int mask) { return __shfl_xor(v, mask); }

// LDS of the team form (spline_mcmc_kernel_team's): the waves' layout-exchange buffers, the spline exchange, the log-det reduction, T
__host__ __device__ inline int spl_imp_lds_tpar(int D, int NT) { return ((4 * 16 * (D + 1) + 3) & ~3) + 4 * NT * 64 * 4 + 4 * 16; }
__host__ __device__ inline int spl_imp_lds_floats(int D, int NT) { return spl_imp_lds_tpar(D, NT) + 4 * 32 * NT; }

template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_importance_kernel_team(ImpArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = q.sp.D, M = a.M;
    float *bufs = lds_buf;                                                                 // 4 x 16 x (D+1)
    f32x4 *xch = reinterpret_cast<f32x4 *>(lds_buf + ((4 * 16 * (D + 1) + 3) & ~3));      // 4 x NT x 64 f32x4
    float *ldred = reinterpret_cast<float *>(xch + 4 * NT * 64);                           // 4 x 16
    float *tpar = lds_buf + spl_imp_lds_tpar(D, NT);                                       // 4 x 32 NT
    for (int d = threadIdx.x; d < 32 * NT; d += 256) {
        const bool v = d < D;
        tpar[d] = v ? (a.t_std ? a.t_std[d] : 1.f) : 0.f;
        tpar[32 * NT + d] = v && a.t_mean ? a.t_mean[d] : 0.f;
        tpar[2 * 32 * NT + d] = v && a.lo ? a.lo[d] : -INFINITY;
        tpar[3 * 32 * NT + d] = v && a.hi ? a.hi[d] : INFINITY;
    }
    __syncthreads();
    SplineInverseTeam<NT, NH, 4> inv = {q.img, q.sp, bufs + (size_t)wv * 16 * (D + 1), xch, ldred, lane, wv};
    const int g = lane >> 4;
    LikeSpec like = a.like;
    like.scale = 1.0f;

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl` (mcmc_tile_walk's target)
    auto target = [&](f32x4 (&xs)[2][NT], double &logl) -> double {
        const float ld = group_sum(inv(xs));
        f32x4 tx[2][NT];
        int inside = 1;
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(tpar + 32 * tau + 8 * g);
            constexpr int PW = 8 * NT;   // f32x4 per parameter
            const f32x4 s0 = p[0], s1 = p[1], m0 = p[PW], m1 = p[PW + 1], l0 = p[2 * PW], l1 = p[2 * PW + 1], h0 = p[3 * PW], h1 = p[3 * PW + 1];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const f32x4 sd = imp_class(s0, s1, c), mu = imp_class(m0, m1, c), lo = imp_class(l0, l1, c), hi = imp_class(h0, h1, c);
                f32x4 t;
                t.x = ens_T(xs[c][tau].x, sd.x, mu.x); t.y = ens_T(xs[c][tau].y, sd.y, mu.y);
                t.z = ens_T(xs[c][tau].z, sd.z, mu.z); t.w = ens_T(xs[c][tau].w, sd.w, mu.w);
                // (NaN counts as inside: UniformPrior, priors.py)
                inside &= !(t.x < lo.x || t.x > hi.x) & !(t.y < lo.y || t.y > hi.y) & !(t.z < lo.z || t.z > hi.z) & !(t.w < lo.w || t.w > hi.w);
                tx[c][tau] = t;
            }
        }
        const bool in_prior = group_all(inside != 0, lane) != 0;
        logl = loglike_tile<NT>(like, D, lane, tx);
        return ens_target(logl, ld, in_prior, 0, 0.0);
    };

    const bool outs = a.z_out != nullptr;
    const int ntiles = (M + IMP_SPLINE_TILE - 1) / IMP_SPLINE_TILE;
    ImpSums run = importance_empty();
#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
        const int row = tile * IMP_SPLINE_TILE + (lane & 15);
        const bool ok = row < M;
        const uint64_t m = a.sample_offset + (uint64_t)row;
        f32x4 z[2][NT], x[2][NT];
        double zz = 0.0;
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) {
            const uint32_t b0 = (uint32_t)(8 * tau + 2 * g);
            const f32x4 n0 = importance_normal4(a.seed, m, b0), n1 = importance_normal4(a.seed, m, b0 + 1u);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const f32x4 e = imp_class(n0, n1, c);
                const int d0 = 32 * tau + 8 * g + c;   // component r of class c is dim d0 + 2 r; padded dims stay 0
                f32x4 zc;
                zc.x = d0 < D ? e.x : 0.f;
                zc.y = d0 + 2 < D ? e.y : 0.f;
                zc.z = d0 + 4 < D ? e.z : 0.f;
                zc.w = d0 + 6 < D ? e.w : 0.f;
                z[c][tau] = zc;
                x[c][tau] = zc;
                zz += (double)zc.x * (double)zc.x + (double)zc.y * (double)zc.y + (double)zc.z * (double)zc.z + (double)zc.w * (double)zc.w;
            }
        }
        zz = group_sum(zz);
        double logl;
        const double lp = target(x, logl);
        const double logw = lp - importance_logb(zz, D);
        importance_add(run, logw, ok);
        if (outs && ok && wv == 0) {
            store_tile<NT>(a.z_out, row, true, D, lane, z);
            store_tile<NT>(a.x_out, row, true, D, lane, x);
            if (lane < 16) {
                a.logl_out[row] = logl;
                a.logw_out[row] = logw;
            }
        }
    }
    // over the 16 rows (the four lane groups hold copies): a butterfly with the symmetric merge
#pragma unroll
    for (int sft = 1; sft < 16; sft <<= 1) {
        const ImpSums o = {imp_shfl_xor(run.a, sft), imp_shfl_xor(run.s1, sft), imp_shfl_xor(run.s2, sft), imp_shfl_xor(run.n, sft)};
        run = importance_merge(run, o);
    }
    if (threadIdx.x == 0) importance_publish(a.partials, a.sums, (int)blockIdx.x, run);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH>
static hipError_t spl_imp_launch_t(const ImpArgs &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)spl_imp_lds_floats(q.sp.D, NT) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_importance_kernel_team<NT, NH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_importance_kernel_team<NT, NH>), dim3(a.groups), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// The shapes of the team form of the random-walk kernel (launch_spline_mcmc)
hipError_t launch_spline_importance(const SplArgs &q, const ImpArgs &a, hipStream_t st) {
    if (!spline_shape_supported(q.sp)) return hipErrorInvalidConfiguration;
    switch (q.sp.NTh * 10 + q.sp.NH) {
        case 11: case 21: case 31: case 41: case 12: case 22: break;
        default: return hipErrorInvalidConfiguration;
    }
    if (a.M <= 0 || a.groups <= 0) return hipSuccess;
    switch (q.sp.NTh * 10 + q.sp.NH) {
        case 11: return spl_imp_launch_t<1, 1>(a, q, st);
        case 21: return spl_imp_launch_t<2, 1>(a, q, st);
        case 31: return spl_imp_launch_t<3, 1>(a, q, st);
        case 41: return spl_imp_launch_t<4, 1>(a, q, st);
        case 12: return spl_imp_launch_t<1, 2>(a, q, st);
        case 22: return spl_imp_launch_t<2, 2>(a, q, st);
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
