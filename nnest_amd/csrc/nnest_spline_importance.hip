// nnest_spline_importance.hip -- IMPORTANCE-SAMPLED EVIDENCE from the trained neural-spline flow (include/nnest_hip.h
// nnest_spline_importance_evidence).  BUILD-DEFINED.  The definition is nnest_importance_evidence's (nnest_importance.hip has it), with
// the same draws, base density, sums and merge (importance_walk.h): only the flow differs -- the spline's inverse (spline_inverse.h)
// replaces the coupling stack -- and with it the layout.
//
// Layout: the TEAM tile of spline_latent.h (which also states the target): 16 samples per workgroup and pass, four waves per tile.
// Every wave carries the same 16 samples in the parity-class tiles of flow_tile.h; only the spline evaluations of the inverse are
// divided between the waves (SplineInverseTeam).  The grid is PERSISTENT: workgroup b takes tiles b, b + groups, ...; T's scale and
// offset and the box are put in LDS once (spl_tile_setup).  The lane's normals: tile_lane_normals, as mcmc_tile_walk draws its eps.
// Rows >= M of the last tile evaluate their point (the sample one past the launch's) and are neither counted nor written.  Every
// wave runs every tile of its workgroup, so the team's barriers inside the inverse always meet.
//
// Reduction: lane (g, r) keeps the running sums of the samples that came through row r; log-det and likelihood are bit-identical on
// the four lane groups and on the four waves (nnest_spline_mcmc.hip), so the four waves hold identical sums.  At the end a butterfly
// over the 16 rows with the symmetric merge leaves every lane with the same bits, and wave 0 publishes.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mcmc.hip is: a loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "importance_walk.h"
#include "spline_latent.h"

namespace nnest {

__device__ __forceinline__ double imp_shfl_xor(double v, int mask) { return __shfl_xor(v, mask); }

template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_importance_kernel_team(ImpArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = q.sp.D, M = a.M;
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    const int g = lane >> 4;
    LikeSpec like = a.like;
    like.scale = 1.0f;

    // x <- f^-1(x) in place; returns lp (nnest_spline_mcmc_steps's), and logL(T(x)) through `logl`
    auto target = [&](f32x4 (&xs)[2][NT], double &logl) -> double {
        return spl_tile_eval<NT>(t.inv, t.tpar, like, D, lane, xs, [&](double l, float ld, bool in_prior) {
            logl = l;
            return ens_target(l, ld, in_prior, 0, 0.0);
        });
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
            f32x4 e[2];
            bool live[2][4];
            tile_lane_normals(tau, g, D, [&](uint32_t b) { return importance_normal4(a.seed, m, b); }, e, live);
#pragma unroll
            for (int c = 0; c < 2; ++c) {   // (padded dims stay 0)
                f32x4 zc;
                zc.x = live[c][0] ? e[c].x : 0.f;
                zc.y = live[c][1] ? e[c].y : 0.f;
                zc.z = live[c][2] ? e[c].z : 0.f;
                zc.w = live[c][3] ? e[c].w : 0.f;
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
    const size_t lds = (size_t)spl_tile_lds_floats(q.sp.D, NT) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_importance_kernel_team<NT, NH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_importance_kernel_team<NT, NH>), dim3(a.groups), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// (a shape's verdict comes before M: nnest_spline_importance_check asks with M = 0)
hipError_t launch_spline_importance(const SplArgs &q, const ImpArgs &a, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        return a.M <= 0 || a.groups <= 0 ? hipSuccess : spl_imp_launch_t<decltype(sh)::NT, decltype(sh)::NH>(a, q, st);
    });
}

}  // namespace nnest
