// nnest_spline_importance_glm.hip -- IMPORTANCE-SAMPLED EVIDENCE of a GENERALISED LINEAR MODEL of the user's data from the trained
// neural-spline flow (include/nnest_hip.h nnest_spline_importance_glm_evidence).  BUILD-DEFINED.  The definition is
// nnest_importance_glm_evidence's (nnest_importance_glm.hip), with the same draws, base density, sums and merge (importance_walk.h):
// only the flow differs, and with it the layout.
//
// Layout: spline_importance_kernel_team's, the TEAM tile of spline_latent.h, 16 samples per workgroup and pass, four waves carrying
// the same 16 samples, a PERSISTENT grid: workgroup b takes tiles b, b + groups, ...  That unit stays what it is, and its loop and
// its evaluation are restated here.  eta = A t^T of the tile's 16 samples is a product on the matrix cores whose row blocks the
// four waves SHARE (glm_data.h glm_tile_loglike); the waves' float64 partials meet in LDS behind the tile's own buffers, in two
// [4][16] arrays of doubles.  The prior's m and r are staged ONCE per workgroup in LDS behind them -- [2][32 NT] floats, padded dims
// 0 --, in front of spl_tile_setup's barrier, and read per evaluation as tpar is (nnest_spline_mcmc_glm_prior.hip).
//
// THE BARRIER of glm_tile_loglike always meets: the tile index is the workgroup's, not the wave's, so every wave of a workgroup
// runs the same number of passes; rows >= M of the last tile evaluate their point (the sample one past the launch's) and are
// neither counted nor written; no wave leaves before the loop's end.  ONE barrier an evaluation is enough because consecutive
// passes ALTERNATE between the two arrays of partials (nnest_spline_mcmc_glm.hip has the argument: a wave that writes array k & 1
// in pass k has passed the barrier of pass k - 1, which every wave reaches only after it has read the partials of pass k - 2).
// The prior term needs no exchange: each wave sums the full ss of its own copy of the tile.
//
// Reduction: spline_importance_kernel_team's -- lane (g, r) keeps the running sums of the samples that came through row r, the four
// waves hold identical sums, a butterfly over the 16 rows with the symmetric merge, and ONE wave publishes.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_importance.hip is: a loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "importance_glm.h"
#include "spline_latent.h"

namespace nnest {

__device__ __forceinline__ double impg_shfl_xor(double v, int mask) { return __shfl_xor(v, mask); }

// x <- f^-1(x) in place; returns combine(logL(T(x)), ld, in_box, log pi(T(x))): glmp_tile_eval (nnest_spline_mcmc_glm_prior.hip),
// restated; PRIOR = false: log pi is 0.0 and ppar is not read.  part: this evaluation's [4][16] doubles in LDS; ppar: [2][32 NT]
template <int NT, int FAM, bool PRIOR, class Inv, class Combine>
__device__ __forceinline__ double impg_tile_eval(const Inv &inv, const float *tpar, const float *ppar, const GlmSpec &gl, double logc,
                                                 double *part, int lane, int wv, f32x4 (&xs)[2][NT], Combine &&combine) {
    const int g = lane >> 4;
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
            const f32x4 sd = tile_class(s0, s1, c), mu = tile_class(m0, m1, c), lo = tile_class(l0, l1, c), hi = tile_class(h0, h1, c);
            f32x4 t;
            t.x = ens_T(xs[c][tau].x, sd.x, mu.x); t.y = ens_T(xs[c][tau].y, sd.y, mu.y);
            t.z = ens_T(xs[c][tau].z, sd.z, mu.z); t.w = ens_T(xs[c][tau].w, sd.w, mu.w);
            // (NaN counts as inside: UniformPrior, priors.py)
            inside &= !(t.x < lo.x || t.x > hi.x) & !(t.y < lo.y || t.y > hi.y) & !(t.z < lo.z || t.z > hi.z) & !(t.w < lo.w || t.w > hi.w);
            tx[c][tau] = t;
        }
    }
    const bool in_box = group_all(inside != 0, lane) != 0;
    double logpi = 0.0;
    if constexpr (PRIOR) logpi = gauss_prior_tile<NT>(tx, ppar, g, logc);
    const double logl = glm_tile_loglike<NT, FAM>(gl, lane, wv, tx, part);
    return combine(logl, ld, in_box, logpi);
}

// behind the tile's buffers (spl_tile_lds_floats is a multiple of 4 floats: 16 bytes): the doubles of the two arrays of partials,
// then the prior's m and r, [2][32 NT] floats
constexpr int IMPG_PART_FLOATS = 2 * 4 * 16 * 2;
__host__ __device__ inline int impg_prior_floats(int NT) { return 2 * 32 * NT; }

template <int NT, int NH, int FAM, bool PRIOR>
__global__ void __launch_bounds__(256) spline_importance_glm_kernel_team(ImpGlmArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = q.sp.D, M = a.M;
    double *parts = reinterpret_cast<double *>(lds_buf + spl_tile_lds_floats(D, NT));
    float *ppar = lds_buf + spl_tile_lds_floats(D, NT) + IMPG_PART_FLOATS;
    if constexpr (PRIOR) {
        // (staged in front of spl_tile_setup's barrier, which orders these writes before every read; nothing writes ppar again)
        for (int d = threadIdx.x; d < 32 * NT; d += 256) {
            const bool v = d < D;
            ppar[d] = v ? a.pr.m[d] : 0.f;
            ppar[32 * NT + d] = v ? a.pr.r[d] : 0.f;
        }
    }
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    const int g = lane >> 4;
    const double logc = PRIOR ? a.pr.logc : 0.0;
    const GlmSpec gl = a.gl;

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`.  `flip`: which of the two arrays of partials
    auto target = [&](f32x4 (&xs)[2][NT], double &logl, int flip) -> double {
        return impg_tile_eval<NT, FAM, PRIOR>(t.inv, t.tpar, ppar, gl, logc, parts + 64 * flip, lane, wv, xs,
                                              [&](double l, float ld, bool in_box, double logpi) {
                                                  logl = l;
                                                  if constexpr (PRIOR) return mcmc_target_tempered_prior(l, ld, true, logpi, 1.0);
                                                  else return ens_target(l, ld, in_box, 0, 0.0);
                                              });
    };

    const bool outs = a.z_out != nullptr;
    const int ntiles = (M + IMP_SPLINE_TILE - 1) / IMP_SPLINE_TILE;
    ImpSums run = importance_empty();
    int flip = 0;
#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {   // (uniform over the workgroup: the barriers meet)
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
        const double lp = target(x, logl, flip);
        flip ^= 1;
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
        const ImpSums o = {impg_shfl_xor(run.a, sft), impg_shfl_xor(run.s1, sft), impg_shfl_xor(run.s2, sft), impg_shfl_xor(run.n, sft)};
        run = importance_merge(run, o);
    }
    if (threadIdx.x == 0) importance_publish(a.partials, a.sums, (int)blockIdx.x, run);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, int FAM, bool PRIOR>
static hipError_t spl_imp_glm_launch_t(const ImpGlmArgs &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)(spl_tile_lds_floats(q.sp.D, NT) + IMPG_PART_FLOATS + impg_prior_floats(NT)) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_importance_glm_kernel_team<NT, NH, FAM, PRIOR>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_importance_glm_kernel_team<NT, NH, FAM, PRIOR>), dim3(a.groups), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// (a shape's verdict comes before M: nnest_spline_importance_glm_check asks with M = 0)
hipError_t launch_spline_importance_glm(const SplArgs &q, const ImpGlmArgs &a, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        constexpr int NT = decltype(sh)::NT, NH = decltype(sh)::NH;
        if (a.M <= 0 || a.groups <= 0) return hipSuccess;
        switch (a.gl.family) {
            case GLM_LOGISTIC:
                return a.prior ? spl_imp_glm_launch_t<NT, NH, GLM_LOGISTIC, true>(a, q, st)
                               : spl_imp_glm_launch_t<NT, NH, GLM_LOGISTIC, false>(a, q, st);
            case GLM_POISSON:
                return a.prior ? spl_imp_glm_launch_t<NT, NH, GLM_POISSON, true>(a, q, st)
                               : spl_imp_glm_launch_t<NT, NH, GLM_POISSON, false>(a, q, st);
        }
        return hipErrorInvalidConfiguration;
    });
}

}  // namespace nnest
