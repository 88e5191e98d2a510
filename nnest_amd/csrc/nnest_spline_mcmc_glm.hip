// nnest_spline_mcmc_glm.hip -- the ADAPTIVE WALK in the latent space of the neural-spline flow on a GENERALISED LINEAR MODEL of the
// user's data (logistic or Poisson regression): nnest_spline_mcmc_adapt_steps's run (nnest_spline_mcmc_adapt.hip) with the
// likelihood of glm_data.h compiled in, in a kernel of its own (include/nnest_hip.h nnest_spline_mcmc_glm_steps).
// BUILD-DEFINED.  The definition is nnest_mcmc_glm_steps's (nnest_mcmc_glm.hip): only the flow differs, and with it the layout.
//
// Layout: mcmc_gdata_tile_walk's, the TEAM tile of spline_latent.h, 16 walkers per workgroup, four waves carrying the same 16
// walkers.  eta = A t^T of the tile's 16 walkers is a product on the matrix cores (glm_data.h glm_tile_loglike) whose row blocks
// the four waves SHARE; the waves' float64 partials meet in LDS behind the tile's own buffers: two [4][16] arrays of doubles.
//
// THE BARRIER of that exchange always meets: every wave of a workgroup runs the same loop -- S and the walk's schedule are launch
// arguments, a walker past C or one that does not move is evaluated all the same, and no wave leaves the kernel before the loop's
// end --, so all 256 threads reach every evaluation's __syncthreads(), the same number of times.
// ONE barrier an evaluation is enough because consecutive evaluations ALTERNATE between the two arrays: a wave that writes
// array k & 1 in evaluation k has passed the barrier of evaluation k - 1, which every wave reaches only after it has read the
// partials of evaluation k - 2 -- the last use of that array.  (The writes of evaluation k are ordered before its reads by its
// own barrier; __syncthreads() waits for the LDS writes in flight.)
// Wave 0 stores.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mcmc_adapt.hip is: a step loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "glm_data.h"
#include "spline_latent.h"

namespace nnest {

// x <- f^-1(x) in place; returns combine(logL(T(x)), ld, in_prior): spl_tile_eval (spline_latent.h) on spl_tile_map, with the likelihood
// of glm_data.h behind T and the box.  part: this evaluation's [4][16] doubles in LDS
template <int NT, int FAM, class Inv, class Combine>
__device__ __forceinline__ double glm_tile_eval(const Inv &inv, const float *tpar, const GlmSpec &gl, double *part, int lane, int wv,
                                                f32x4 (&xs)[2][NT], Combine &&combine) {
    const float ld = group_sum(inv(xs));
    f32x4 tx[2][NT];
    const bool in_prior = spl_tile_map<NT>(tpar, lane, xs, tx);
    const double logl = glm_tile_loglike<NT, FAM>(gl, lane, wv, tx, part);
    return combine(logl, ld, in_prior);
}

// The walk of one tile (16 walkers, this wave's copy) through the S steps of a launch: mcmc_gdata_tile_walk with the target above.
// tpar: [4][32 NT] in LDS -- std, mean, lo, hi; parts: [2][4][16] doubles in LDS.  `writer`: the wave that stores.
template <int NT, int FAM, class Inv>
__device__ __forceinline__ void mcmc_glm_tile_walk(const McmcGlmArgs &a, int D, int tile, int lane, int wv, const Inv &inv, const float *tpar,
                                                   double *parts, bool writer) {
    const int S = a.S, C = a.C;
    const int g = lane >> 4;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const bool ok = row < C;
    const bool store = writer && ok;
    const uint64_t w = a.walker_offset + (uint64_t)row;
    // the walker's step: float64 between the steps, rounded to float32 where the proposal uses it
    double sigma = a.step_in && ok ? adapt_clamp(a.step_in[row]) : (double)a.step;
    const double beta = a.beta;
    const GlmSpec gl = a.gl;
    MixedPhase phase;
    phase.init(a.step0, a.global_every);

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`.  `flip`: which of the two arrays of partials
    auto target = [&](f32x4 (&xs)[2][NT], double &logl, int flip) -> double {
        return glm_tile_eval<NT, FAM>(inv, tpar, gl, parts + 64 * flip, lane, wv, xs, [&](double l, float ld, bool in_prior) {
            logl = l;
            return mcmc_target_tempered(l, ld, in_prior, beta);
        });
    };

    // ONE loop over the launch's evaluations, so that the inverse is inlined once: i = -1 is the start (nobody moves, every walker
    // takes its own point's x, lp and logL), then the steps
    f32x4 z[2][NT], x[2][NT];
    load_tile<NT>(a.z_in, row, ok, D, lane, z);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < NT; ++t) x[c][t] = z[c][t];
    double lp = 0.0, logl = 0.0;
    int n_acc = 0, n_acc_g = 0;
    const bool hist = a.hist_z != nullptr;
#pragma unroll 1
    for (int i = -1; i < S; ++i) {
        const bool init = i < 0;
        const bool moving = !init && ok;
        const uint32_t t = a.step0 + (uint32_t)i;
        const bool glob = !init && phase.next_is_global();
        f32x4 q[2][NT], xq[2][NT];
        const float step = (float)sigma;
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) {
            f32x4 e[2];
            bool live[2][4];
            tile_lane_normals(tau, g, D, [&](uint32_t b) { return mcmc_normal4(a.seed, w, t, b); }, e, live);
#pragma unroll
            for (int c = 0; c < 2; ++c) {   // (padded dims stay 0)
                const f32x4 zc = z[c][tau];
                const float qx = mcmc_propose(zc.x, step, e[c].x), qy = mcmc_propose(zc.y, step, e[c].y);
                const float qz = mcmc_propose(zc.z, step, e[c].z), qw = mcmc_propose(zc.w, step, e[c].w);
                q[c][tau].x = moving && live[c][0] ? (glob ? e[c].x : qx) : zc.x;
                q[c][tau].y = moving && live[c][1] ? (glob ? e[c].y : qy) : zc.y;
                q[c][tau].z = moving && live[c][2] ? (glob ? e[c].z : qz) : zc.z;
                q[c][tau].w = moving && live[c][3] ? (glob ? e[c].w : qw) : zc.w;
                xq[c][tau] = q[c][tau];
            }
        }
        const float uacc = mcmc_uniform(a.seed, w, t);
        double loglq;
        const double lpq = target(xq, loglq, i & 1);
        // the two sides of the accept rule: lp on a local step, the log importance weight on a global one
        double lnew = lpq, lold = lp;
        if (glob) {
            lnew = mixed_logw(lpq, tile_row_zz<NT>(q), D);
            lold = mixed_logw(lp, tile_row_zz<NT>(z), D);
        }
        const bool acc = moving && ens_accept_factor(lnew, lold, 0.0, uacc);
        const bool take = acc || init;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                z[c][tt].x = take ? q[c][tt].x : z[c][tt].x; z[c][tt].y = take ? q[c][tt].y : z[c][tt].y;
                z[c][tt].z = take ? q[c][tt].z : z[c][tt].z; z[c][tt].w = take ? q[c][tt].w : z[c][tt].w;
                x[c][tt].x = take ? xq[c][tt].x : x[c][tt].x; x[c][tt].y = take ? xq[c][tt].y : x[c][tt].y;
                x[c][tt].z = take ? xq[c][tt].z : x[c][tt].z; x[c][tt].w = take ? xq[c][tt].w : x[c][tt].w;
            }
        lp = take ? lpq : lp;
        logl = take ? loglq : logl;
        if (init && a.lp_in && ok) { lp = a.lp_in[row]; logl = a.logl_in[row]; }
        n_acc += acc ? 1 : 0;
        n_acc_g += acc && glob ? 1 : 0;
        if (moving && !glob && t < a.adapt_steps) sigma = adapt_update(sigma, t, acc, a.adapt_rate, a.target_accept);
        if (store && a.hist_step && !init && lane < 16) a.hist_step[(long)row * S + i] = sigma;
        if (store && hist && !init) {
            const long hr = (long)row * S + i;
            store_tile<NT>(a.hist_z, hr, true, D, lane, z);
            store_tile<NT>(a.hist_x, hr, true, D, lane, x);
            if (lane < 16) a.hist_logl[hr] = logl;
        }
    }
    if (!store) return;
    if (S > 0) store_tile<NT>(a.z_out, row, true, D, lane, z);   // (steps = 0 evaluates the start: x, lp and logL only)
    store_tile<NT>(a.x_out, row, true, D, lane, x);
    if (lane < 16) {
        a.lp_out[row] = lp;
        a.logl_out[row] = logl;
        if (S > 0 && a.n_accept) a.n_accept[row] = n_acc;
        if (S > 0 && a.n_accept_global) a.n_accept_global[row] = n_acc_g;
        if (S > 0 && a.step_out) a.step_out[row] = sigma;
    }
}

// the doubles of the two arrays of partials, behind the tile's buffers (spl_tile_lds_floats is a multiple of 4 floats: 16 bytes)
constexpr int GLM_PART_FLOATS = 2 * 4 * 16 * 2;

template <int NT, int NH, int FAM>
__global__ void __launch_bounds__(256) spline_mcmc_glm_kernel_team(McmcGlmArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double *parts = reinterpret_cast<double *>(lds_buf + spl_tile_lds_floats(q.sp.D, NT));
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    mcmc_glm_tile_walk<NT, FAM>(a, q.sp.D, blockIdx.x, lane, wv, t.inv, t.tpar, parts, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, int FAM>
static hipError_t spl_mcmc_glm_launch_t(const McmcGlmArgs &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)(spl_tile_lds_floats(q.sp.D, NT) + GLM_PART_FLOATS) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_mcmc_glm_kernel_team<NT, NH, FAM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_mcmc_glm_kernel_team<NT, NH, FAM>), dim3((a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// (a shape's verdict comes before C: nnest_spline_mcmc_glm_check asks with C = 0)
hipError_t launch_spline_mcmc_glm(const SplArgs &q, const McmcGlmArgs &a, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        constexpr int NT = decltype(sh)::NT, NH = decltype(sh)::NH;
        if (a.C <= 0) return hipSuccess;
        switch (a.gl.family) {
            case GLM_LOGISTIC: return spl_mcmc_glm_launch_t<NT, NH, GLM_LOGISTIC>(a, q, st);
            case GLM_POISSON: return spl_mcmc_glm_launch_t<NT, NH, GLM_POISSON>(a, q, st);
        }
        return hipErrorInvalidConfiguration;
    });
}

}  // namespace nnest
