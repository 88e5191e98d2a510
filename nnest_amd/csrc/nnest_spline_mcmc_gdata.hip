// nnest_spline_mcmc_gdata.hip -- the ADAPTIVE WALK in the latent space of the neural-spline flow on a GAUSSIAN LIKELIHOOD FROM USER
// DATA: nnest_spline_mcmc_adapt_steps's run (nnest_spline_mcmc_adapt.hip) with logL(t) = logl0 - 1/2 |R (t - mu)|^2 compiled in, in a
// kernel of its own (include/nnest_hip.h nnest_spline_mcmc_gdata_steps).  BUILD-DEFINED.  The definition is
// nnest_mcmc_gdata_steps's (nnest_mcmc_gdata.hip): only the flow differs, and with it the layout.
//
// Layout: mcmc_adapt_tile_walk's, the TEAM tile of spline_latent.h, 16 walkers per workgroup, four waves carrying the same 16
// walkers.  y = d R^T of the tile's 16 walkers is a product on the matrix cores (mcmc_gdata.h gdata_tile_loglike), computed whole by
// every wave: the waves stay bit-identical without an exchange.  mu sits in LDS behind the tile's own buffers.  Wave 0 stores.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mcmc_adapt.hip is: a step loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "mcmc_gdata.h"
#include "spline_latent.h"

namespace nnest {

// x <- f^-1(x) in place; returns combine(logL(T(x)), ld, in_prior): spl_tile_eval (spline_latent.h) on spl_tile_map, with the likelihood
// of mcmc_gdata.h behind T and the box
template <int NT, class Inv, class Combine>
__device__ __forceinline__ double gdata_tile_eval(const Inv &inv, const float *tpar, const GdataSpec &gd, const float *gmu, int lane,
                                                  f32x4 (&xs)[2][NT], Combine &&combine) {
    const float ld = group_sum(inv(xs));
    f32x4 tx[2][NT];
    const bool in_prior = spl_tile_map<NT>(tpar, lane, xs, tx);
    const double logl = gdata_tile_loglike<NT>(gd, lane, tx, gmu);
    return combine(logl, ld, in_prior);
}

// The walk of one tile (16 walkers, this wave's copy) through the S steps of a launch: mcmc_adapt_tile_walk with the target above.
// tpar: [4][32 NT] in LDS -- std, mean, lo, hi; gmu: [32 NT] in LDS.  `writer`: the wave that stores.
template <int NT, class Inv>
__device__ __forceinline__ void mcmc_gdata_tile_walk(const McmcGdataArgs &a, int D, int tile, int lane, const Inv &inv, const float *tpar,
                                                     const float *gmu, bool writer) {
    const int S = a.S, C = a.C;
    const int g = lane >> 4;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const bool ok = row < C;
    const bool store = writer && ok;
    const uint64_t w = a.walker_offset + (uint64_t)row;
    // the walker's step: float64 between the steps, rounded to float32 where the proposal uses it
    double sigma = a.step_in && ok ? adapt_clamp(a.step_in[row]) : (double)a.step;
    const double beta = a.beta;
    const GdataSpec gd = a.gd;
    MixedPhase phase;
    phase.init(a.step0, a.global_every);

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](f32x4 (&xs)[2][NT], double &logl) -> double {
        return gdata_tile_eval<NT>(inv, tpar, gd, gmu, lane, xs, [&](double l, float ld, bool in_prior) {
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
        const double lpq = target(xq, loglq);
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

template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_mcmc_gdata_kernel_team(McmcGdataArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // mu behind the tile's buffers: [32 NT], padded dims 0 (spl_tile_setup's barrier covers it)
    float *gmu = lds_buf + spl_tile_lds_floats(q.sp.D, NT);
    for (int d = threadIdx.x; d < 32 * NT; d += 256) gmu[d] = d < q.sp.D ? a.gd.mu[d] : 0.f;
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    mcmc_gdata_tile_walk<NT>(a, q.sp.D, blockIdx.x, lane, t.inv, t.tpar, gmu, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH>
static hipError_t spl_mcmc_gdata_launch_t(const McmcGdataArgs &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)(spl_tile_lds_floats(q.sp.D, NT) + 32 * NT) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_mcmc_gdata_kernel_team<NT, NH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_mcmc_gdata_kernel_team<NT, NH>), dim3((a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// (a shape's verdict comes before C: nnest_spline_mcmc_gdata_check asks with C = 0)
hipError_t launch_spline_mcmc_gdata(const SplArgs &q, const McmcGdataArgs &a, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        return a.C <= 0 ? hipSuccess : spl_mcmc_gdata_launch_t<decltype(sh)::NT, decltype(sh)::NH>(a, q, st);
    });
}

}  // namespace nnest
