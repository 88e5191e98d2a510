// nnest_spline_mcmc.hip -- RANDOM-WALK METROPOLIS in the latent space of the neural-spline flow, every step of a launch in the kernel
// (include/nnest_hip.h nnest_spline_mcmc_steps).  BUILD-DEFINED STREAM, THE REFERENCE'S MOVE.  The definition is nnest_mcmc_steps's
// (nnest_mcmc.hip has it), with the same draws and the same arithmetic (mcmc_walk.h, ensemble_common.h): only the flow differs -- the
// spline's inverse (spline_inverse.h) replaces the coupling stack -- and with it the layout.
//
// Layout: the TEAM tile of spline_latent.h (which also states the target): 16 walkers per workgroup, four waves per tile.  Every
// wave carries the same 16 walkers in the parity-class tiles of flow_tile.h (z, x, lp and logL stay in registers for the launch) and
// takes the same decisions; only the spline evaluations of the inverse are divided between the waves (SplineInverseTeam).  Wave 0
// stores.  T's scale and offset and the box sit in LDS ([4][32 NT] floats: spl_tile_setup).
//
// A step is ONE tile evaluation in which every live row proposes; rows >= C evaluate their own point and the result is discarded.
// The lane's normals of a tile column: tile_lane_normals (the four lane groups of a walker draw different Philox blocks, the four
// waves the same ones).  The log-det (summed through LDS in the same order on every wave, then by group_sum) and the likelihood
// (loglike_tile) come out bit-identical on the four lane groups of a walker and on the four waves, and the accept draw is a function
// of (walker, step), so the decision is: the waves never exchange it (as in ens_tile_walk).  Walkers are independent: no hand-off,
// no residency limit, no work buffer.  Every wave runs every evaluation of the launch, so the team's barriers inside the inverse
// always meet.
//
// The TEMPERED run (nnest_spline_mcmc_tempered_steps) is the same kernel with the likelihood to the power beta in lp
// (mcmc_target_tempered), a compile-time variant.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_ensemble.hip is: a step loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "mcmc_walk.h"
#include "spline_latent.h"

namespace nnest {

// The walk of one tile (16 walkers, this wave's copy) through the S steps of a launch.  tpar: [4][32 NT] in LDS -- std, mean, lo, hi
// (padded dims: 0, 0, -inf, +inf).  `writer`: the wave that stores.
// TP: the tempered target at `beta` (mcmc_target_tempered), a compile-time variant; beta is not read otherwise.
template <int NT, bool TP, class Inv>
__device__ __forceinline__ void mcmc_tile_walk(const McmcArgs &a, double beta, int D, int tile, int lane, const Inv &inv, const float *tpar, bool writer) {
    const int S = a.S, C = a.C;
    const int g = lane >> 4;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const bool ok = row < C;
    const bool store = writer && ok;
    const uint64_t w = a.walker_offset + (uint64_t)row;
    const float step = a.step;
    LikeSpec like = a.like;
    like.scale = 1.0f;

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](f32x4 (&xs)[2][NT], double &logl) -> double {
        return spl_tile_eval<NT>(inv, tpar, like, D, lane, xs, [&](double l, float ld, bool in_prior) {
            logl = l;
            if constexpr (TP) return mcmc_target_tempered(l, ld, in_prior, beta);
            else return ens_target(l, ld, in_prior, 0, 0.0);
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
    int n_acc = 0;
    const bool hist = a.hist_z != nullptr;
#pragma unroll 1
    for (int i = -1; i < S; ++i) {
        const bool init = i < 0;
        const bool moving = !init && ok;
        const uint32_t t = a.step0 + (uint32_t)i;
        f32x4 q[2][NT], xq[2][NT];
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) {
            f32x4 e[2];
            bool live[2][4];
            tile_lane_normals(tau, g, D, [&](uint32_t b) { return mcmc_normal4(a.seed, w, t, b); }, e, live);
#pragma unroll
            for (int c = 0; c < 2; ++c) {   // (padded dims stay 0)
                const f32x4 zc = z[c][tau];
                q[c][tau].x = moving && live[c][0] ? mcmc_propose(zc.x, step, e[c].x) : zc.x;
                q[c][tau].y = moving && live[c][1] ? mcmc_propose(zc.y, step, e[c].y) : zc.y;
                q[c][tau].z = moving && live[c][2] ? mcmc_propose(zc.z, step, e[c].z) : zc.z;
                q[c][tau].w = moving && live[c][3] ? mcmc_propose(zc.w, step, e[c].w) : zc.w;
                xq[c][tau] = q[c][tau];
            }
        }
        const float uacc = mcmc_uniform(a.seed, w, t);
        double loglq;
        const double lpq = target(xq, loglq);
        const bool acc = moving && ens_accept_factor(lpq, lp, 0.0, uacc);
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
    }
}

// (TP = false: the kernels of nnest_spline_mcmc_steps)
template <int NT, int NH, bool TP>
__global__ void __launch_bounds__(256) spline_mcmc_kernel_team(typename McmcArgsOf<TP>::type a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    if constexpr (TP) mcmc_tile_walk<NT, true>(a, a.beta, q.sp.D, blockIdx.x, lane, t.inv, t.tpar, wv == 0);
    else mcmc_tile_walk<NT, false>(a, 0.0, q.sp.D, blockIdx.x, lane, t.inv, t.tpar, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, bool TP>
static hipError_t spl_mcmc_launch_t(const typename McmcArgsOf<TP>::type &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)spl_tile_lds_floats(q.sp.D, NT) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_mcmc_kernel_team<NT, NH, TP>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_mcmc_kernel_team<NT, NH, TP>), dim3((a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

template <bool TP>
static hipError_t spl_mcmc_dispatch(const SplArgs &q, const typename McmcArgsOf<TP>::type &a, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        return a.C <= 0 ? hipSuccess : spl_mcmc_launch_t<decltype(sh)::NT, decltype(sh)::NH, TP>(a, q, st);
    });
}

hipError_t launch_spline_mcmc(const SplArgs &q, const McmcArgs &a, hipStream_t st) { return spl_mcmc_dispatch<false>(q, a, st); }
hipError_t launch_spline_mcmc_tempered(const SplArgs &q, const McmcTemperedArgs &a, hipStream_t st) {
    return spl_mcmc_dispatch<true>(q, a, st);
}

}  // namespace nnest
