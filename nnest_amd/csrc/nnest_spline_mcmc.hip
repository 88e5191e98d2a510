// nnest_spline_mcmc.hip -- RANDOM-WALK METROPOLIS in the latent space of the neural-spline flow, every step of a launch in the kernel
// (include/nnest_hip.h nnest_spline_mcmc_steps).  BUILD-DEFINED STREAM, THE REFERENCE'S MOVE.  The definition is nnest_mcmc_steps's
// (nnest_mcmc.hip has it), with the same draws and the same arithmetic (mcmc_walk.h, ensemble_common.h): only the flow differs -- the
// spline's inverse (spline_inverse.h) replaces the coupling stack -- and with it the layout.
//
// Layout: the TEAM tile of nnest_spline_ensemble.hip: 16 walkers per workgroup, four waves per tile.  Every wave carries the same 16
// walkers in the parity-class tiles of flow_tile.h (z, x, lp and logL stay in registers for the launch) and takes the same decisions;
// only the spline evaluations of the inverse are divided between the waves (SplineInverseTeam).  Wave 0 stores.  T's scale and offset
// and the box sit in LDS ([4][32 NT] floats).
//
// A step is ONE tile evaluation in which every live row proposes; rows >= C evaluate their own point and the result is discarded.
// A lane's eight dims of tile column tau, 32 tau + 8 g .. + 7, are exactly the Philox blocks 8 tau + 2 g and 8 tau + 2 g + 1 of its
// walker; the four lane groups of a walker draw different blocks, the four waves the same ones.  The log-det (summed through LDS in
// the same order on every wave, then by group_sum) and the likelihood (loglike_tile) come out bit-identical on the four lane groups
// of a walker and on the four waves, and the accept draw is a function of (walker, step), so the decision is: the waves never
// exchange it (as in ens_tile_walk).  Walkers are independent: no hand-off, no residency limit, no work buffer.  Every wave runs
// every evaluation of the launch, so the team's barriers inside the inverse always meet.
//
// The TEMPERED run (nnest_spline_mcmc_tempered_steps) is the same kernel with the likelihood to the power beta in lp
// (mcmc_target_tempered), a compile-time variant.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_ensemble.hip is: a step loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "mcmc_walk.h"
#include "mh_common.h"
#include "nnest_internal.h"
#include "spline_train_tile.h"

namespace nnest {

#include "spline_inverse.h"

constexpr int SPL_MCMC_TILE = 16;   // walkers per workgroup

// class c of the lane's eight consecutive values v0 (dims 0..3 of its block pair) and v1 (4..7): load_tile's layout
__device__ __forceinline__ f32x4 mcmc_class(const f32x4 &v0, const f32x4 &v1, int c) {
    return c ? (f32x4){v0.y, v0.w, v1.y, v1.w} : (f32x4){v0.x, v0.z, v1.x, v1.z};
}

// The walk of one tile (16 walkers, this wave's copy) through the S steps of a launch.  tpar: [4][32 NT] in LDS -- std, mean, lo, hi
// (padded dims: 0, 0, -inf, +inf).  `writer`: the wave that stores.
// TP: the tempered target at `beta` (mcmc_target_tempered), a compile-time variant; beta is not read otherwise.
template <int NT, bool TP, class Inv>
__device__ __forceinline__ void mcmc_tile_walk(const McmcArgs &a, double beta, int D, int tile, int lane, const Inv &inv, const float *tpar, bool writer) {
    const int S = a.S, C = a.C;
    const int g = lane >> 4;
    const int row = tile * SPL_MCMC_TILE + (lane & 15);
    const bool ok = row < C;
    const bool store = writer && ok;
    const uint64_t w = a.walker_offset + (uint64_t)row;
    const float step = a.step;
    LikeSpec like = a.like;
    like.scale = 1.0f;

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
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
                const f32x4 sd = mcmc_class(s0, s1, c), mu = mcmc_class(m0, m1, c), lo = mcmc_class(l0, l1, c), hi = mcmc_class(h0, h1, c);
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
        if constexpr (TP) return mcmc_target_tempered(logl, ld, in_prior, beta);
        else return ens_target(logl, ld, in_prior, 0, 0.0);
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
            const uint32_t b0 = (uint32_t)(8 * tau + 2 * g);
            const f32x4 n0 = mcmc_normal4(a.seed, w, t, b0), n1 = mcmc_normal4(a.seed, w, t, b0 + 1u);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const f32x4 e = mcmc_class(n0, n1, c);
                const int d0 = 32 * tau + 8 * g + c;   // component r of class c is dim d0 + 2 r; padded dims stay 0
                const f32x4 zc = z[c][tau];
                q[c][tau].x = moving && d0 < D ? mcmc_propose(zc.x, step, e.x) : zc.x;
                q[c][tau].y = moving && d0 + 2 < D ? mcmc_propose(zc.y, step, e.y) : zc.y;
                q[c][tau].z = moving && d0 + 4 < D ? mcmc_propose(zc.z, step, e.z) : zc.z;
                q[c][tau].w = moving && d0 + 6 < D ? mcmc_propose(zc.w, step, e.w) : zc.w;
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

// LDS of the team form (spline_ensemble_kernel_team's): the waves' layout-exchange buffers, the spline exchange, the log-det
// reduction, T
__host__ __device__ inline int spl_mcmc_lds_tpar(int D, int NT) { return ((4 * 16 * (D + 1) + 3) & ~3) + 4 * NT * 64 * 4 + 4 * 16; }
__host__ __device__ inline int spl_mcmc_lds_floats(int D, int NT) { return spl_mcmc_lds_tpar(D, NT) + 4 * 32 * NT; }

// (TP = false: the kernels of nnest_spline_mcmc_steps as they were, instruction for instruction)
template <int NT, int NH, bool TP>
__global__ void __launch_bounds__(256) spline_mcmc_kernel_team(typename McmcArgsOf<TP>::type a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = q.sp.D;
    float *bufs = lds_buf;                                                                 // 4 x 16 x (D+1)
    f32x4 *xch = reinterpret_cast<f32x4 *>(lds_buf + ((4 * 16 * (D + 1) + 3) & ~3));      // 4 x NT x 64 f32x4
    float *ldred = reinterpret_cast<float *>(xch + 4 * NT * 64);                           // 4 x 16
    float *tpar = lds_buf + spl_mcmc_lds_tpar(D, NT);                                      // 4 x 32 NT
    for (int d = threadIdx.x; d < 32 * NT; d += 256) {
        const bool v = d < D;
        tpar[d] = v ? (a.t_std ? a.t_std[d] : 1.f) : 0.f;
        tpar[32 * NT + d] = v && a.t_mean ? a.t_mean[d] : 0.f;
        tpar[2 * 32 * NT + d] = v && a.lo ? a.lo[d] : -INFINITY;
        tpar[3 * 32 * NT + d] = v && a.hi ? a.hi[d] : INFINITY;
    }
    __syncthreads();
    SplineInverseTeam<NT, NH, 4> inv = {q.img, q.sp, bufs + (size_t)wv * 16 * (D + 1), xch, ldred, lane, wv};
    if constexpr (TP) mcmc_tile_walk<NT, true>(a, a.beta, D, blockIdx.x, lane, inv, tpar, wv == 0);
    else mcmc_tile_walk<NT, false>(a, 0.0, D, blockIdx.x, lane, inv, tpar, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, bool TP>
static hipError_t spl_mcmc_launch_t(const typename McmcArgsOf<TP>::type &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)spl_mcmc_lds_floats(q.sp.D, NT) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_mcmc_kernel_team<NT, NH, TP>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_mcmc_kernel_team<NT, NH, TP>), dim3((a.C + SPL_MCMC_TILE - 1) / SPL_MCMC_TILE), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// The shapes of the team form of the ensemble kernel (spl_ens_dispatch)
template <bool TP>
static hipError_t spl_mcmc_dispatch(const SplArgs &q, const typename McmcArgsOf<TP>::type &a, hipStream_t st) {
    if (!spline_shape_supported(q.sp)) return hipErrorInvalidConfiguration;
    if (a.C <= 0) return hipSuccess;
    switch (q.sp.NTh * 10 + q.sp.NH) {
        case 11: return spl_mcmc_launch_t<1, 1, TP>(a, q, st);
        case 21: return spl_mcmc_launch_t<2, 1, TP>(a, q, st);
        case 31: return spl_mcmc_launch_t<3, 1, TP>(a, q, st);
        case 41: return spl_mcmc_launch_t<4, 1, TP>(a, q, st);
        case 12: return spl_mcmc_launch_t<1, 2, TP>(a, q, st);
        case 22: return spl_mcmc_launch_t<2, 2, TP>(a, q, st);
    }
    return hipErrorInvalidConfiguration;
}

hipError_t launch_spline_mcmc(const SplArgs &q, const McmcArgs &a, hipStream_t st) { return spl_mcmc_dispatch<false>(q, a, st); }
hipError_t launch_spline_mcmc_tempered(const SplArgs &q, const McmcTemperedArgs &a, hipStream_t st) {
    return spl_mcmc_dispatch<true>(q, a, st);
}

}  // namespace nnest
