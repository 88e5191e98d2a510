// nnest_spline_mcmc_glm_prior.hip -- the ADAPTIVE WALK in the latent space of the neural-spline flow on a GENERALISED LINEAR MODEL of
// the user's data UNDER INDEPENDENT NORMAL PRIORS on the coefficients: nnest_spline_mcmc_glm_steps's run (nnest_spline_mcmc_glm.hip)
// with log pi of gauss_prior.h in the target where that kernel adds 0.0, in a kernel of its own (include/nnest_hip.h
// nnest_spline_mcmc_glm_prior_steps).  BUILD-DEFINED.  The definition is nnest_mcmc_glm_prior_steps's
// (nnest_mcmc_glm_prior.hip): only the flow differs, and with it the layout.
//
// Layout: mcmc_glm_tile_walk's, the TEAM tile of spline_latent.h, 16 walkers per workgroup, four waves carrying the same 16 walkers;
// that unit stays what it is, and its walk and its evaluation are restated here.  The prior's m and r are staged ONCE per workgroup
// in LDS BEHIND the two [4][16] arrays of float64 partials -- [2][32 NT] floats, padded dims 0 --, in front of spl_tile_setup's own
// barrier, and read per evaluation as tpar is (registers: at NT = 2 the likelihood's second operand set already goes to AGPRs,
// glm_data.h; 16 NT more live values across the inverse would follow it).  spl_tile_setup, spl_tile_lds_floats and tpar's [4][32 NT]
// stay as they are.
//
// THE BARRIER ARGUMENT of nnest_spline_mcmc_glm.hip still holds, because the evaluation count per wave is unchanged: the prior term
// needs no exchange between the waves -- each wave sums the full ss of its own copy of the tile (group_sum over a walker's four
// lane groups), so the four waves hold the same bits of log pi --, it adds no __syncthreads(), and it neither writes LDS after
// the setup's barrier nor touches the arrays of partials.  Every wave of a workgroup still runs the same loop and reaches the one
// barrier of each evaluation (glm_tile_loglike's) the same number of times, and consecutive evaluations still alternate between the
// two arrays.  Wave 0 stores.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mcmc_glm.hip is: a step loop around the same inverse.
#include <stdio.h>
#include <string.h>

#include "gauss_prior.h"
#include "spline_latent.h"

namespace nnest {

// x <- f^-1(x) in place; returns combine(logL(T(x)), ld, in_box, log pi(T(x))): glm_tile_eval (nnest_spline_mcmc_glm.hip), restated on spl_tile_map
// with the prior term of gauss_prior.h beside the likelihood.  part: this evaluation's [4][16] doubles in LDS; ppar: [2][32 NT] in LDS
template <int NT, int FAM, class Inv, class Combine>
__device__ __forceinline__ double glmp_tile_eval(const Inv &inv, const float *tpar, const float *ppar, const GlmSpec &gl, double logc,
                                                 double *part, int lane, int wv, f32x4 (&xs)[2][NT], Combine &&combine) {
    const int g = lane >> 4;
    const float ld = group_sum(inv(xs));
    f32x4 tx[2][NT];
    const bool in_box = spl_tile_map<NT>(tpar, lane, xs, tx);
    const double logpi = gauss_prior_tile<NT>(tx, ppar, g, logc);
    const double logl = glm_tile_loglike<NT, FAM>(gl, lane, wv, tx, part);
    return combine(logl, ld, in_box, logpi);
}

// The walk of one tile (16 walkers, this wave's copy) through the S steps of a launch: mcmc_glm_tile_walk with the target above.
// tpar: [4][32 NT] in LDS -- std, mean, lo, hi; parts: [2][4][16] doubles in LDS; ppar: [2][32 NT] in LDS -- the prior's m, r.
// `writer`: the wave that stores.
template <int NT, int FAM, class Inv>
__device__ __forceinline__ void mcmc_glm_prior_tile_walk(const McmcGlmPriorArgs &a, int D, int tile, int lane, int wv, const Inv &inv,
                                                         const float *tpar, double *parts, const float *ppar, bool writer) {
    const int S = a.S, C = a.C;
    const int g = lane >> 4;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const bool ok = row < C;
    const bool store = writer && ok;
    const uint64_t w = a.walker_offset + (uint64_t)row;
    // the walker's step: float64 between the steps, rounded to float32 where the proposal uses it
    double sigma = a.step_in && ok ? adapt_clamp(a.step_in[row]) : (double)a.step;
    const double beta = a.beta, logc = a.pr.logc;
    const GlmSpec gl = a.gl;
    MixedPhase phase;
    phase.init(a.step0, a.global_every);

    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`.  `flip`: which of the two arrays of partials
    auto target = [&](f32x4 (&xs)[2][NT], double &logl, int flip) -> double {
        return glmp_tile_eval<NT, FAM>(inv, tpar, ppar, gl, logc, parts + 64 * flip, lane, wv, xs,
                                       [&](double l, float ld, bool in_box, double logpi) {
                                           logl = l;
                                           return mcmc_target_tempered_prior(l, ld, in_box, logpi, beta);
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

// behind the tile's buffers (spl_tile_lds_floats is a multiple of 4 floats: 16 bytes): the doubles of the two arrays of partials,
// then the prior's m and r, [2][32 NT] floats
constexpr int GLMP_PART_FLOATS = 2 * 4 * 16 * 2;
__host__ __device__ inline int glmp_prior_floats(int NT) { return 2 * 32 * NT; }

template <int NT, int NH, int FAM>
__global__ void __launch_bounds__(256) spline_mcmc_glm_prior_kernel_team(McmcGlmPriorArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double *parts = reinterpret_cast<double *>(lds_buf + spl_tile_lds_floats(q.sp.D, NT));
    float *ppar = lds_buf + spl_tile_lds_floats(q.sp.D, NT) + GLMP_PART_FLOATS;
    // (staged in front of spl_tile_setup's barrier, which orders these writes before every read; nothing writes ppar again)
    for (int d = threadIdx.x; d < 32 * NT; d += 256) {
        const bool v = d < q.sp.D;
        ppar[d] = v ? a.pr.m[d] : 0.f;
        ppar[32 * NT + d] = v ? a.pr.r[d] : 0.f;
    }
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    mcmc_glm_prior_tile_walk<NT, FAM>(a, q.sp.D, blockIdx.x, lane, wv, t.inv, t.tpar, parts, ppar, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, int FAM>
static hipError_t spl_mcmc_glm_prior_launch_t(const McmcGlmPriorArgs &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)(spl_tile_lds_floats(q.sp.D, NT) + GLMP_PART_FLOATS + glmp_prior_floats(NT)) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_mcmc_glm_prior_kernel_team<NT, NH, FAM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_mcmc_glm_prior_kernel_team<NT, NH, FAM>), dim3((a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS), dim3(256), lds,
                       st, a, q);
    return hipGetLastError();
}

// (a shape's verdict comes before C: nnest_spline_mcmc_glm_prior_check asks with C = 0)
hipError_t launch_spline_mcmc_glm_prior(const SplArgs &q, const McmcGlmPriorArgs &a, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        constexpr int NT = decltype(sh)::NT, NH = decltype(sh)::NH;
        if (a.C <= 0) return hipSuccess;
        switch (a.gl.family) {
            case GLM_LOGISTIC: return spl_mcmc_glm_prior_launch_t<NT, NH, GLM_LOGISTIC>(a, q, st);
            case GLM_POISSON: return spl_mcmc_glm_prior_launch_t<NT, NH, GLM_POISSON>(a, q, st);
        }
        return hipErrorInvalidConfiguration;
    });
}

}  // namespace nnest
