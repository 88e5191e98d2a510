// nnest_spline_mh_glm.hip -- the constrained METROPOLIS proposal in latent space of the neural-spline flow on a GENERALISED LINEAR
// MODEL of the user's data (logistic or Poisson regression): K4's hard-constraint step (mh_body.h; reference sampler.py:229-463) with
//   logL(x) := GLM(T(x)),  T(x)_d = ens_T(x_d, t_std[d], t_mean[d])  (spl_tile_map; NULL t_std / t_mean: the identity)
// and the likelihood of glm_data.h compiled in, in a kernel of its own (include/nnest_hip.h nnest_spline_mh_glm_steps; DESIGN.md
// 3.23).  The definition is nnest_mh_glm_steps's (nnest_mh_glm.hip has it, operation for operation): only the flow differs, and with
// it the layout.  The box is on x (inbox_tile), NOT on T(x): the map gets no lo / hi.
//
// Layout: the TEAM tile of spline_latent.h, 16 walkers per workgroup, four waves carrying the same 16 walkers -- the only form:
// glm_tile_loglike shares the data's row blocks between the four waves and needs the whole workgroup.  The step loop is this kernel's
// own: mh_body is bound to LikeSpec and stays as it is.
//
// EVERY WAVE OF A WORKGROUP TAKES THE SAME BRANCHES.  The four waves carry the same 16 walkers: they load the same z and logl, take
// the same draws (functions of seed, walker and step, or the same recorded words), and the inverse sums the log-det through LDS in
// the same order on every wave (SplineInverseTeam), so proposal, x', log-det, box verdict, `pre` and -- glm_tile_loglike ends with
// the same bits on the four waves -- logL' and `acc` are bit-identical across the waves.  Under a step rule the scale is too: the
// tile's count is a ballot of `acc`, the batch's total one number in device memory.  All 256 threads therefore meet at every barrier
// of the inverse and of the likelihood the same number of times.
//
// THE LIKELIHOOD IS SKIPPED in a step where nothing reads it: a proposal with pre == false is rejected whatever its logL.
// glm_tile_loglike contains a __syncthreads(), so the branch is taken by the workgroup, not by the walker: only when NO valid walker
// of the tile has pre (a ballot, the same on the four waves).  The value a walker without pre gets in a step that does evaluate is
// not read either, so the skip shows in no output.
// THE TWO ARRAYS OF PARTIALS alternate by the count of likelihood evaluations actually done, not by step: the proof that one barrier
// an evaluation is enough (nnest_spline_mcmc_glm.hip) needs strict alternation, and a skipped step does no evaluation.
//
// THE STEP RULE: per tile (NNEST_MH_DYNAMIC_STEP: the count is the tile's own ballot, no communication, any C) or over the batch
// (NNEST_MH_DYNAMIC_BATCH: mh_common.h's counters in mh_body's order -- read of step it - lag at the top, total before the post, at
// lag 0 both behind it; wave 0 posts, every wave reads).  The waits are the bounded ones; the launcher refuses a grid that is not
// proven resident.  Wave 0 stores.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mh.hip and nnest_spline_mcmc_glm.hip are: a step loop
// around the same inverse.
#include <stdio.h>
#include <string.h>

#include "glm_data.h"
#include "mh_glm.h"
#include "spline_latent.h"

namespace nnest {

// the doubles of the two arrays of partials, behind the tile's buffers (spl_tile_lds_floats is a multiple of 4 floats: 16 bytes)
constexpr int GLM_PART_FLOATS = 2 * 4 * 16 * 2;

// The step loop of one tile (16 walkers, this wave's copy).  tpar: [4][32 NT] in LDS -- std, mean, -inf, +inf; parts: [2][4][16]
// doubles in LDS.  `writer`: the wave that stores and posts.
template <int NT, int FAM, class Inv>
__device__ __forceinline__ void mh_glm_tile_steps(const MhGlmArgs &a, int D, int tile, int ntiles, int lane, int wv, const Inv &inv,
                                                  const float *tpar, double *parts, bool writer) {
    const int g = lane >> 4;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const int S = a.steps, C = a.C;
    const bool ok = row < C;
    const bool store = writer && ok;
    const int nvalid = min((int)SPL_TILE_WALKERS, C - tile * SPL_TILE_WALKERS);   // walkers of this tile
    const GlmSpec gl = a.gl;
    const double loglstar = a.loglstar;
    const bool batch = (a.flags & NNEST_MH_DYNAMIC_BATCH) != 0;
    const bool dynamic = batch || (a.flags & NNEST_MH_DYNAMIC_STEP) != 0;
    const int lag = mh_flag_lag(a.flags);
    const uint64_t seed = a.seed, walker = a.walker_offset + (uint64_t)row;

    f32x4 z[2][NT], x[2][NT];
    load_tile<NT>(a.z, row, ok, D, lane, z);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < NT; ++t) x[c][t] = z[c][t];
    float ld = group_sum(inv(x));
    double logl = ok ? a.logl[row] : 0.0;
    if (a.x0) store_tile<NT>(a.x0, row, store, D, lane, x);
    if (a.hist_x) store_tile<NT>(a.hist_x, (long)row * (S + 1), store, D, lane, x);
    if (a.hist_logl && store && lane < 16) a.hist_logl[(size_t)row * (S + 1)] = logl;

    double scale = (double)a.step_size;   // python float in the reference (sampler.py:255, :428-431)
    MhGlmVotes votes;
    int n_acc = 0, n_call = 0;
    int n_like = 0;   // likelihood evaluations done by the workgroup so far (uniform): which array of partials is next
#pragma unroll 1
    for (int it = 1; it <= S; ++it) {
        // the batch rule: the counts of step it - lag are requested now and consumed behind the decision
        unsigned long long early = 0;
        const bool have_total = batch && it - lag >= 1;
        if (have_total && lag > 0) early = mh_sync_read(a.sync, it - lag);
        const float fs = (float)scale;
        f32x4 e[2][NT], zp[2][NT], xp[2][NT];
        float u;
        if (a.noise_dz) {
            load_tile<NT>(a.noise_dz, (long)(it - 1) * C + row, ok, D, lane, e);
            u = ok ? a.noise_u[(size_t)(it - 1) * C + row] : 1.f;
        } else {
#pragma unroll
            for (int tau = 0; tau < NT; ++tau) {
                f32x4 n[2];
                bool live[2][4];
                tile_lane_normals(tau, g, D, [&](uint32_t b) { return noise_normal4(seed, walker, (uint32_t)it, b, NOISE_STREAM_DZ); }, n, live);
#pragma unroll
                for (int c = 0; c < 2; ++c)   // (padded dims get 0)
                    e[c][tau] = (f32x4){live[c][0] ? n[c].x : 0.f, live[c][1] ? n[c].y : 0.f, live[c][2] ? n[c].z : 0.f, live[c][3] ? n[c].w : 0.f};
            }
            u = noise_uniform(seed, walker, (uint32_t)it);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {   // z' = z + eps * fs: a product and a sum, as torch rounds them (no contraction)
                zp[c][t].x = __fadd_rn(z[c][t].x, __fmul_rn(e[c][t].x, fs)); zp[c][t].y = __fadd_rn(z[c][t].y, __fmul_rn(e[c][t].y, fs));
                zp[c][t].z = __fadd_rn(z[c][t].z, __fmul_rn(e[c][t].z, fs)); zp[c][t].w = __fadd_rn(z[c][t].w, __fmul_rn(e[c][t].w, fs));
                xp[c][t] = zp[c][t];
            }
        const float ldp = group_sum(inv(xp));
        const int inb = inbox_tile<NT>(xp, lane);   // UniformPrior(D, -1, 1) on x: priors.py:39-43
        const float log_ratio = inb ? (ldp - ld) : -INFINITY;
        float ratio = fminf(__expf(log_ratio), 1.0f);
        if (log_ratio != log_ratio) ratio = log_ratio;   // NaN stays NaN (u < NaN is false, as in torch)
        const bool pre = ok && (u < ratio);
        double lp = -1e100;   // (a skipped likelihood: never read, pre is false wherever it stands)
        if (__ballot(pre) != 0ull) {   // (the same on the four waves: the whole workgroup evaluates, or none of it)
            f32x4 tx[2][NT];
            spl_tile_map<NT>(tpar, lane, xp, tx);
            lp = glm_tile_loglike<NT, FAM>(gl, lane, wv, tx, parts + 64 * (n_like & 1));
            n_like += 1;
        }
        const bool acc = pre && (lp > loglstar);
        n_call += pre ? 1 : 0;
        n_acc += acc ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                z[c][t].x = acc ? zp[c][t].x : z[c][t].x; z[c][t].y = acc ? zp[c][t].y : z[c][t].y;
                z[c][t].z = acc ? zp[c][t].z : z[c][t].z; z[c][t].w = acc ? zp[c][t].w : z[c][t].w;
                x[c][t].x = acc ? xp[c][t].x : x[c][t].x; x[c][t].y = acc ? xp[c][t].y : x[c][t].y;
                x[c][t].z = acc ? xp[c][t].z : x[c][t].z; x[c][t].w = acc ? xp[c][t].w : x[c][t].w;
            }
        ld = acc ? ldp : ld;
        logl = acc ? lp : logl;
        if (dynamic) {   // sampler.py:422-431 per tile, or over the whole batch with the counts of step it - lag
            const int tile_accepted = __popcll(__ballot(acc && g == 0));
            int num_accepted = tile_accepted, num_total = nvalid;
            bool apply = true;
            if (batch) {
                apply = have_total;
                if (apply && lag > 0) num_accepted = mh_sync_total(a.sync, it - lag, ntiles, early, a.sync_err);
                if (writer && lane == 0) mh_sync_post(a.sync, it, tile, tile_accepted);
                if (apply && lag == 0) num_accepted = mh_sync_total(a.sync, it, ntiles, mh_sync_read(a.sync, it), a.sync_err);
                num_total = C;
            }
            if (apply) votes.vote(scale, num_accepted, num_total);
        }
        if (a.hist_x) store_tile<NT>(a.hist_x, (long)row * (S + 1) + it, store, D, lane, x);
        if (a.hist_logl && store && lane < 16) a.hist_logl[(size_t)row * (S + 1) + it] = logl;
    }
    if (a.scale_out && writer && lane == 0) a.scale_out[tile] = (float)scale;
    if (!store) return;
    store_tile<NT>(a.z, row, true, D, lane, z);
    if (a.x) store_tile<NT>(a.x, row, true, D, lane, x);
    if (lane < 16) {
        a.logl[row] = logl;
        if (a.n_call) a.n_call[row] = n_call;
        if (a.n_accept) a.n_accept[row] = n_acc | ((!a.x0 && n_acc > 0) ? NNEST_MH_ALL_MOVED : 0);   // (no side buffer: the accept count stands in)
    }
}

template <int NT, int NH, int FAM>
__global__ void __launch_bounds__(256) spline_mh_glm_kernel_team(MhGlmArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double *parts = reinterpret_cast<double *>(lds_buf + spl_tile_lds_floats(q.sp.D, NT));
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, nullptr, nullptr, lane, wv);
    mh_glm_tile_steps<NT, FAM>(a, q.sp.D, blockIdx.x, gridDim.x, lane, wv, t.inv, t.tpar, parts, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, int FAM>
static hipError_t spl_mh_glm_launch_t(const MhGlmArgs &a, const SplArgs &q, int num_cu, int *max_grid, hipStream_t st) {
    const size_t lds = (size_t)(spl_tile_lds_floats(q.sp.D, NT) + GLM_PART_FLOATS) * sizeof(float);
    const int grid = (a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_mh_glm_kernel_team<NT, NH, FAM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (max_grid || (a.flags & NNEST_MH_DYNAMIC_BATCH)) {   // the batch rule's waits span the grid: every workgroup must be resident
        int per_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(spline_mh_glm_kernel_team<NT, NH, FAM>), 256, lds);
        if (e != hipSuccess) return e;
        const int cap = (per_cu > 0 ? per_cu : 0) * num_cu;
        if (max_grid) { *max_grid = cap; return hipSuccess; }
        if (grid > cap) return hipErrorLaunchOutOfResources;
    }
    if (a.C <= 0) return hipSuccess;
    hipLaunchKernelGGL((spline_mh_glm_kernel_team<NT, NH, FAM>), dim3(grid), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

hipError_t launch_spline_mh_glm(const SplArgs &q, const MhGlmArgs &args, int num_cu, int *max_grid, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        constexpr int NT = decltype(sh)::NT, NH = decltype(sh)::NH;
        const int C = args.C;
        MhGlmArgs a = args;
        const bool runs = !max_grid && C > 0;
        if (runs && a.x && a.n_accept && !(a.x0 = mh_first_x_buffer((size_t)C * q.sp.D, st))) return hipErrorOutOfMemory;
        hipError_t e = hipErrorInvalidConfiguration;
        switch (a.gl.family) {
            case GLM_LOGISTIC: e = spl_mh_glm_launch_t<NT, NH, GLM_LOGISTIC>(a, q, num_cu, max_grid, st); break;
            case GLM_POISSON: e = spl_mh_glm_launch_t<NT, NH, GLM_POISSON>(a, q, num_cu, max_grid, st); break;
        }
        if (e != hipSuccess || !runs) return e;
        // every coordinate of the chain's last x differs from its first (nested.py:432): the follow-up kernel of the tile forms
        MhArgs m{};
        m.x0 = a.x0; m.x = a.x; m.n_accept = a.n_accept; m.C = C; m.s.D = q.sp.D;
        return launch_mh_all_moved(m, st);
    });
}

}  // namespace nnest
