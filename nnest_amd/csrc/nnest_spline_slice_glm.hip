// nnest_spline_slice_glm.hip -- the SLICE proposal in latent space of the neural-spline flow on a GENERALISED LINEAR MODEL of the
// user's data (logistic or Poisson regression): nnest_spline_slice_steps's update (nnest_spline_slice.hip; the definition is
// nnest_slice_steps's, the bracket rule slice_walk.h's) with
//   logL(x) := GLM(T(x)),  T(x)_d = ens_T(x_d, t_std[d], t_mean[d])  (spl_tile_map; NULL t_std / t_mean: the identity)
// and the likelihood of glm_data.h compiled in, in a kernel of its own (include/nnest_hip.h nnest_spline_slice_glm_steps; DESIGN.md
// 3.22).  BUILD-DEFINED.  The definition is nnest_slice_glm_steps's (nnest_slice_glm.hip): only the flow differs, and with it the
// layout.  The box is on x (inbox_tile), NOT on T(x): the map gets no lo / hi.
//
// Layout: the TEAM tile of spline_latent.h, 16 walkers per workgroup, four waves carrying the same 16 walkers -- the only form:
// glm_tile_loglike shares the data's row blocks between the four waves and needs the whole workgroup.  No step-size rule, so no
// workgroup waits for another: any C is a legal grid.  The loop runs in ROUNDS on the state machine of slice_walk.h, as
// nnest_spline_slice.hip's slice_body does (the rule is shared, the loop is this kernel's own): each walker with work left
// evaluates its own next candidate, a walker that has finished evaluates its frozen point and the result is dropped.
//
// EVERY WAVE OF A WORKGROUP TAKES THE SAME BRANCHES.  The four waves carry the same 16 walkers: they load the same z and logl,
// draw the same uniforms and directions (functions of seed, walker and update), and the inverse sums the log-det through LDS in the
// same order on every wave (SplineInverseTeam), so candidate, x, log-det, box verdict and -- glm_tile_loglike ends with the same
// bits on the four waves -- logL are bit-identical across the waves.  Hence the walkers' state (`active`, SliceWalk, `pre`) is, and so
// are the two ballots that steer the workgroup: "any walker with work left" (the round loop's condition) and "any active walker
// with pre" (below).  All 256 threads therefore meet at every barrier of the inverse and of the likelihood the same number of times.
//
// THE LIKELIHOOD IS SKIPPED in a round where no decision depends on it: a candidate with pre == false (outside the box, or below
// the slice level) cannot lie in the slice and its logL is never read; an idle walker's is dropped anyway.  glm_tile_loglike contains a
// __syncthreads(), so the branch is taken by the workgroup, not by the walker: only when NO active walker of the tile has pre.
// The value a walker without pre gets in a round that does evaluate is not read either, so the skip shows in no output.
// THE TWO ARRAYS OF PARTIALS alternate by the count of likelihood evaluations actually done, not by round: the proof that one
// barrier an evaluation is enough (nnest_spline_mcmc_glm.hip) needs strict alternation -- a wave that writes array k & 1 in
// evaluation k has passed the barrier of evaluation k - 1, which every wave reaches only after it has read the partials of
// evaluation k - 2 --, and a skipped round does no evaluation.
// Wave 0 stores.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_slice.hip and nnest_spline_mcmc_glm.hip are: a round loop
// around the same inverse.
#include <stdio.h>
#include <string.h>

#include "glm_data.h"
#include "slice_glm.h"
#include "spline_latent.h"

namespace nnest {

// the doubles of the two arrays of partials, behind the tile's buffers (spl_tile_lds_floats is a multiple of 4 floats: 16 bytes)
constexpr int GLM_PART_FLOATS = 2 * 4 * 16 * 2;

// The round loop of one tile (16 walkers, this wave's copy).  tpar: [4][32 NT] in LDS -- std, mean, -inf, +inf; parts: [2][4][16]
// doubles in LDS.  `writer`: the wave that stores.
template <int NT, int FAM, class Inv>
__device__ __forceinline__ void slice_glm_tile_rounds(const SliceGlmArgs &a, int D, int tile, int lane, int wv, const Inv &inv, const float *tpar,
                                                      double *parts, bool writer) {
    const int g = lane >> 4;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const bool ok = row < a.C;
    const bool store = writer && ok;
    const int S = a.steps, max_out = a.max_out, max_shrink = a.max_shrink, C = a.C;
    const GlmSpec gl = a.gl;
    const double loglstar = a.loglstar;
    const float width = a.width;
    const uint64_t seed = a.seed, walker = a.walker_offset + (uint64_t)row;

    f32x4 z[2][NT], x[2][NT], e[2][NT];
    load_tile<NT>(a.z, row, ok, D, lane, z);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < NT; ++t) { x[c][t] = z[c][t]; e[c][t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    float ld = group_sum(inv(x));
    double logl = ok ? a.logl[row] : 0.0;
    if (a.x0) store_tile<NT>(a.x0, row, store, D, lane, x);
    if (a.hist_x) store_tile<NT>(a.hist_x, (long)row * (S + 1), store, D, lane, x);

    SliceWalk sw = {};               // the bracket rule's state (slice_walk.h); sw.tc: the candidate of the next round
    float logy = 0.f;                // slice level
    int n_call = 0, n_move = 0, n_eval = 0;
    int n_like = 0;                  // likelihood evaluations done by the workgroup so far (uniform): which array of partials is next
    bool active = ok && S > 0;
    auto draw = [&](int k) { return noise_uniform(seed, walker, 64u * (uint32_t)sw.it + (uint32_t)k); };
    auto begin_update = [&]() {   // (divergent: no cross-lane work)
        sw.begin(draw, max_out);
        if (a.noise_dz) {
            load_tile<NT>(a.noise_dz, (long)(sw.it - 1) * C + row, true, D, lane, e);
        } else {
#pragma unroll
            for (int tau = 0; tau < NT; ++tau) {
                f32x4 n[2];
                bool live[2][4];
                tile_lane_normals(tau, g, D, [&](uint32_t b) { return noise_normal4(seed, walker, (uint32_t)sw.it, b, NOISE_STREAM_DZ); }, n, live);
#pragma unroll
                for (int c = 0; c < 2; ++c)   // (padded dims get 0)
                    e[c][tau] = (f32x4){live[c][0] ? n[c].x : 0.f, live[c][1] ? n[c].y : 0.f, live[c][2] ? n[c].z : 0.f, live[c][3] ? n[c].w : 0.f};
            }
        }
        logy = ld + __logf(draw(1));   // (u1 = 0: -inf, the whole feasible line is the slice)
    };
    if (active) begin_update();

    while (__ballot(active) != 0ull) {   // (the same on the four waves: see the top)
        // one evaluation per walker: candidate z + tc * width * eps (an idle walker: tc = 0, its own point)
        const float tw = sw.tc * width;
        f32x4 xc[2][NT];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                xc[c][t].x = __builtin_fmaf(e[c][t].x, tw, z[c][t].x); xc[c][t].y = __builtin_fmaf(e[c][t].y, tw, z[c][t].y);
                xc[c][t].z = __builtin_fmaf(e[c][t].z, tw, z[c][t].z); xc[c][t].w = __builtin_fmaf(e[c][t].w, tw, z[c][t].w);
            }
        const float ldc = group_sum(inv(xc));
        const int inb = inbox_tile<NT>(xc, lane);   // UniformPrior(D, -1, 1) on x: priors.py:39-43
        const bool pre = inb && (ldc > logy);
        double lc = -1e100;   // (a skipped likelihood: never read, pre is false wherever it stands)
        if (__ballot(active && pre) != 0ull) {   // (the same on the four waves: the whole workgroup evaluates, or none of it)
            f32x4 tx[2][NT];
            spl_tile_map<NT>(tpar, lane, xc, tx);
            lc = glm_tile_loglike<NT, FAM>(gl, lane, wv, tx, parts + 64 * (n_like & 1));
            n_like += 1;
        }
        const bool ins = pre && (lc > loglstar);
        const bool mv = active && sw.phase == 2 && ins;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {   // the move: the candidate's z is recomputed (the same fma), its x is the evaluation's
                z[c][t].x = mv ? __builtin_fmaf(e[c][t].x, tw, z[c][t].x) : z[c][t].x;
                z[c][t].y = mv ? __builtin_fmaf(e[c][t].y, tw, z[c][t].y) : z[c][t].y;
                z[c][t].z = mv ? __builtin_fmaf(e[c][t].z, tw, z[c][t].z) : z[c][t].z;
                z[c][t].w = mv ? __builtin_fmaf(e[c][t].w, tw, z[c][t].w) : z[c][t].w;
                x[c][t].x = mv ? xc[c][t].x : x[c][t].x; x[c][t].y = mv ? xc[c][t].y : x[c][t].y;
                x[c][t].z = mv ? xc[c][t].z : x[c][t].z; x[c][t].w = mv ? xc[c][t].w : x[c][t].w;
            }
        ld = mv ? ldc : ld;
        logl = mv ? lc : logl;
        if (active) {
            n_eval += 1;
            n_call += pre ? 1 : 0;
            if (sw.advance(ins, draw, max_out, max_shrink)) {
                n_move += ins ? 1 : 0;
                if (a.hist_x) store_tile<NT>(a.hist_x, (long)row * (S + 1) + sw.it, store, D, lane, x);
                if (sw.it < S) begin_update();
                else { active = false; sw.tc = 0.f; }
            }
        }
    }
    if (!store) return;
    store_tile<NT>(a.z, row, true, D, lane, z);
    if (a.x) store_tile<NT>(a.x, row, true, D, lane, x);
    if (lane < 16) {
        a.logl[row] = logl;
        if (a.n_call) a.n_call[row] = n_call;
        if (a.n_move) a.n_move[row] = n_move | ((!a.x0 && n_move > 0) ? NNEST_MH_ALL_MOVED : 0);   // (no x: the move count stands in)
        if (a.n_eval) a.n_eval[row] = n_eval;
    }
}

template <int NT, int NH, int FAM>
__global__ void __launch_bounds__(256) spline_slice_glm_kernel_team(SliceGlmArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double *parts = reinterpret_cast<double *>(lds_buf + spl_tile_lds_floats(q.sp.D, NT));
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, nullptr, nullptr, lane, wv);
    slice_glm_tile_rounds<NT, FAM>(a, q.sp.D, blockIdx.x, lane, wv, t.inv, t.tpar, parts, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH, int FAM>
static hipError_t spl_slice_glm_launch_t(const SliceGlmArgs &a, const SplArgs &q, hipStream_t st) {
    const size_t lds = (size_t)(spl_tile_lds_floats(q.sp.D, NT) + GLM_PART_FLOATS) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_slice_glm_kernel_team<NT, NH, FAM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((spline_slice_glm_kernel_team<NT, NH, FAM>), dim3((a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// (a shape's verdict comes before C: nnest_spline_slice_glm_check asks with C = 0)
hipError_t launch_spline_slice_glm(const SplArgs &q, const SliceGlmArgs &args, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        constexpr int NT = decltype(sh)::NT, NH = decltype(sh)::NH;
        const int C = args.C;
        if (C <= 0) return hipSuccess;
        SliceGlmArgs a = args;
        if (a.x && a.n_move && !(a.x0 = mh_first_x_buffer((size_t)C * q.sp.D, st))) return hipErrorOutOfMemory;
        hipError_t e = hipErrorInvalidConfiguration;
        switch (a.gl.family) {
            case GLM_LOGISTIC: e = spl_slice_glm_launch_t<NT, NH, GLM_LOGISTIC>(a, q, st); break;
            case GLM_POISSON: e = spl_slice_glm_launch_t<NT, NH, GLM_POISSON>(a, q, st); break;
        }
        if (e != hipSuccess) return e;
        // every coordinate of the chain's last x differs from its first (nested.py:432): the follow-up kernel of the tile forms
        MhArgs m{};
        m.x0 = a.x0; m.x = a.x; m.n_accept = a.n_move; m.C = C; m.s.D = q.sp.D;
        return launch_mh_all_moved(m, st);
    });
}

}  // namespace nnest
