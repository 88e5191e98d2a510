// nnest_spline_slice.hip -- the SLICE proposal in latent space with the neural-spline flow (include/nnest_hip.h
// nnest_spline_slice_steps: the definition and the noise streams; slice_walk.h: the bracket rule of one update).  BUILD-DEFINED, parity
// unpinned.  Only the flow differs from nnest_slice_steps: the spline's inverse (spline_inverse.h) replaces the coupling stack.
//
// Layout: the tiles of the spline proposal kernels -- 16 walkers per wave (WAVE), four waves per 16 walkers (TEAM), or four waves
// per 8 walkers held twice (PAIR) -- with the state in the parity-class tiles of flow_tile.h.  Slice walkers do not stay in step:
// the evaluations an update takes vary from walker to walker.  So the loop runs in ROUNDS: each walker keeps its own state (update
// index, phase -- left step-out, right step-out, shrinkage --, bracket, candidate, slice level), and in every round each walker with
// work left evaluates its own next candidate.  A walker that has finished its `steps` updates evaluates its frozen point (t = 0) and
// the result is discarded; the tile ends when a ballot finds no walker with work left.  Walkers never wait for each other at an
// update's end: a tile costs max over its walkers of the walker's evaluation count, not the sum over updates of the slowest walker.
// In the TEAM and PAIR forms every wave carries the same walkers and takes the same decisions (the log-det is summed in the same
// order on every wave), so the ballots agree across the workgroup and every wave runs the same number of rounds (the inverse has
// workgroup barriers).
#include <stdlib.h>
#include <string.h>

#include "flow_tile.h"
#include "mh_common.h"
#include "nnest_internal.h"
#include "spline_train_tile.h"

namespace nnest {

#include "spline_inverse.h"

// this lane's part of the direction of (walker, update it): dims 32 tau + 8 g + j are the quads 8 tau + 2 g and 8 tau + 2 g + 1 of
// noise_normal4 (what nnest_slice_fill_noise exports); padded dims get 0
template <int NT>
__device__ __forceinline__ void slice_direction(uint64_t seed, uint64_t walker, uint32_t it, int D, int lane, f32x4 (&e)[2][NT]) {
    const int g = lane >> 4;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        const int d0 = 32 * tau + 8 * g;
        f32x4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = {0.f, 0.f, 0.f, 0.f};
        if (d0 < D) {
            n0 = noise_normal4(seed, walker, it, (uint32_t)(8 * tau + 2 * g), NOISE_STREAM_DZ);
            n1 = noise_normal4(seed, walker, it, (uint32_t)(8 * tau + 2 * g + 1), NOISE_STREAM_DZ);
        }
        const float v[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = d0 + j < D ? v[j] : 0.f;
        e[0][tau] = (f32x4){m[0], m[2], m[4], m[6]};
        e[1][tau] = (f32x4){m[1], m[3], m[5], m[7]};
    }
}

// The round loop.  GW = walkers per tile: 16, or 8 held twice (lanes w and w ^ 8 carry walker w & 7, as in mh_body); counts and
// stores take the low copy.  `writer`: the wave that stores (every wave of a TEAM / PAIR workgroup computes the same state).
template <int NT, class Inv, int GW = 16>
__device__ __forceinline__ void slice_body(const SliceArgs &a, int D, int tile, int lane, const Inv &inv, bool writer) {
    static_assert(GW == 16 || GW == 8, "walkers per tile");
    const int w = lane & 15;
    const int row = tile * GW + (w & (GW - 1));
    const bool first_copy = GW == 16 || w < 8;
    const bool ok = row < a.C;
    const bool store = writer && ok && first_copy;
    const int S = a.steps, max_out = a.max_out, max_shrink = a.max_shrink, C = a.C;
    const LikeSpec like = a.like;
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
    bool active = ok && S > 0;
    auto draw = [&](int k) { return noise_uniform(seed, walker, 64u * (uint32_t)sw.it + (uint32_t)k); };
    auto begin_update = [&]() {   // (divergent: no cross-lane work)
        sw.begin(draw, max_out);
        if (a.noise_dz) load_tile<NT>(a.noise_dz, (long)(sw.it - 1) * C + row, true, D, lane, e);
        else slice_direction<NT>(seed, walker, (uint32_t)sw.it, D, lane, e);
        logy = ld + __logf(draw(1));   // (u1 = 0: -inf, the whole feasible line is the slice)
    };
    if (active) begin_update();

    while (__ballot(active) != 0ull) {
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
        const int inb = inbox_tile<NT>(xc, lane);   // UniformPrior(D, -1, 1): priors.py:39-43
        const bool pre = inb && (ldc > logy);
        const double lc = loglike_tile<NT>(like, D, lane, xc);
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

// WAVE: one wave per 16 walkers, the waves of a workgroup independent
template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_slice_kernel_wave(SliceArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int tile = blockIdx.x * wpb + wave;
    if (tile >= ((a.C + 15) >> 4)) return;
    SplineInverse<NT, NH> inv = {q.img, q.sp, lds_buf + (size_t)wave * 16 * (q.sp.D + 1), lane};
    slice_body<NT>(a, q.sp.D, tile, lane, inv, true);
}

// TEAM: four waves per 16 walkers, the spline evaluations of the inverse divided between them (spline_mh_kernel_team's layout)
template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_slice_kernel_team(SliceArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *bufs = lds_buf;                                                                     // 4 x 16 x (D+1)
    f32x4 *xch = reinterpret_cast<f32x4 *>(lds_buf + ((4 * 16 * (q.sp.D + 1) + 3) & ~3));     // 4 x NT x 64 f32x4
    float *ldred = reinterpret_cast<float *>(xch + 4 * NT * 64);                               // 4 x 16
    SplineInverseTeam<NT, NH, 4> inv = {q.img, q.sp, bufs + (size_t)wv * 16 * (q.sp.D + 1), xch, ldred, lane, wv};
    slice_body<NT>(a, q.sp.D, blockIdx.x, lane, inv, wv == 0);
}

// PAIR: four waves per 8 walkers held in both halves of the matrix-core columns (spline_mh_kernel_pair's layout); x_dim > 32
template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_slice_kernel_pair(SliceArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *bufs = lds_buf;                                                                     // 4 x 16 x (D+1)
    f32x4 *xch = reinterpret_cast<f32x4 *>(lds_buf + ((4 * 16 * (q.sp.D + 1) + 3) & ~3));     // 2 x 4 x NT x 64 f32x4
    float *ldred = reinterpret_cast<float *>(xch + 2 * 4 * NT * 64);                           // 2 x 4 x 16
    float *trunks = ldred + 2 * 4 * 16;                                                        // B x 2 x spl_cond_hidden_floats
    spline_stage_trunks<NT, NH>(q.img, q.sp, trunks, threadIdx.x, 256);
    __syncthreads();
    SplineInverseHalves<NT, NH> inv = {q.img, q.sp, bufs + (size_t)wv * 16 * (q.sp.D + 1), xch, ldred, trunks, lane, wv};
    slice_body<NT, SplineInverseHalves<NT, NH>, 8>(a, q.sp.D, blockIdx.x, lane, inv, wv == 0);
}

// Which form runs for C walkers (nnest_spline_slice_form_for): flags bits 0..3 pin one (NNEST_SPLINE_SLICE_FORM), else the rule of
// the spline proposal kernel without its batch-rule branch (spline_mh_form): PAIR at x_dim > 32 while its 8-walker tiles fit one per
// CU, TEAM while the 16-walker tiles fit two per CU, WAVE beyond.  -1: the pinned form does not exist for this shape (PAIR needs two
// or more 16-slot tiles per half: x_dim > 32).
int spline_slice_form(const SplineShape &sp, int C, int flags, int num_cu) {
    const int pin = (flags & 15) - 1;
    if (pin == NNEST_SPLINE_MH_WAVE || pin == NNEST_SPLINE_MH_TEAM) return pin;
    if (pin == NNEST_SPLINE_MH_PAIR) return sp.NTh >= 2 ? pin : -1;
    if (pin >= 0) return -1;
    if (sp.NTh >= 2 && (C + 7) / 8 <= num_cu) return NNEST_SPLINE_MH_PAIR;
    if ((C + 15) / 16 <= 2 * num_cu) return NNEST_SPLINE_MH_TEAM;
    return NNEST_SPLINE_MH_WAVE;
}

template <int NT, int NH>
static hipError_t launch_slice_t(const SliceArgs &a, const SplArgs &q, int form, int num_cu, hipStream_t st) {
    const int D = q.sp.D, ntiles = (a.C + 15) / 16;
    if (form == NNEST_SPLINE_MH_WAVE) {
        int wpb = 1;   // (pick_geometry's rule: the waves of a workgroup share a CU)
        if (ntiles > 2 * num_cu) wpb = 2;
        if (ntiles > 4 * num_cu) wpb = 4;
        const size_t lds = (size_t)wpb * 16 * (D + 1) * sizeof(float);
        hipLaunchKernelGGL((spline_slice_kernel_wave<NT, NH>), dim3((ntiles + wpb - 1) / wpb), dim3(64 * wpb), lds, st, a, q);
        return hipGetLastError();
    }
    if (form == NNEST_SPLINE_MH_TEAM) {
        const size_t lds = (size_t)(((4 * 16 * (D + 1) + 3) & ~3) + 4 * NT * 64 * 4 + 4 * 16) * sizeof(float);
        hipLaunchKernelGGL((spline_slice_kernel_team<NT, NH>), dim3(ntiles), dim3(256), lds, st, a, q);
        return hipGetLastError();
    }
    if constexpr (NT >= 2) {
        const size_t lds = (size_t)(((4 * 16 * (D + 1) + 3) & ~3) + 2 * 4 * NT * 64 * 4 + 2 * 4 * 16 + q.sp.B * 2 * spl_cond_hidden_floats(NT, NH)) * sizeof(float);
        if (lds > 64 * 1024) {   // (above 64 KB of dynamic LDS a kernel has to be told so once)
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spline_slice_kernel_pair<NT, NH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((spline_slice_kernel_pair<NT, NH>), dim3((a.C + 7) / 8), dim3(256), lds, st, a, q);
        return hipGetLastError();
    }
    return hipErrorInvalidConfiguration;
}

hipError_t launch_spline_slice(const SplArgs &q, const SliceArgs &args, int flags, int num_cu, hipStream_t st) {
    const SplineShape &sp = q.sp;
    const int C = args.C;
    if (C <= 0) return hipSuccess;
    const int form = spline_slice_form(sp, C, flags, num_cu);
    if (form < 0 || !spline_shape_supported(sp)) return hipErrorInvalidConfiguration;
    SliceArgs a = args;
    if (a.x && a.n_move && !(a.x0 = mh_first_x_buffer((size_t)C * sp.D, st))) return hipErrorOutOfMemory;
    hipError_t e;
    switch (sp.NTh * 10 + sp.NH) {
        case 11: e = launch_slice_t<1, 1>(a, q, form, num_cu, st); break;
        case 21: e = launch_slice_t<2, 1>(a, q, form, num_cu, st); break;
        case 31: e = launch_slice_t<3, 1>(a, q, form, num_cu, st); break;
        case 41: e = launch_slice_t<4, 1>(a, q, form, num_cu, st); break;
        case 12: e = launch_slice_t<1, 2>(a, q, form, num_cu, st); break;
        case 22: e = launch_slice_t<2, 2>(a, q, form, num_cu, st); break;
        default: return hipErrorInvalidConfiguration;
    }
    if (e != hipSuccess) return e;
    // every coordinate of the chain's last x differs from its first (nested.py:432): the follow-up kernel of the tile forms
    MhArgs m{};
    m.x0 = a.x0; m.x = a.x; m.n_accept = a.n_move; m.C = C; m.s.D = sp.D;
    return launch_mh_all_moved(m, st);
}

}  // namespace nnest
