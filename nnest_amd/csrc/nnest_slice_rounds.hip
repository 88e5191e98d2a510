// nnest_slice_rounds.hip -- the SLICE proposal in latent space as a state machine on the device that advances in ROUNDS, with the
// flow's inverse and the likelihood outside the kernels (include/nnest_hip.h nnest_slice_rounds_*: the definition and the noise
// streams, nnest_slice_steps's; slice_walk.h: the bracket rule of one update).  BUILD-DEFINED, parity unpinned.
//
// One round: the caller maps every walker's candidate z' through ANY flow's inverse (x', log|det|), rounds_screen_kernel tests the box
// and the slice level and packs the x' rows that need a likelihood in ascending walker order, the caller evaluates the likelihood on
// those rows only (a host callable, or a device likelihood kernel), and rounds_advance_kernel consumes the results, steps each
// walker's state machine and writes its next candidate.  Walkers do not wait for each other: a walker that finishes an update starts
// its next one in the next round, so a batch takes as many rounds as its busiest walker has evaluations.  Finished walkers propose
// nothing (their candidate row keeps its last, finite value: the flow still maps it, the screen skips it).
//
// Layout: begin / advance / finish run one wave per walker, each lane owning the dims 4q..4q+3 of quads q = lane, lane + 64, ...
// (the quads of noise_normal4: a lane reads back only what it wrote); the walker's scalar state is wave-uniform.  The screen is ONE
// workgroup: a wave64 ballot + mbcnt prefix per wave and an LDS prefix over the waves give every walker that needs a likelihood its
// packed row -- deterministic, no atomics, so repeated and sharded launches reproduce bit for bit.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flow_tile.h"
#include "mh_common.h"
#include "nnest_internal.h"

namespace nnest {

struct SliceWalker {   // one walker's state machine
    double logl;       // logL of the current point
    float ld, ldc;     // log|det dx/dz| of the current point, of this round's candidate
    float logy;        // slice level
    SliceWalk walk;    // update, phase and bracket (slice_walk.h); walk.tc: this round's candidate t
    int active;        // updates left (this round's candidate is live)
    int pre, slot;     // this round's screen: box and level passed; packed row (-1: none)
    int n_call, n_move, n_eval;
};

struct RoundArgs {
    SliceWalker *w;
    float *z, *x, *x0, *e;    // [C][D]: current point, its x, the first x, the update's direction
    int *base;                // [2]: global index of this round's first packed row, of the next round's
    int C, D, steps, max_out, max_shrink;
    float width;
    double loglstar;
    uint64_t seed, walker_offset;
    const float *noise_dz;    // recorded directions [steps][C][D] or NULL
    float *hist_x, *hist_z;   // [C][steps + 1][D] or NULL
    double *hist_logl;        // [C][steps + 1] or NULL
    int *move_ref;            // [C][steps]: global packed row the update moved to, -1: stayed (or NULL)
};

// the dims of this lane: quads q = lane + 64 j, dims 4 q + r < D
#define FOR_LANE_DIMS(D, lane, d)                                                   \
    for (int q__ = (lane); 4 * q__ < (D); q__ += 64)                               \
        for (int r__ = 0, d = 4 * q__; r__ < 4; ++r__, d = 4 * q__ + r__)          \
            if (d < (D))

// uniform k of the walker's current update
struct RoundDraw {
    uint64_t seed, walker;
    const SliceWalk &walk;
    __device__ __forceinline__ float operator()(int k) const { return noise_uniform(seed, walker, 64u * (uint32_t)walk.it + (uint32_t)k); }
};

// the next update: bracket and first candidate (slice_walk.h), direction, level
__device__ __forceinline__ void begin_update(const RoundArgs &a, SliceWalker &s, int c, int lane) {
    const uint64_t walker = a.walker_offset + (uint64_t)c;
    const RoundDraw draw = {a.seed, walker, s.walk};
    s.walk.begin(draw, a.max_out);
    const int D = a.D, it = s.walk.it;
    float *e = a.e + (size_t)c * D;
    if (a.noise_dz) {
        const float *src = a.noise_dz + ((size_t)(it - 1) * a.C + c) * D;
        FOR_LANE_DIMS(D, lane, d) e[d] = src[d];
    } else {
        for (int q = lane; 4 * q < D; q += 64) {
            const f32x4 n = noise_normal4(a.seed, walker, (uint32_t)it, (uint32_t)q, NOISE_STREAM_DZ);
            const float v[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * q + r < D) e[4 * q + r] = v[r];
        }
    }
    s.logy = s.ld + __logf(draw(1));   // (u1 = 0: -inf, the whole feasible line is the slice)
}

// z' = z + t * width * eps, one fused multiply-add per dim (slice_kernel_solo's candidate)
__device__ __forceinline__ void propose(const RoundArgs &a, const SliceWalker &s, int c, int lane, float *z_cand) {
    const int D = a.D;
    const float tw = s.walk.tc * a.width;
    const float *z = a.z + (size_t)c * D, *e = a.e + (size_t)c * D;
    float *o = z_cand + (size_t)c * D;
    FOR_LANE_DIMS(D, lane, d) o[d] = __builtin_fmaf(e[d], tw, z[d]);
}

__device__ __forceinline__ void store_history(const RoundArgs &a, const SliceWalker &s, int c, int lane, int it) {
    const int D = a.D;
    const size_t r = (size_t)c * (a.steps + 1) + it;
    if (a.hist_x) { const float *x = a.x + (size_t)c * D; FOR_LANE_DIMS(D, lane, d) a.hist_x[r * D + d] = x[d]; }
    if (a.hist_z) { const float *z = a.z + (size_t)c * D; FOR_LANE_DIMS(D, lane, d) a.hist_z[r * D + d] = z[d]; }
    if (a.hist_logl && lane == 0) a.hist_logl[r] = s.logl;
}

__global__ void __launch_bounds__(256) rounds_begin_kernel(RoundArgs a, const float *z_in, const float *x_in, const float *ld_in,
                                                           const double *logl_in, float *z_cand) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c == 0 && lane == 0) { a.base[0] = 0; a.base[1] = 0; }
    if (c >= a.C) return;
    const int D = a.D;
    SliceWalker s;
    memset(&s, 0, sizeof(s));
    s.logl = logl_in[c];
    s.ld = ld_in[c];
    s.slot = -1;
    s.active = a.steps > 0;
    const size_t o = (size_t)c * D;
    FOR_LANE_DIMS(D, lane, d) {
        a.z[o + d] = z_in[o + d];
        a.x[o + d] = x_in[o + d];
        a.x0[o + d] = x_in[o + d];
    }
    store_history(a, s, c, lane, 0);
    if (a.move_ref)
        for (int j = lane; j < a.steps; j += 64) a.move_ref[(size_t)c * a.steps + j] = -1;
    if (s.active) {
        begin_update(a, s, c, lane);
        propose(a, s, c, lane, z_cand);
    } else {
        FOR_LANE_DIMS(D, lane, d) z_cand[o + d] = z_in[o + d];   // (a finite row for the flow to map)
    }
    if (lane == 0) a.w[c] = s;
}

// ONE workgroup of SCREEN_THREADS: the box (or the caller's prior flags) and the slice level of every live candidate; the rows that
// need a likelihood are packed in ascending walker order.  counts = {packed rows, walkers with a live candidate}.
constexpr int SCREEN_THREADS = 1024;
__global__ void __launch_bounds__(SCREEN_THREADS) rounds_screen_kernel(RoundArgs a, const float *x_cand, const float *ld_cand,
                                                                       const int *inbox, float *rows, int *idx, int *counts) {
    constexpr int NW = SCREEN_THREADS / 64;
    __shared__ int wrows[NW], wact[NW], outside[SCREEN_THREADS], src[SCREEN_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, D = a.D;
    int n_rows = 0, n_active = 0;   // block-uniform
    for (int c0 = 0; c0 < a.C; c0 += SCREEN_THREADS) {
        const int c = c0 + tid;
        if (!inbox) {   // UniformPrior(D, -1, 1) (priors.py:39-43; inbox_tile): NaN counts as inside.  The chunk's rows are read
                        // contiguously by the whole workgroup (a row per thread: uncoalesced)
            outside[tid] = 0;
            __syncthreads();
            const int nw = a.C - c0 < SCREEN_THREADS ? a.C - c0 : SCREEN_THREADS;
            const float *xb = x_cand + (size_t)c0 * D;
#pragma unroll 8
            for (int i = tid; i < nw * D; i += SCREEN_THREADS) {   // (unrolled: eight loads in flight, not one)
                const float v = xb[i];
                if (v < -1.f || v > 1.f) outside[i / D] = 1;   // (a benign race: every writer stores 1)
            }
            __syncthreads();
        }
        bool act = false, need = false;
        if (c < a.C) {
            SliceWalker &s = a.w[c];
            act = s.active != 0;
            if (act) {
                const float ldc = ld_cand[c];
                const int inb = inbox ? inbox[c] != 0 : !outside[tid];
                need = inb && (ldc > s.logy);
                s.ldc = ldc;
                s.pre = need;
            }
        }
        const unsigned long long m = __ballot(need), am = __ballot(act);
        if (lane == 0) { wrows[wv] = __popcll(m); wact[wv] = __popcll(am); }
        __syncthreads();
        int wbase = n_rows, tot = 0, atot = 0;
        for (int j = 0; j < NW; ++j) {
            if (j < wv) wbase += wrows[j];
            tot += wrows[j];
            atot += wact[j];
        }
        __syncthreads();   // (wrows / wact are rewritten by the next chunk)
        const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (c < a.C) a.w[c].slot = need ? wbase + below : -1;
        if (need) {
            idx[wbase + below] = c;
            src[wbase + below - n_rows] = c;
        }
        __syncthreads();
        // the chunk's packed rows, copied by the whole workgroup element by element (a walker at a time per wave
        // made the copies a serial chain)
#pragma unroll 8
        for (int i = tid; i < tot * D; i += SCREEN_THREADS) {
            const int r = i / D, d = i - r * D;
            rows[(size_t)(n_rows + r) * D + d] = x_cand[(size_t)src[r] * D + d];
        }
        n_rows += tot;
        n_active += atot;
    }
    if (tid == 0) {
        counts[0] = n_rows;
        counts[1] = n_active;
        const int b = a.base[1];
        a.base[0] = b;
        a.base[1] = b + n_rows;
    }
}

// the decisions of the round (the screen's flag, logL of the packed rows), the state machine's step, the next candidate
__global__ void __launch_bounds__(256) rounds_advance_kernel(RoundArgs a, const float *rows, const double *logl_rows, float *z_cand) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.C) return;
    SliceWalker s = a.w[c];
    if (!s.active) return;
    const int D = a.D;
    const size_t o = (size_t)c * D;
    const bool pre = s.pre != 0;
    const double lc = pre ? logl_rows[s.slot] : 0.0;
    const bool ins = pre && (lc > a.loglstar);
    s.n_eval += 1;
    s.n_call += pre ? 1 : 0;
    const int it = s.walk.it;
    const bool done = s.walk.advance(ins, RoundDraw{a.seed, a.walker_offset + (uint64_t)c, s.walk}, a.max_out, a.max_shrink);
    if (done && ins) {   // the walker moves to the candidate (its z' and the packed x' row)
        const float *xr = rows + (size_t)s.slot * D;
        FOR_LANE_DIMS(D, lane, d) {
            a.z[o + d] = z_cand[o + d];
            a.x[o + d] = xr[d];
        }
        s.ld = s.ldc;
        s.logl = lc;
        s.n_move += 1;
        if (a.move_ref && lane == 0) a.move_ref[(size_t)c * a.steps + it - 1] = a.base[0] + s.slot;
    }
    if (done) {
        store_history(a, s, c, lane, it);
        if (it < a.steps) begin_update(a, s, c, lane);
        else s.active = 0;
    }
    if (s.active) propose(a, s, c, lane, z_cand);
    if (lane == 0) a.w[c] = s;
}

__global__ void __launch_bounds__(256) rounds_finish_kernel(RoundArgs a, float *z_out, float *x_out, double *logl_out, int *n_call,
                                                            int *n_move, int *n_eval) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.C) return;
    const SliceWalker s = a.w[c];
    const int D = a.D;
    const size_t o = (size_t)c * D;
    bool mine = true;   // every coordinate of the chain's last x differs from its first (NNEST_MH_ALL_MOVED; nested.py:432)
    FOR_LANE_DIMS(D, lane, d) {
        const float xv = a.x[o + d];
        mine = mine && xv != a.x0[o + d];
        if (z_out) z_out[o + d] = a.z[o + d];
        if (x_out) x_out[o + d] = xv;
    }
    const bool all_moved = __ballot(!mine) == 0ull;
    if (lane == 0) {
        if (logl_out) logl_out[c] = s.logl;
        if (n_call) n_call[c] = s.n_call;
        if (n_move) n_move[c] = s.n_move | (all_moved ? NNEST_MH_ALL_MOVED : 0);
        if (n_eval) n_eval[c] = s.n_eval;
    }
}

}  // namespace nnest

using namespace nnest;

struct nnest_slice_rounds {
    int C, D, steps;
    int begun;
    void *mem;        // one allocation: walkers, z, x, x0, e, base
    RoundArgs a;
};

static int rfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    set_last_error(buf);
    return code;
}

#define RHIP(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return rfail(NNEST_E_HIP, "%s: %s", #expr, hipGetErrorString(e__));        \
    } while (0)

static int walker_grid(int C) { return (C + 3) / 4; }

extern "C" {

int nnest_slice_rounds_create(int C, int D, int steps, nnest_slice_rounds_t **out) {
    if (!out) return rfail(NNEST_E_ARG, "out is NULL");
    *out = nullptr;
    if (C < 1 || D < 1 || steps < 0) return rfail(NNEST_E_ARG, "bad C=%d D=%d steps=%d", C, D, steps);
    const size_t walkers = ((size_t)C * sizeof(SliceWalker) + 255) & ~(size_t)255;
    const size_t rowsz = ((size_t)C * D * sizeof(float) + 255) & ~(size_t)255;
    void *mem = nullptr;
    RHIP(hipMalloc(&mem, walkers + 4 * rowsz + 256));
    nnest_slice_rounds *h = new nnest_slice_rounds();
    memset(h, 0, sizeof(*h));
    h->C = C; h->D = D; h->steps = steps; h->mem = mem;
    char *p = (char *)mem;
    h->a.w = (SliceWalker *)p;
    h->a.z = (float *)(p + walkers);
    h->a.x = (float *)(p + walkers + rowsz);
    h->a.x0 = (float *)(p + walkers + 2 * rowsz);
    h->a.e = (float *)(p + walkers + 3 * rowsz);
    h->a.base = (int *)(p + walkers + 4 * rowsz);
    h->a.C = C; h->a.D = D; h->a.steps = steps;
    *out = h;
    return NNEST_OK;
}

int nnest_slice_rounds_destroy(nnest_slice_rounds_t *h) {
    if (!h) return NNEST_OK;
    hipError_t e = hipFree(h->mem);
    delete h;
    if (e != hipSuccess) return rfail(NNEST_E_HIP, "hipFree: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_slice_rounds_begin(nnest_slice_rounds_t *h, const float *z_dev, const float *x_dev, const float *ld_dev, const double *logl_dev,
                             double loglstar, float width, int max_stepout, int max_shrink, const float *noise_dz_dev, uint64_t seed,
                             uint64_t walker_offset, float *hist_x_dev, float *hist_z_dev, double *hist_logl_dev, int *move_ref_dev,
                             float *z_cand_dev, void *stream) {
    if (!h) return rfail(NNEST_E_ARG, "NULL handle");
    if (!z_dev || !x_dev || !ld_dev || !logl_dev || !z_cand_dev) return rfail(NNEST_E_ARG, "NULL device buffer");
    if (!slice_params_ok(h->steps, max_stepout, max_shrink, width))
        return rfail(NNEST_E_ARG, "max_stepout=%d (0..2^24) max_shrink=%d (1..60) width=%g", max_stepout, max_shrink, (double)width);
    RoundArgs &a = h->a;
    a.loglstar = loglstar; a.width = width; a.max_out = max_stepout; a.max_shrink = max_shrink;
    a.noise_dz = noise_dz_dev; a.seed = seed; a.walker_offset = walker_offset;
    a.hist_x = hist_x_dev; a.hist_z = hist_z_dev; a.hist_logl = hist_logl_dev; a.move_ref = move_ref_dev;
    hipLaunchKernelGGL(rounds_begin_kernel, dim3(walker_grid(h->C)), dim3(256), 0, (hipStream_t)stream, a, z_dev, x_dev, ld_dev,
                       logl_dev, z_cand_dev);
    RHIP(hipGetLastError());
    h->begun = 1;
    return NNEST_OK;
}

int nnest_slice_rounds_screen(nnest_slice_rounds_t *h, const float *x_cand_dev, const float *ld_cand_dev, const int *inbox_dev,
                              float *rows_dev, int *idx_dev, int *counts_dev, void *stream) {
    if (!h) return rfail(NNEST_E_ARG, "NULL handle");
    if (!x_cand_dev || !ld_cand_dev || !rows_dev || !idx_dev || !counts_dev) return rfail(NNEST_E_ARG, "NULL device buffer");
    if (!h->begun) return rfail(NNEST_E_ARG, "nnest_slice_rounds_begin has not run on this handle");
    hipLaunchKernelGGL(rounds_screen_kernel, dim3(1), dim3(SCREEN_THREADS), 0, (hipStream_t)stream, h->a, x_cand_dev, ld_cand_dev,
                       inbox_dev, rows_dev, idx_dev, counts_dev);
    RHIP(hipGetLastError());
    return NNEST_OK;
}

int nnest_slice_rounds_advance(nnest_slice_rounds_t *h, const float *rows_dev, const double *logl_rows_dev, float *z_cand_dev, void *stream) {
    if (!h) return rfail(NNEST_E_ARG, "NULL handle");
    if (!rows_dev || !logl_rows_dev || !z_cand_dev) return rfail(NNEST_E_ARG, "NULL device buffer");
    if (!h->begun) return rfail(NNEST_E_ARG, "nnest_slice_rounds_begin has not run on this handle");
    hipLaunchKernelGGL(rounds_advance_kernel, dim3(walker_grid(h->C)), dim3(256), 0, (hipStream_t)stream, h->a, rows_dev, logl_rows_dev,
                       z_cand_dev);
    RHIP(hipGetLastError());
    return NNEST_OK;
}

int nnest_slice_rounds_finish(nnest_slice_rounds_t *h, float *z_dev, float *x_dev, double *logl_dev, int *n_call_dev, int *n_move_dev,
                              int *n_eval_dev, void *stream) {
    if (!h) return rfail(NNEST_E_ARG, "NULL handle");
    if (!h->begun) return rfail(NNEST_E_ARG, "nnest_slice_rounds_begin has not run on this handle");
    hipLaunchKernelGGL(rounds_finish_kernel, dim3(walker_grid(h->C)), dim3(256), 0, (hipStream_t)stream, h->a, z_dev, x_dev, logl_dev,
                       n_call_dev, n_move_dev, n_eval_dev);
    RHIP(hipGetLastError());
    return NNEST_OK;
}

}  // extern "C"
