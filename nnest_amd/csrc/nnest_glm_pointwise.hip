// nnest_glm_pointwise.hip -- POINTWISE PREDICTIVE STATISTICS of the regression likelihoods of user data over a set of posterior
// draws (include/nnest_hip.h nnest_glm_pointwise, nnest_glm_predict; glm_pointwise.h): per data row the max-shifted
// sums, the count and the moments of l_is over the draws s -- what lppd, WAIC and importance-sampled leave-one-out are made of --,
// and per new design row the moments of the inverse link.  The [S x n] matrix of terms is never stored.
//
// THE MIRROR OF glm_tile_loglike (glm_data.h): there the 16 walkers are the invariant operand and the rows of A stream; here A^T
// eta^T = A t^T is the same [n x D] [D x 16] product on the matrix cores (v_mfma_f32_16x16x4f32, mfma4) with A the invariant one.
//   * A wave owns ONE block of 16 data rows, rb = 4 blockIdx.x + wave.  Lane = 16 g + m holds A[16 rb + m, 32 tau + 8 g + j]
//     (tau < NT, j < 8: NT * 8 registers, read once from at, the 16 lanes m one run) for the whole launch.
//   * The draws stream in tiles of 16: lane (m, g) reads, of draw 16 tile + m, the 8 consecutive floats at column 32 tau + 8 g of
//     its row of t -- 32 B PER LANE STRAIGHT FROM GLOBAL MEMORY, no LDS and so no barrier: the four lanes g of a draw read one
//     128-byte run, and a tile of t is used by this wave alone, so staging it in LDS would add a round trip and share nothing.  The
//     loads carry no branch (a column past D - 1 reads column D - 1 and is zeroed behind the load, a draw past S - 1 reads draw
//     S - 1 and is not counted), and the NEXT tile's loads are issued before this tile's float64 terms, which are what the kernel
//     spends its time on (one exp and one log1p or exp for the term, two exp for the shifted sums, a division for the mean, per pair).
//     In the ISA (NT = 2) the loop is: s_waitcnt vmcnt(0), twelve MFMAs, the next tile's sixteen global_load_dword back to back, the
//     last four MFMAs, the four terms and their statistics (about a thousand instructions), and only then the wait for those loads.
//   * The accumulator starts from the offsets; lane (m, g) ends a tile with eta of rows 16 rb + 4 g + v (v < 4) of draw m: four
//     distinct (row, draw) pairs, no float64 term twice in a wave.  It keeps running statistics of its four rows.
//   * After its last tile the 16 lanes m that share the rows 4 g + v are merged by a butterfly (xor 1, 2, 4, 8) with the
//     symmetric merge: every lane ends with the same bits, lane m = 0 writes the rows i < n into the group's partials.
//   * The grid is ceil(n / 64) row groups x G draw groups (glm_pointwise_groups); draw group c takes the tiles c, c + G, ...  A
//     second kernel, one thread per row, merges the G partials in index order.  No atomics of any kind.
// Rows i >= n are masked (never written; what the padded arrays hold there reaches only those rows' own accumulators), no read
// goes past [D, ld] (16 (rb + 1) <= ld for every row block the grid starts, a wave past the last one returns), no barrier is used.
#include <type_traits>

#include "glm_pointwise.h"

namespace nnest {

#pragma clang fp contract(off)
// the inverse link, float64 from the float32 linear predictor (NaN where that is not finite)
template <int FAM>
__device__ __forceinline__ double glm_inverse_link(float eta) {
    if (!(fabsf(eta) <= 3.40282346638528860e38f)) return __builtin_nan("");
    const double e = (double)eta;
    if constexpr (FAM == GLM_LOGISTIC) return 1.0 / (1.0 + exp(-e));
    else return exp(e);
}
#pragma clang fp contract(fast)

__device__ __forceinline__ PwShift pw_xor(const PwShift &r, int k) { return PwShift{__shfl_xor(r.m, k), __shfl_xor(r.s1, k), __shfl_xor(r.s2, k)}; }
__device__ __forceinline__ PwMoments pw_xor(const PwMoments &r, int k) { return PwMoments{__shfl_xor(r.n, k), __shfl_xor(r.mean, k), __shfl_xor(r.m2, k)}; }
__device__ __forceinline__ PwStats pw_xor(const PwStats &r, int k) {
    return PwStats{pw_xor(r.p, k), pw_xor(r.q, k), __shfl_xor(r.n, k), __shfl_xor(r.mean, k), __shfl_xor(r.m2, k)};
}

template <int NT, int FAM, int PRED>
__global__ void __launch_bounds__(256) glm_pointwise_kernel(GlmSpec gl, const float *__restrict__ t, double *__restrict__ partials, int S, int G) {
    using T = typename std::conditional<PRED != 0, PwMoments, PwStats>::type;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int D = gl.D, n = gl.n;
    const int rb = 4 * blockIdx.x + wave, chunk = blockIdx.y;
    if (16 * rb >= n) return;   // (uniform in the wave; no barrier follows)
    const int i0 = 16 * rb + 4 * g;
    float a[NT][8];
    pw_load_a<NT>(gl, rb, m, g, a);
    const f32x4 off = *reinterpret_cast<const f32x4 *>(gl.o + i0);
    f32x4 yv = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (!PRED) yv = *reinterpret_cast<const f32x4 *>(gl.y + i0);
    T st[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) st[v] = PwSlots<T>::empty();

    const int ntiles = (S + GLMPW_TILE - 1) / GLMPW_TILE;
    float b[NT][8];
    if (chunk < ntiles) pw_load_tile<NT>(t, (long)GLMPW_TILE * chunk + m, S, D, g, b);
    for (int tl = chunk; tl < ntiles; tl += G) {   // (uniform)
        const long s = (long)GLMPW_TILE * tl + m;
        float bn[NT][8];
        // the next tile's loads in front of this tile's terms (past the last tile: this group's last tile again, dropped)
        pw_load_tile<NT>(t, (long)GLMPW_TILE * (tl + G < ntiles ? tl + G : tl) + m, S, D, g, bn);
        f32x4 acc = off;
#pragma unroll
        for (int tau = 0; tau < NT; ++tau)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = mfma4(a[tau][j], b[tau][j], acc);
        const bool in = s < S;
        const float eta[4] = {acc.x, acc.y, acc.z, acc.w};
        const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            double val;
            if constexpr (PRED) val = glm_inverse_link<FAM>(eta[v]);
            else val = glm_term<FAM>(eta[v], yy[v]);
            pw_add(st[v], val, in);
        }
#pragma unroll
        for (int tau = 0; tau < NT; ++tau)
#pragma unroll
            for (int j = 0; j < 8; ++j) b[tau][j] = bn[tau][j];
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        st[v] = pw_merge(st[v], pw_xor(st[v], 1));
        st[v] = pw_merge(st[v], pw_xor(st[v], 2));
        st[v] = pw_merge(st[v], pw_xor(st[v], 4));
        st[v] = pw_merge(st[v], pw_xor(st[v], 8));
    }
    if (m == 0) {
        constexpr int NS = PwSlots<T>::N;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (i0 + v < n) PwSlots<T>::store(partials + ((size_t)chunk * n + (i0 + v)) * NS, st[v]);   // (masked, not padded)
    }
}

// the second stage: one thread per data row merges the row's G partials in index order (G = 0: the empty statistics)
template <typename T>
__global__ void __launch_bounds__(256) glm_pointwise_combine_kernel(const double *__restrict__ partials, double *__restrict__ stats, int n, int G) {
    constexpr int NS = PwSlots<T>::N;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T r = PwSlots<T>::empty();
    for (int c = 0; c < G; ++c) r = pw_merge(r, PwSlots<T>::load(partials + ((size_t)c * n + i) * NS));
    PwSlots<T>::store(stats + (size_t)i * NS, r);
}

// ------------------------------------------------------------------------------------------------
// host side
int glm_pointwise_groups(int S, int n) {
    if (S <= 0 || n <= 0) return 0;
    const long ntiles = ((long)S + GLMPW_TILE - 1) / GLMPW_TILE, rg = (n + 63) / 64;
    long G = (GLMPW_TARGET_GROUPS + rg - 1) / rg;
    const long cap = GLMPW_MAX_PARTIAL_ROWS / n, fill = (ntiles + GLMPW_MIN_TILES - 1) / GLMPW_MIN_TILES;
    if (G > cap) G = cap;
    if (G > fill) G = fill;
    return (int)(G < 1 ? 1 : G);
}

template <int NT, int FAM, int PRED>
static hipError_t glm_pointwise_launch_k(const GlmSpec &gl, const float *t, double *partials, int S, int G, hipStream_t st) {
    hipLaunchKernelGGL((glm_pointwise_kernel<NT, FAM, PRED>), dim3((gl.n + 63) / 64, G), dim3(256), 0, st, gl, t, partials, S, G);
    return hipGetLastError();
}

template <int FAM, int PRED>
static hipError_t glm_pointwise_launch_f(const GlmSpec &gl, const float *t, double *partials, int S, int G, hipStream_t st) {
    switch ((gl.D + 31) / 32) {   // (NT: the lane's 8 NT columns, 32 NT >= D)
        case 1: return glm_pointwise_launch_k<1, FAM, PRED>(gl, t, partials, S, G, st);
        case 2: return glm_pointwise_launch_k<2, FAM, PRED>(gl, t, partials, S, G, st);
        case 3: return glm_pointwise_launch_k<3, FAM, PRED>(gl, t, partials, S, G, st);
        case 4: return glm_pointwise_launch_k<4, FAM, PRED>(gl, t, partials, S, G, st);
    }
    return hipErrorInvalidConfiguration;
}

hipError_t launch_glm_pointwise(const GlmSpec &gl, const float *t, double *stats, double *partials, int S, int predict, hipStream_t st) {
    const int G = glm_pointwise_groups(S, gl.n);
    hipError_t e = hipSuccess;
    if (G > 0) {
        const int key = 2 * gl.family + (predict ? 1 : 0);
        switch (key) {
            case 2 * GLM_LOGISTIC: e = glm_pointwise_launch_f<GLM_LOGISTIC, 0>(gl, t, partials, S, G, st); break;
            case 2 * GLM_LOGISTIC + 1: e = glm_pointwise_launch_f<GLM_LOGISTIC, 1>(gl, t, partials, S, G, st); break;
            case 2 * GLM_POISSON: e = glm_pointwise_launch_f<GLM_POISSON, 0>(gl, t, partials, S, G, st); break;
            case 2 * GLM_POISSON + 1: e = glm_pointwise_launch_f<GLM_POISSON, 1>(gl, t, partials, S, G, st); break;
            default: return hipErrorInvalidConfiguration;
        }
        if (e != hipSuccess) return e;
    }
    const dim3 grid((gl.n + 255) / 256);
    if (predict) hipLaunchKernelGGL(glm_pointwise_combine_kernel<PwMoments>, grid, dim3(256), 0, st, partials, stats, gl.n, G);
    else hipLaunchKernelGGL(glm_pointwise_combine_kernel<PwStats>, grid, dim3(256), 0, st, partials, stats, gl.n, G);
    return hipGetLastError();
}

}  // namespace nnest
