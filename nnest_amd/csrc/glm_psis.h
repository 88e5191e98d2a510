// glm_psis.h -- PARETO-SMOOTHED LEAVE-ONE-OUT of the regression likelihoods and the matrix of their terms (include/nnest_hip.h
// nnest_glm_psis, nnest_glm_terms; nnest_glm_psis.hip): the sizes, the layout of the work buffer and of a row's
// result, and the launchers' declarations.  glm_pointwise.h has the wave's operands and the draw groups; the kernels here stream the
// draws in its layout, so that eta -- and with it every term -- has the bits nnest_glm_pointwise saw.
#pragma once
#include "glm_pointwise.h"

namespace nnest {

constexpr int GLMPSIS_MAX_DRAWS = 1 << 20;           // all S draws of one call are resident; thin a longer run
constexpr int GLMPSIS_SORT = 4096;                   // the fit kernel's sort buffer in LDS: a power of two >= the tail of 2^20 draws
constexpr long long GLMPSIS_MAX_WORK = 1ll << 30;    // bytes of work_dev
constexpr long long GLMPSIS_MAX_TERMS = 1ll << 30;   // S n of nnest_glm_terms (8 GiB of float64)
constexpr int GLMPSIS_SLOTS = 16;                    // doubles of a row's result
constexpr int GLMPSIS_KEY_SHIFT = 40;                // key(d) = the pattern of d >> 40: sign, exponent, 12 bits of the mantissa
// flag bits (slot 11)
constexpr int GLMPSIS_F_DROPPED = 1, GLMPSIS_F_NOFIT = 2, GLMPSIS_F_BADK = 4;

// ceil(3 sqrt(c)): the smallest integer m with m^2 >= 9 c, in integer arithmetic
__host__ __device__ __forceinline__ long long psis_ceil3sqrt(long long c) {
    long long m = (long long)sqrt(9.0 * (double)c);
    while (m * m < 9 * c) ++m;
    while (m > 0 && (m - 1) * (m - 1) >= 9 * c) --m;
    return m;
}
// M* of a row with cnt live draws
__host__ __device__ __forceinline__ long long psis_tail_target(long long cnt) {
    const long long a = cnt / 5, b = psis_ceil3sqrt(cnt);
    return a < b ? a : b;
}
// Mcap: the slots of a row's tail buffer, from S alone (>= M* of any cnt <= S)
inline int glm_psis_tail_cap(int S) { return S <= 0 ? 1 : (int)psis_ceil3sqrt(S); }

// work_dev, in bytes from its start (every part a multiple of 8):
//   tail      [n, Mcap] float64      row i's tail, sorted ascending in d, in its first M_i slots
//   partials  [max(G, 1), n, 3] float64   the draw groups' body sums
//   hist      [n, 256] uint32        the digit counts of the pass in hand
//   sel       [n, 2] uint32          {prefix of the key found so far, draws below it}
//   counter   [n] uint32 (+ 1 pad where n is odd)   the tail slots handed out
struct GlmPsisWork {
    long long tail, partials, hist, sel, counter, bytes;
    int mcap, G;
};
inline GlmPsisWork glm_psis_work(int S, int n) {
    GlmPsisWork w;
    w.mcap = glm_psis_tail_cap(S);
    w.G = glm_pointwise_groups(S, n);
    w.tail = 0;
    w.partials = w.tail + 8ll * n * w.mcap;
    w.hist = w.partials + 8ll * (w.G < 1 ? 1 : w.G) * n * 3;
    w.sel = w.hist + 4ll * n * 256;
    w.counter = w.sel + 8ll * n;
    w.bytes = w.counter + 4ll * (n + (n & 1));
    return w;
}

// nnest_glm_psis.hip
hipError_t launch_glm_terms(const GlmSpec &gl, const float *t, double *out, int S, hipStream_t st);
// stats [n, 8] of nnest_glm_pointwise for the same draws; out [n, GLMPSIS_SLOTS]; work as glm_psis_work lays it out
hipError_t launch_glm_psis(const GlmSpec &gl, const float *t, const double *stats, double *out, void *work, int S, hipStream_t st);

}  // namespace nnest
