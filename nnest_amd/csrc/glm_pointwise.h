// glm_pointwise.h -- the POINTWISE PREDICTIVE STATISTICS of the regression likelihoods (include/nnest_hip.h nnest_glm_pointwise,
// nnest_glm_predict; nnest_glm_pointwise.hip): the running statistics of one data row over the draws, their merge,
// the size of the partials and the launchers' declarations.  glm_data.h has the descriptor and the term; the reduction here runs
// the other way from its kernels': over the draws per data row, not over the rows per draw.
#pragma once
#include "glm_data.h"

namespace nnest {

constexpr int GLMPW_TILE = 16;             // draws per pass of a wave's loop: one MFMA tile
constexpr int GLMPW_MIN_TILES = 4;         // a draw group gets at least this many tiles, but the last one of a short run
constexpr int GLMPW_TARGET_GROUPS = 1024;  // workgroups to aim for: four a CU of the largest part, whatever the device is
constexpr int GLMPW_MAX_DRAWS = 1 << 30;
constexpr long GLMPW_MAX_PARTIAL_ROWS = 65536;   // G n <= this (4 MB of partials), beside G >= 1

#pragma clang fp contract(off)
// a running max-shifted sum: m = the largest value seen (-inf: none), s1 = sum e^(v - m), s2 = sum e^(2 (v - m))
struct PwShift { double m, s1, s2; };
// the statistics of one data row over a set of draws (stats_dev[i][0 .. 7] in this order)
struct PwStats {
    PwShift p;   // of l:  a, P (its s2 is not kept by the caller)
    PwShift q;   // of -l: b, Q, Q2
    double n, mean, m2;
};
struct PwMoments { double n, mean, m2; };   // nnest_glm_predict's three

__host__ __device__ __forceinline__ PwShift pw_shift_empty() { return PwShift{-INFINITY, 0.0, 0.0}; }
__host__ __device__ __forceinline__ PwMoments pw_moments_empty() { return PwMoments{0.0, 0.0, 0.0}; }
__host__ __device__ __forceinline__ PwStats pw_empty() { return PwStats{pw_shift_empty(), pw_shift_empty(), 0.0, 0.0, 0.0}; }

// one finite value more: ONE exponential, whichever side of the maximum it falls
__device__ __forceinline__ void pw_shift_add(PwShift &r, double v) {
    const double d = v - r.m;                 // (+inf on the first value)
    const double e = exp(-fabs(d));           // (0 then)
    const bool up = d > 0.0;
    r.s1 = up ? r.s1 * e + 1.0 : r.s1 + e;
    r.s2 = up ? r.s2 * (e * e) + 1.0 : r.s2 + e * e;
    r.m = up ? v : r.m;
}
// Welford's step: Chan's rule with a set of one
__device__ __forceinline__ void pw_moments_add(double &n, double &mean, double &m2, double v) {
    n += 1.0;
    const double d = v - mean;
    mean += d / n;
    m2 += d * (v - mean);
}
// one pair more (`counted`: a row and a draw of the launch; a dead pair -- the value NaN or +-inf -- is not counted)
__device__ __forceinline__ void pw_add(PwStats &r, double l, bool counted) {
    if (!(counted && fabs(l) <= 1.79769313486231570e308)) return;
    pw_shift_add(r.p, l);
    pw_shift_add(r.q, -l);
    pw_moments_add(r.n, r.mean, r.m2, l);
}
__device__ __forceinline__ void pw_add(PwMoments &r, double mu, bool counted) {
    if (!(counted && fabs(mu) <= 1.79769313486231570e308)) return;
    pw_moments_add(r.n, r.mean, r.m2, mu);
}

// the statistics of the union of two sets of draws.  Symmetric in their arguments, operation by operation (importance_merge's
// idiom): both sides of a butterfly exchange hold the same bits
__host__ __device__ __forceinline__ PwShift pw_merge(const PwShift &p, const PwShift &q) {
    PwShift r;
    r.m = p.m > q.m ? p.m : q.m;
    const double ep = p.m == r.m ? 1.0 : exp(p.m - r.m), eq = q.m == r.m ? 1.0 : exp(q.m - r.m);   // (-inf beside -inf: 1, on sums of 0)
    r.s1 = p.s1 * ep + q.s1 * eq;
    r.s2 = p.s2 * (ep * ep) + q.s2 * (eq * eq);
    return r;
}
// Chan, Golub & LeVeque's rule for (count, mean, M2); the mean as the weighted mean of the two, which is symmetric
__host__ __device__ __forceinline__ PwMoments pw_merge(const PwMoments &p, const PwMoments &q) {
    if (p.n == 0.0) return q.n == 0.0 ? PwMoments{0.0, 0.0, 0.0} : q;   // (an empty side leaves the other's bits as they are)
    if (q.n == 0.0) return p;
    PwMoments r;
    r.n = p.n + q.n;
    const double d = p.mean > q.mean ? p.mean - q.mean : q.mean - p.mean;
    r.mean = (p.n * p.mean + q.n * q.mean) / r.n;
    r.m2 = (p.m2 + q.m2) + (d * d) * ((p.n * q.n) / r.n);
    return r;
}
__host__ __device__ __forceinline__ PwStats pw_merge(const PwStats &p, const PwStats &q) {
    const PwMoments m = pw_merge(PwMoments{p.n, p.mean, p.m2}, PwMoments{q.n, q.mean, q.m2});
    return PwStats{pw_merge(p.p, q.p), pw_merge(p.q, q.q), m.n, m.mean, m.m2};
}
#pragma clang fp contract(fast)

// the layout of a row's statistics in memory: 8 doubles (nnest_glm_pointwise), 3 (nnest_glm_predict)
template <typename T> struct PwSlots;
template <> struct PwSlots<PwStats> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void store(double *o, const PwStats &r) {
        o[0] = r.p.m; o[1] = r.p.s1; o[2] = r.q.m; o[3] = r.q.s1; o[4] = r.q.s2; o[5] = r.n; o[6] = r.mean; o[7] = r.m2;
    }
    __device__ static __forceinline__ PwStats load(const double *o) {
        return PwStats{PwShift{o[0], o[1], 0.0}, PwShift{o[2], o[3], o[4]}, o[5], o[6], o[7]};
    }
    __device__ static __forceinline__ PwStats empty() { return pw_empty(); }
};
template <> struct PwSlots<PwMoments> {
    static constexpr int N = 3;
    __device__ static __forceinline__ void store(double *o, const PwMoments &r) { o[0] = r.n; o[1] = r.mean; o[2] = r.m2; }
    __device__ static __forceinline__ PwMoments load(const double *o) { return PwMoments{o[0], o[1], o[2]}; }
    __device__ static __forceinline__ PwMoments empty() { return pw_moments_empty(); }
};

// ---- the wave's operands, shared by every kernel that streams the draws in this layout (nnest_glm_pointwise.hip, nnest_glm_psis.hip):
// lane = 16 g + m.  The same loads and the same MFMA order give the same bits of eta in each of them. ----
// the tile's operand: of draw min(s, S - 1), the columns 32 tau + 8 g + j
template <int NT>
__device__ __forceinline__ void pw_load_tile(const float *__restrict__ t, long s, int S, int D, int g, float (&b)[NT][8]) {
    const float *row = t + (size_t)(s < S ? s : S - 1) * D;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 32 * tau + 8 * g + j;
            const float v = row[min(c, D - 1)];
            b[tau][j] = c < D ? v : 0.f;
        }
}
// the invariant operand: A[16 rb + m, 32 tau + 8 g + j], read once from at
template <int NT>
__device__ __forceinline__ void pw_load_a(const GlmSpec &gl, int rb, int m, int g, float (&a)[NT][8]) {
    const int D = gl.D;
    const size_t ld = (size_t)gl.ld;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 32 * tau + 8 * g + j;
            const float v = gl.at[(size_t)min(c, D - 1) * ld + 16 * rb + m];   // (no read past [D, ld])
            a[tau][j] = c < D ? v : 0.f;
        }
}

// nnest_glm_pointwise.hip.  G, the draw groups of S draws over n rows (the partials are [G, n, slots]): enough for
// GLMPW_TARGET_GROUPS workgroups at ceil(n / 64) row groups, at least GLMPW_MIN_TILES tiles of draws each, G n bounded.  A function
// of (S, n) alone -- not of the device: the same call gives the same bits on any part
int glm_pointwise_groups(int S, int n);
// predict = 0: stats [n, 8], partials [G, n, 8]; 1: stats [n, 3], partials [G, n, 3].  S = 0 writes the empty statistics
hipError_t launch_glm_pointwise(const GlmSpec &gl, const float *t, double *stats, double *partials, int S, int predict, hipStream_t st);

}  // namespace nnest
