// mcmc_gdata.h -- the GAUSSIAN LIKELIHOOD FROM USER DATA of the fused Metropolis runs (include/nnest_hip.h nnest_mcmc_gdata_steps;
// nnest_mcmc_gdata.hip: the NVP's one-walker-per-wave kernel and the likelihood alone; nnest_spline_mcmc_gdata.hip: the spline
// flow's tile kernel): the adaptive walk (mcmc_adapt.h, unchanged) with
//   logL(t) = logl0 - 1/2 |R (t - mu)|^2,   R upper triangular, R^T R = the precision matrix,
// in place of the analytic likelihoods.  Here are the likelihood in both layouts, the arguments and the launchers' declarations.
// The arithmetic, with t = T(x) the float32 row:
//   d_c = t_c - mu_c                       float32, one rounding
//   y_r = sum_{c >= r} R[r, c] d_c         float32, in the layout's own order, fused multiply-adds
//   q   = sum_r (double)y_r (double)y_r    float64, in a fixed order: the same bits on every lane that holds the walker
//   logL = logl0 - 0.5 q, -1e100 where that is not finite (the rule of the known likelihoods).
// R is read from global memory, row-major [D, D], through the caches: every walker reads the same D^2 floats.
#pragma once
#include "mcmc_adapt.h"
#include "solo_tile.h"

namespace nnest {

// the descriptor on the device side (nnest_gdata_t, checked)
struct GdataSpec {
    const float *mu;   // [D]
    const float *r;    // [D, D] row-major, upper triangular
    double logl0;
    int D;
};

// the arguments of a launch: the adaptive launch's (its `like` unused), the descriptor beside them.  A type of its own: the
// adaptive kernels keep the arguments -- and with them the code -- they had
struct McmcGdataArgs : McmcAdaptArgs {
    GdataSpec gd;
};

#pragma clang fp contract(off)
// logL from q: the safe rule of solo_loglike / loglike_tile
__device__ __forceinline__ double gdata_finish(double logl0, double q) {
    double acc = logl0 - 0.5 * q;   // (0.5 q is exact)
    if (!(fabs(acc) <= 1.79769313486231570e308)) acc = -1e100;
    return acc;
}
#pragma clang fp contract(fast)

// ---- the solo layout (solo_tile.h): lane = 16 g + p holds dims 2U p + 2u + c of the walker's row; the four 16-lane rows g hold
// copies.  Copy g takes the rows r = g, g + 4, ... of R: the 16 positions read R[r, :] as one coalesced run, each multiplies its 2U
// columns, solo_row_sum (DPP row rotations: the same bits on all 16 positions) makes y_r, and the copy adds y_r^2 up in float64 in
// the order of r.  The four partial sums meet in a butterfly over the copies (xor 16, xor 32): float64 addition commutes, so every
// lane of the wave ends with the same bits.  gmu: the lane's dims of mu (padded dims 0: there t is 0 too, and d) ----
template <int U>
__device__ __forceinline__ double gdata_solo_loglike(const GdataSpec &gd, int lane, const float (&tx)[2][U], const float (&gmu)[2][U]) {
    const int D = gd.D, pos = lane & 15, g = lane >> 4;
    const int c0 = 2 * U * pos;
    float d[2 * U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) d[2 * u + c] = tx[c][u] - gmu[c][u];
    double q = 0.0;
    const int nj = (D + 3) >> 2;
    for (int j = 0; j < nj; ++j) {
        const int r = 4 * j + g;
        const float *rr = gd.r + (size_t)r * D + c0;
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * U; ++k) {
            const int c = c0 + k;
            const float w = (r < D && c >= r && c < D) ? rr[k] : 0.f;   // (the lower triangle is not read; no read past [D, D])
            part = fmaf(w, d[k], part);
        }
        const float y = solo_row_sum(part);
        q += (double)y * (double)y;   // (the product of two float32 is exact in float64)
    }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    return gdata_finish(gd.logl0, q);
}

// the lane's dims of mu, once per kernel
template <int U>
__device__ __forceinline__ void gdata_solo_mu(const GdataSpec &gd, int pos, float (&gmu)[2][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int dd = 2 * U * pos + 2 * u + c;
            gmu[c][u] = dd < gd.D ? gd.mu[dd] : 0.f;
        }
}

// ---- the team tile (flow_tile.h, spline_latent.h): lane = 16 g + m holds, of walker m, the dims 32 tau + 8 g + j (j = 0 .. 7;
// class c = j & 1, component j >> 1 of tx[c][tau]).  y^T = R d^T is a [D x D] [D x 16] product on the matrix cores, 16 rows of R to
// an accumulator, v_mfma_f32_16x16x4f32 (mfma4): K-step (tau, j) takes the four columns 32 tau + 8 k + j (k = 0 .. 3) -- lane
// (m, g) gives A[m][g] = R[16 rb + m, 32 tau + 8 g + j] and B[g][m] = d of walker m at that column, which it holds --, and the
// accumulator of lane (m, g) ends with y_r, r = 16 rb + 4 g + v (v = 0 .. 3), of walker m.  The column blocks tau with
// 32 (tau + 1) <= 16 rb lie wholly in the lower triangle and are skipped.  q is summed in float64 in the order (rb, v) and over the
// four lane groups by group_sum: the same bits on the four lane groups; every wave computes the whole product from the same
// operands in the same order, so the four waves agree without an exchange.  gmu: [32 NT] in LDS, padded dims 0 ----
template <int NT>
__device__ __forceinline__ double gdata_tile_loglike(const GdataSpec &gd, int lane, const f32x4 (&tx)[2][NT], const float *gmu) {
    const int D = gd.D, m = lane & 15, g = lane >> 4;
    float d[NT][8];
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(gmu + 32 * tau + 8 * g);
        const f32x4 m0 = p[0], m1 = p[1];
        d[tau][0] = tx[0][tau].x - m0.x; d[tau][1] = tx[1][tau].x - m0.y; d[tau][2] = tx[0][tau].y - m0.z; d[tau][3] = tx[1][tau].y - m0.w;
        d[tau][4] = tx[0][tau].z - m1.x; d[tau][5] = tx[1][tau].z - m1.y; d[tau][6] = tx[0][tau].w - m1.z; d[tau][7] = tx[1][tau].w - m1.w;
    }
    double q = 0.0;
#pragma unroll
    for (int rb = 0; rb < 2 * NT; ++rb) {
        if (16 * rb >= D) break;   // (uniform)
        const int r = 16 * rb + m;
        const float *rr = gd.r + (size_t)r * D;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tau = rb / 2; tau < NT; ++tau) {
            const int c0 = 32 * tau + 8 * g;
            float a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = (r < D && c0 + j >= r && c0 + j < D) ? rr[c0 + j] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = mfma4(a[j], d[tau][j], acc);
        }
        q += (double)acc.x * (double)acc.x;
        q += (double)acc.y * (double)acc.y;
        q += (double)acc.z * (double)acc.z;
        q += (double)acc.w * (double)acc.w;
    }
    q = group_sum(q);
    return gdata_finish(gd.logl0, q);
}

hipError_t launch_loglike_gdata(const GdataSpec &gd, const float *t, double *logl, int N, hipStream_t st);
hipError_t launch_mcmc_gdata(const FlowShape &s, const float *packed, const McmcGdataArgs &a, hipStream_t st);
// hipErrorInvalidConfiguration: a shape the team tile is not instantiated for (a.C <= 0: the shape's verdict, nothing is launched)
hipError_t launch_spline_mcmc_gdata(const SplArgs &q, const McmcGdataArgs &a, hipStream_t st);
// nnest_abi.hip: the check of a descriptor against the flow's x_dim (sets the error string), and the descriptor checked
int gdata_ok(const nnest_gdata_t *gdata, int D, GdataSpec *out);

}  // namespace nnest
