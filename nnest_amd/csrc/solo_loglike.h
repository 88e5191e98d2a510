// solo_loglike.h -- the analytic likelihoods on a solo wave (one walker per wave, solo_tile.h layout): shared by the proposal
// kernels of nnest_solo.hip and the ensemble kernel of nnest_ensemble.hip.
#pragma once
#include "solo_tile.h"

namespace nnest {

// ---- likelihoods on a solo wave (the per-term arithmetic of loglike_tile, flow_tile.h; sums over the 16 positions) ----
#pragma clang fp contract(off)
// ld_ride: if given, the lane's log-det partial, replaced by the walker's total (solo_logdet_total) -- its reduction rides in the
// wait states of the likelihood's own row sum where there is one (Rosenbrock: solo_logdet_total_and_row_sum), same bits either way.
template <int U, int LK>   // LK >= 0: the likelihood id is known at compile time (the other branches are not instantiated)
static __device__ __forceinline__ double solo_loglike(const LikeSpec &lk_in, int D, int lane, const float (&xs)[2][U], float *ld_ride = nullptr) {
    struct { int id; float scale; const float *p; } lk = {LK >= 0 ? LK : lk_in.id, lk_in.scale, lk_in.p};
    if (ld_ride && lk.id != 0) *ld_ride = solo_logdet_total(*ld_ride);
    const int m = lane & 15;
    const float scale = lk.scale;
    float th[2 * U + 1];
#pragma unroll
    for (int u = 0; u < U; ++u) { th[2 * u] = scale * xs[0][u]; th[2 * u + 1] = scale * xs[1][u]; }
    double acc;
    if (lk.id == 0) {
        // Rosenbrock (likelihoods.py:51): -sum_i 100 (x[i+1] - x[i]^2)^2 + (1 - x[i])^2, i = 0..D-2
        th[2 * U] = solo_ror<15>(th[0]);  // first dim of position m + 1
        float facc = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * U; ++k) {
            const int i = 2 * U * m + k;
            float a = th[k] * th[k];
            float b = th[k + 1] - a;
            float c = b * b;
            float e = 100.0f * c;
            float f = 1.0f - th[k];
            float q = f * f;
            float term = e + q;
            facc = facc + ((i + 1 < D) ? term : 0.f);
        }
        if (ld_ride) solo_logdet_total_and_row_sum(*ld_ride, facc);
        else facc = solo_row_sum(facc);
        acc = -(double)facc;
    } else if (lk.id == 1) {
        // GaussianMix (likelihoods.py:165-189): logsumexp_k[ log w_k - |theta - mu_k|^2/2 - (D/2) log 2pi ]
        float facc = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * U; ++k) {
            const int d = 2 * U * m + k;
            float sq = th[k] * th[k];
            facc = facc + ((d >= 2 && d < D) ? sq : 0.f);
        }
        const double base = (double)solo_row_sum(facc);
        const float t0 = solo_lane0(th[0]), t1 = solo_lane0(th[1]);  // theta[0], theta[1]: position 0
        const float mu0[4] = {0.f, 0.f, 4.f, -4.f}, mu1[4] = {4.f, -4.f, 0.f, 0.f};
        const double lw[4] = {-0.916290731874155, -1.203972804325936, -1.6094379124341003, -2.302585092994046};
        double l[4], mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a = t0 - mu0[k], b = t1 - mu1[k];
            double s = base + (double)(a * a) + (D > 1 ? (double)(b * b) : 0.0);
            l[k] = -(s * 0.5) - 0.9189385332046727 * (double)D + lw[k];
            mx = l[k] > mx ? l[k] : mx;
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) se += __expf((float)(l[k] - mx));
        acc = mx + (double)__logf(se);
    } else if (lk.id == 2) {
        // Himmelblau (likelihoods.py:70) summed over consecutive pairs (x[2i], x[2i+1])
        float facc = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d1 = 2 * U * m + 2 * u + 1;
            float x0 = th[2 * u], x1 = th[2 * u + 1];
            float a = x0 * x0 + x1 - 11.f;
            float b = x0 + x1 * x1 - 7.f;
            float v = -(a * a) - b * b;
            facc = facc + ((d1 < D) ? v : 0.f);
        }
        acc = (double)solo_row_sum(facc);
    } else if (lk.id == 4) {
        // Eggbox (likelihoods.py:104-106), x_dim = 2
        const float t0 = solo_lane0(th[0]), t1 = solo_lane0(th[1]);
        float chi = cosf(t0 / 2.f) * cosf(t1 / 2.f);
        float b = 2.f + chi;
        float b2 = b * b;
        acc = (double)(b2 * b2 * b);
    } else {
        // float64 moments of theta (Gaussian, GaussianShell, DoubleGaussianShell: loglike_tile, flow_tile.h)
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * U; ++k) {
            const bool valid = 2 * U * m + k < D;
            const double t = valid ? (double)th[k] : 0.0;
            s1 += t;
            s2 += t * t;
        }
#pragma unroll
        for (int o = 1; o <= 8; o <<= 1) {  // totals over the 16 positions, identical in every lane of a row
            s1 = s1 + __shfl_xor(s1, o);
            s2 = s2 + __shfl_xor(s2, o);
        }
        const double Dd = (double)D;
        if (lk.id == 3) {
            const double c = (double)lk.p[0];
            const double quad = (s2 - c * s1 * s1 / (1.0 + (Dd - 1.0) * c)) / (1.0 - c);
            const double logdet = (Dd - 1.0) * log(1.0 - c) + log(1.0 + (Dd - 1.0) * c);
            acc = -0.5 * quad - 0.5 * logdet - 0.9189385332046727 * Dd;
        } else {
            double sh[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double sig = (double)lk.p[3 * k], rs = (double)lk.p[3 * k + 1], cen = (double)lk.p[3 * k + 2];
                double r2 = s2 - 2.0 * cen * s1 + Dd * cen * cen;
                double rad = sqrt(r2 < 0.0 ? 0.0 : r2);   // (a NaN moment stays NaN: the safe rule maps the row)
                sh[k] = -((rad - rs) * (rad - rs)) / (2.0 * sig * sig);
            }
            if (lk.id == 5) acc = sh[0];
            else {
                const double mx = sh[0] > sh[1] ? sh[0] : sh[1], mn = sh[0] > sh[1] ? sh[1] : sh[0];
                acc = mx + log1p(exp(mn - mx));
            }
        }
    }
    if (!(fabs(acc) <= 1.79769313486231570e308)) acc = -1e100;  // logl[~isfinite] = -1e100   sampler.py:128
    return acc;
}
#pragma clang fp contract(fast)

}  // namespace nnest
