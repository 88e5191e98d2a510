// nnest_chain_stats.hip -- chain statistics of a batch of MCMC histories x[C, T, D] on the device: the acceptance rate, the mean
// jump distance, the lag autocorrelations and the effective sample size, and the Gelman-Rubin R-hat, as the reference computes
// them on the host (nnest/utils/evaluation.py; Sampler._chain_stats, nnest/sampler.py:474-492).  Definitions and the reference's
// quirks (the autocorrelation divided by the STANDARD DEVIATION, the global stop of the ESS sum) in include/nnest_hip.h.
//
// Launches (all plain multi-launch, no grid-wide wait, no float atomics):
//   k_chain        one workgroup per chain: per-dimension mean and variance over the steps, accepted pairs, sum of jump lengths
//   k_chain_sum    the per-chain table summed over chains in a fixed order -> the additive chain sums
//   k_prepare      mean / std (given, or from the chain sums), ESS state reset
//   k_lags         the hot path: sum_i sum_{j<T-s} y_ij y_i,j+s for a block of lags, y = T(x) - mu in f32.  A workgroup owns a
//                  group of chains and <= 64 dimensions; per chain, steps in tiles of JT: rows j0.. of the tile (A) and rows j0+s0..
//                  (B, JT + LB of them) are staged in LDS, zero beyond T; a lane owns (8 consecutive lags, one dimension) and slides
//                  8-row windows of A and B: 64 f32 FMAs per 16 LDS reads.  Tile sums (<= JT products) in f32, flushed into f64
//                  per tile; per-workgroup partials in f64.
//   k_lag_reduce   the partials summed over chain groups in a fixed order -> the additive lag sums of the block
//   k_advance      p_s = lag sum / (C (T - s) sd), the global stop test and the ESS sum over the block; later blocks are skipped
//                  on the device once the stop lag is known
//   k_finish       ESS, R-hat, acceptance, jump -> out
// emcee's normalised autocorrelation function (a different estimator: per-walker mean and normalisation, every lag, float64) has
// its own two kernels further down, k_ac_moments and k_ac_lags, and shares k_lag_reduce.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "nnest_internal.h"

namespace {

constexpr int LB = 256;       // lags per block (one block covers every lag of T <= 257)
constexpr int RL = 8;         // lags per lane
constexpr int JT = 128;       // steps per LDS tile
constexpr int DT = 32;        // dimensions per workgroup
constexpr int NCG = 256;      // chain groups (fixed: the sums do not depend on the device)
constexpr int MMAX = 8;       // blocks of LB lags per launch at most
constexpr int LAG_THREADS = 1024;
constexpr int LAG_ITEMS = (LB / RL) * DT / LAG_THREADS;   // items per thread (1)
static_assert((LB / RL) * DT % LAG_THREADS == 0, "item split");
static_assert(JT % RL == 0 && LB % RL == 0, "tile split");

// work layout (doubles)
struct Layout {
    size_t tab, mu, sd, e, center, state, sums, lag_sums, partial, total;
    Layout(int C, int D) {
        const size_t ncg = C < NCG ? C : NCG;
        size_t o = 0;
        tab = o;      o += (size_t)C * (2 * D + 2);
        mu = o;       o += D;
        sd = o;       o += D;
        e = o;        o += D;
        center = o;   o += D;
        state = o;    o += 4;
        sums = o;     o += 3 + 3 * (size_t)D;
        lag_sums = o; o += (size_t)MMAX * LB * D;
        partial = o;  o += (ncg > (size_t)MMAX ? ncg : (size_t)MMAX) * LB * D;   // k_lags: ncg' * m <= max(min(C, NCG), m)
        total = o;
    }
};

__device__ __forceinline__ double tr(float x, const double *aff, int D, int d) {
    // T(x) = x * a + b rounded as numpy rounds x * std + mean (no contraction)
    return aff ? __dadd_rn(__dmul_rn((double)x, aff[d]), aff[D + d]) : (double)x;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- per chain ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chain(const float *__restrict__ x, int T, int D, long long cs, long long ss,
                                                const double *__restrict__ aff, double *__restrict__ tab) {
    __shared__ double r1[256], r2[256];
    __shared__ double wj[4], wc[4];
    const int i = blockIdx.x, t = threadIdx.x;
    const float *xc = x + (long long)i * cs;
    double *row = tab + (size_t)i * (2 * D + 2);
    const int Dc = D < 256 ? D : 256;
    const int nsl = 256 / Dc;
    for (int db = 0; db < D; db += Dc) {
        const int d = db + t % Dc, sl = t / Dc;
        double s1 = 0.0, s2 = 0.0;
        if (sl < nsl && d < D) {
            const double v0 = tr(xc[d], aff, D, d);
            for (int j = sl; j < T; j += nsl) {
                const double u = tr(xc[(long long)j * ss + d], aff, D, d) - v0;
                s1 += u;
                s2 += u * u;
            }
        }
        r1[t] = s1;
        r2[t] = s2;
        __syncthreads();
        if (t < Dc && d < D) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < nsl; ++k) {
                a += r1[k * Dc + t];
                b += r2[k * Dc + t];
            }
            const double m = a / T;
            row[d] = tr(xc[d], aff, D, d) + m;           // theta_i
            row[D + d] = fmax(b / T - m * m, 0.0);        // sigma^2_i (ddof 0)
        }
        __syncthreads();
    }
    // consecutive pairs: wave w takes j = 1 + w, 5 + w, ...; lanes over the dimensions
    const int w = t >> 6, l = t & 63;
    double jump = 0.0, cnt = 0.0;
    for (int j = 1 + w; j < T; j += 4) {
        const float *pa = xc + (long long)(j - 1) * ss, *pb = xc + (long long)j * ss;
        double q = 0.0;
        int diff = 0;
        for (int d = l; d < D; d += 64) {
            const double va = tr(pa[d], aff, D, d), vb = tr(pb[d], aff, D, d);
            diff |= !(va == vb);
            const double dd = va - vb;
            q += dd * dd;
        }
        q = wave_sum(q);
        jump += sqrt(q);
        cnt += __any(diff) ? 1.0 : 0.0;
    }
    if (l == 0) {
        wj[w] = jump;
        wc[w] = cnt;
    }
    __syncthreads();
    if (t == 0) {
        row[2 * D] = wc[0] + wc[1] + wc[2] + wc[3];
        row[2 * D + 1] = ((wj[0] + wj[1]) + wj[2]) + wj[3];
    }
}

// block b < D: sums over chains of theta - c, (theta - c)^2, sigma^2 for dimension b, about the centre c = center[b] (the same on
// every shard of a batch) or the first chain's theta; block D: accepted pairs, jump, chain count.  c is kept in the work area.
__global__ __launch_bounds__(256) void k_chain_sum(const double *__restrict__ tab, int C, int D, const double *__restrict__ center,
                                                   double *__restrict__ center_out, double *__restrict__ sums) {
    __shared__ double r[3][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int W = 2 * D + 2;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const double c = b < D ? (center ? center[b] : tab[b]) : 0.0;
    for (int i = t; i < C; i += 256) {
        const double *row = tab + (size_t)i * W;
        if (b < D) {
            const double th = row[b] - c;
            a0 += th;
            a1 += th * th;
            a2 += row[D + b];
        } else {
            a0 += row[2 * D];
            a1 += row[2 * D + 1];
        }
    }
    r[0][t] = a0;
    r[1][t] = a1;
    r[2][t] = a2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            r[0][t] += r[0][t + o];
            r[1][t] += r[1][t + o];
            r[2][t] += r[2][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (b < D) {
            center_out[b] = c;
            sums[3 + b] = r[0][0];
            sums[3 + D + b] = r[1][0];
            sums[3 + 2 * D + b] = r[2][0];
        } else {
            sums[0] = r[0][0];
            sums[1] = r[1][0];
            sums[2] = (double)C;
        }
    }
}

// var = mean_i sigma2_i + mean_i (theta_i - c)^2 - (mean_i theta_i - c)^2: centred sums, no large-moment cancellation
__global__ void k_prepare(const double *__restrict__ sums, int D, const double *__restrict__ mean, const double *__restrict__ stdv,
                          const double *__restrict__ center, double *__restrict__ mu, double *__restrict__ sd, double *__restrict__ e,
                          double *__restrict__ state) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < D) {
        const double C = sums[2];
        const double m = sums[3 + d] / C;
        mu[d] = mean ? mean[d] : center[d] + m;
        sd[d] = stdv ? stdv[d] : sqrt(fmax(sums[3 + 2 * D + d] / C + (sums[3 + D + d] / C - m * m), 0.0));
        e[d] = 1.0;
    }
    if (d < 4) state[d] = 0.0;
}

// ---- lag block ------------------------------------------------------------------------------------------------------
// grid (ncg, m, ceil(D / DT)); partial [ncg][m * LB][D]
__global__ __launch_bounds__(LAG_THREADS) void k_lags(const float *__restrict__ x, int C, int T, int D, long long cs, long long ss,
                                                      const double *__restrict__ aff, const double *__restrict__ mu, int lag0, int ncg,
                                                      const double *__restrict__ state, int all_lags, double *__restrict__ partial) {
    if (!all_lags && state[0] != 0.0) return;   // the stop lag lies in an earlier block
    extern __shared__ float lds[];
    const int cg = blockIdx.x, sub = blockIdx.y, m = gridDim.y;
    const int dbase = blockIdx.z * DT;
    const int Dt = min(DT, D - dbase);
    const int s0 = lag0 + sub * LB;
    const int t = threadIdx.x;
    float *A = lds, *B = lds + JT * Dt;
    const int c0 = (int)((long long)cg * C / ncg), c1 = (int)((long long)(cg + 1) * C / ncg);
    const int nit = (LB / RL) * Dt;
    double accd[LAG_ITEMS][RL];
#pragma unroll
    for (int q = 0; q < LAG_ITEMS; ++q)
#pragma unroll
        for (int r = 0; r < RL; ++r) accd[q][r] = 0.0;
    const int rows = 2 * JT + LB;
    for (int c = c0; c < c1; ++c) {
        const float *xc = x + (long long)c * cs;
        for (int j0 = 0; j0 < T - s0; j0 += JT) {
            __syncthreads();
            for (int el = t; el < rows * Dt; el += LAG_THREADS) {
                const int rl = el / Dt, dl = el - rl * Dt, d = dbase + dl;
                const int row = rl < JT ? j0 + rl : j0 + s0 + (rl - JT);
                float y = 0.f;
                if (row < T) y = (float)(tr(xc[(long long)row * ss + d], aff, D, d) - mu[d]);
                lds[el] = y;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < LAG_ITEMS; ++q) {
                const int k = t + q * LAG_THREADS;
                if (k >= nit) continue;
                const int g = k / Dt, d = k - g * Dt;
                const int sg = s0 + g * RL;
                const int jn = min(JT, T - sg - j0);
                if (jn <= 0) continue;
                const float *Ap = A + d, *Bp = B + g * RL * Dt + d;
                float acc[RL], wv[2 * RL];
#pragma unroll
                for (int r = 0; r < RL; ++r) {
                    acc[r] = 0.f;
                    wv[r] = Bp[r * Dt];
                }
                for (int jc = 0; jc < jn; jc += RL) {
                    float a[RL];
#pragma unroll
                    for (int k2 = 0; k2 < RL; ++k2) {
                        a[k2] = Ap[(jc + k2) * Dt];
                        wv[RL + k2] = Bp[(jc + RL + k2) * Dt];
                    }
#pragma unroll
                    for (int k2 = 0; k2 < RL; ++k2)
#pragma unroll
                        for (int r = 0; r < RL; ++r) acc[r] = fmaf(a[k2], wv[k2 + r], acc[r]);
#pragma unroll
                    for (int r = 0; r < RL; ++r) wv[r] = wv[RL + r];
                }
#pragma unroll
                for (int r = 0; r < RL; ++r) accd[q][r] += (double)acc[r];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < LAG_ITEMS; ++q) {
        const int k = t + q * LAG_THREADS;
        if (k >= nit) continue;
        const int g = k / Dt, d = k - g * Dt;
        double *p = partial + ((size_t)cg * m * LB + (size_t)sub * LB + g * RL) * D + dbase + d;
#pragma unroll
        for (int r = 0; r < RL; ++r) p[(size_t)r * D] = accd[q][r];
    }
}

// ---- emcee's integrated autocorrelation time: the normalised autocorrelation function -------------------------------------------
// f(s) = mean_k acf_k(s) / acf_k(0), acf_k(s) = sum_{t < T - s} (x_kt - m_k)(x_k,t+s - m_k) with m_k the walker's OWN mean (emcee 3
// autocorr.integrated_time with has_walkers: include/nnest_hip.h).  Float64 throughout -- the products, the sums and the centred rows
// in LDS: the window of the estimate compares s with 5 tau(s), and a float32 lag sum could move it.  The sum is direct, all lags
// 0 .. T - 1 in blocks of A_LB: O(C D T^2 / 2) float64 FMAs, a few ms at the sizes a bootstrap run has.
//   k_ac_moments   one workgroup per chain: m_k and 1 / acf_k(0) per dimension
//   k_ac_lags      k_lags' tiling with float64 rows: a workgroup owns a group of chains, A_DT dimensions and A_LB lags; a lane owns
//                  (8 consecutive lags, one dimension); per chain the lane's sums are scaled by 1 / acf_k(0) and added to its partial
//   k_lag_reduce   (shared) the partials summed over chain groups in a fixed order
constexpr int A_LB = 128, A_JT = 64, A_DT = 16, A_NCG = 64, A_MMAX = 8;
constexpr int A_THREADS = (A_LB / RL) * A_DT;   // 256
constexpr int A_ROWS = 2 * A_JT + A_LB;

struct AcLayout {
    size_t mom, lag_sums, partial, total;
    AcLayout(int C, int D) {
        const size_t ncg = C < A_NCG ? C : A_NCG;
        size_t o = 0;
        mom = o;      o += (size_t)C * 2 * D;
        lag_sums = o; o += (size_t)A_MMAX * A_LB * D;
        partial = o;  o += ncg * A_MMAX * A_LB * D;
        total = o;
    }
};

__global__ __launch_bounds__(256) void k_ac_moments(const float *__restrict__ x, int T, int D, long long cs, long long ss,
                                                     double *__restrict__ mom) {
    __shared__ double r[256];
    __shared__ double mean[256];
    const int i = blockIdx.x, t = threadIdx.x;
    const float *xc = x + (long long)i * cs;
    double *row = mom + (size_t)i * 2 * D;
    const int Dc = D < 256 ? D : 256;
    const int nsl = 256 / Dc;
    for (int db = 0; db < D; db += Dc) {
        const int d = db + t % Dc, sl = t / Dc;
        const bool live = sl < nsl && d < D;
        for (int pass = 0; pass < 2; ++pass) {
            double a = 0.0;
            if (live) {
                const double m = pass ? mean[t % Dc] : (double)xc[d];   // (pass 0 sums about the first state)
                for (int j = sl; j < T; j += nsl) {
                    const double u = (double)xc[(long long)j * ss + d] - m;
                    a += pass ? u * u : u;
                }
            }
            r[t] = a;
            __syncthreads();
            if (t < Dc && d < D) {
                double b = 0.0;
                for (int k = 0; k < nsl; ++k) b += r[k * Dc + t];
                if (pass == 0) {
                    mean[t] = (double)xc[d] + b / T;
                    row[d] = mean[t];
                } else {
                    row[D + d] = 1.0 / b;
                }
            }
            __syncthreads();
        }
    }
}

// grid (ncg, m, ceil(D / A_DT)); partial [ncg][m * A_LB][D]
__global__ __launch_bounds__(A_THREADS) void k_ac_lags(const float *__restrict__ x, int C, int T, int D, long long cs, long long ss,
                                                       const double *__restrict__ mom, int lag0, int ncg, double *__restrict__ partial) {
    __shared__ double lds[A_ROWS * A_DT];
    const int cg = blockIdx.x, sub = blockIdx.y, m = gridDim.y;
    const int dbase = blockIdx.z * A_DT;
    const int Dt = min(A_DT, D - dbase);
    const int s0 = lag0 + sub * A_LB;
    const int t = threadIdx.x;
    const double *A = lds, *B = lds + A_JT * Dt;
    const int c0 = (int)((long long)cg * C / ncg), c1 = (int)((long long)(cg + 1) * C / ncg);
    const int g = t / Dt, d = t - g * Dt;   // this lane's lags s0 + g RL .. + RL - 1 and dimension dbase + d
    const bool live = t < (A_LB / RL) * Dt;
    const int sg = s0 + g * RL;
    double accd[RL];
#pragma unroll
    for (int r = 0; r < RL; ++r) accd[r] = 0.0;
    for (int c = c0; c < c1; ++c) {
        const float *xc = x + (long long)c * cs;
        const double *mc = mom + (size_t)c * 2 * D;
        double acc[RL];
#pragma unroll
        for (int r = 0; r < RL; ++r) acc[r] = 0.0;
        for (int j0 = 0; j0 < T - s0; j0 += A_JT) {
            __syncthreads();
            for (int el = t; el < A_ROWS * Dt; el += A_THREADS) {
                const int rl = el / Dt, dl = el - rl * Dt, dd = dbase + dl;
                const int row = rl < A_JT ? j0 + rl : j0 + s0 + (rl - A_JT);
                lds[el] = row < T ? (double)xc[(long long)row * ss + dd] - mc[dd] : 0.0;   // zero beyond T: those products drop out
            }
            __syncthreads();
            const int jn = min(A_JT, T - sg - j0);
            if (!live || jn <= 0) continue;
            const double *Ap = A + d, *Bp = B + g * RL * Dt + d;
            double wv[2 * RL];
#pragma unroll
            for (int r = 0; r < RL; ++r) wv[r] = Bp[r * Dt];
            for (int jc = 0; jc < jn; jc += RL) {
                double a[RL];
#pragma unroll
                for (int k2 = 0; k2 < RL; ++k2) {
                    a[k2] = Ap[(jc + k2) * Dt];
                    wv[RL + k2] = Bp[(jc + RL + k2) * Dt];
                }
#pragma unroll
                for (int k2 = 0; k2 < RL; ++k2)
#pragma unroll
                    for (int r = 0; r < RL; ++r) acc[r] = fma(a[k2], wv[k2 + r], acc[r]);
#pragma unroll
                for (int r = 0; r < RL; ++r) wv[r] = wv[RL + r];
            }
        }
        if (live) {
            const double inv0 = mc[D + dbase + d];
#pragma unroll
            for (int r = 0; r < RL; ++r) accd[r] += acc[r] * inv0;
        }
    }
    if (live) {
        double *p = partial + ((size_t)cg * m * A_LB + (size_t)sub * A_LB + g * RL) * D + dbase + d;
#pragma unroll
        for (int r = 0; r < RL; ++r) p[(size_t)r * D] = accd[r];
    }
}

// 64 sums per workgroup; the chain groups in 16 fixed segments, one per wave, the segments added in order
__global__ __launch_bounds__(1024) void k_lag_reduce(const double *__restrict__ partial, int ncg, int n, const double *__restrict__ state,
                                                     int all_lags, double *__restrict__ lag_sums) {
    if (!all_lags && state[0] != 0.0) return;
    __shared__ double r[16][64];
    const int l = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + l;
    double s = 0.0;
    if (k < n) {
        const int a = (int)((long long)seg * ncg / 16), b = (int)((long long)(seg + 1) * ncg / 16);
        for (int cg = a; cg < b; ++cg) s += partial[(size_t)cg * n + k];
    }
    r[seg][l] = s;
    __syncthreads();
    if (seg == 0 && k < n) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += r[q][l];
        lag_sums[k] = t;
    }
}

// one workgroup: p_s for lags lag0 .. lag0 + n - 1, the first lag at which no dimension exceeds 0.05, the ESS sum before it
__global__ __launch_bounds__(1024) void k_advance(const double *__restrict__ lag_sums, const double *__restrict__ sums, int T, int D,
                                                  int lag0, int n, const double *__restrict__ sd, double *__restrict__ e,
                                                  double *__restrict__ state, int all_lags, double *__restrict__ p_out) {
    const bool stopped = state[0] != 0.0;
    if (stopped && !all_lags) return;
    __shared__ int first;
    const int t = threadIdx.x;
    if (t == 0) first = 0x7fffffff;
    __syncthreads();
    const double C = sums[2];
    for (int s = t; s < n; s += 1024) {
        const int lag = lag0 + s;
        const double den = C * (double)(T - lag);
        int any = 0;
        for (int d = 0; d < D; ++d) {
            const double p = lag_sums[(size_t)s * D + d] / den / sd[d];
            if (p_out) p_out[(size_t)(lag - 1) * D + d] = p;
            any |= p > 0.05;
        }
        if (!any) atomicMin(&first, s);
    }
    __syncthreads();
    if (stopped) return;
    const int lim = min(first, n);
    const int w = t >> 6, l = t & 63;
    for (int d = w; d < D; d += 16) {
        double a = 0.0;
        for (int s = l; s < lim; s += 64) {
            const int lag = lag0 + s;
            const double p = lag_sums[(size_t)s * D + d] / (C * (double)(T - lag)) / sd[d];
            if (p > 0.05) a += 2.0 * p * (1.0 - (double)lag / (double)T);
        }
        a = wave_sum(a);
        if (l == 0) e[d] += a;
    }
    if (t == 0 && first < n) state[0] = (double)(lag0 + first);
}

// one workgroup of 256: B sums over the chains AND the dimensions (evaluation.py:88, np.sum without an axis); W, V per dimension
__global__ __launch_bounds__(256) void k_finish(const double *__restrict__ sums, int T, int D, int flags, const double *__restrict__ mu,
                                                const double *__restrict__ center, const double *__restrict__ sd, const double *__restrict__ e, const double *__restrict__ state,
                                                double *__restrict__ out) {
    __shared__ double r[256];
    const int t = threadIdx.x;
    const double C = sums[2];
    double bs = 0.0;
    for (int d = t; d < D; d += 256) {
        const double s1 = sums[3 + d], s2 = sums[3 + D + d];
        // theta_bar - c (s1, s2: sums of theta_i - c and its square)
        const double tb = (flags & NNEST_CHAIN_STATS_RHAT_AT_MEAN) ? mu[d] - center[d] : s1 / C;
        bs += fmax(s2 - 2.0 * tb * s1 + C * tb * tb, 0.0);
    }
    r[t] = bs;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) r[t] += r[t + o];
        __syncthreads();
    }
    const double b = C > 1.0 ? (double)T / (C - 1.0) * r[0] : NAN;
    if (t == 0) {
        out[0] = sums[0] / (C * (T - 1));
        out[1] = sums[1] / (C * (T - 1));
        out[2] = (flags & NNEST_CHAIN_STATS_NO_ESS) ? NAN : (state[0] != 0.0 ? state[0] : (double)T);
        out[3] = C;
    }
    double *o = out + 4;
    for (int d = t; d < D; d += 256) {
        o[d] = (flags & NNEST_CHAIN_STATS_NO_ESS) ? NAN : (double)T / e[d];
        double rhat = NAN;
        if (C > 1.0) {
            const double w = 1.0 / (C * sums[3 + 2 * D + d] + 1e-5);
            const double v = (double)(T - 1) / (double)T * w + (C + 1.0) / (C * T) * b;
            rhat = sqrt(v / w);
        }
        o[D + d] = rhat;
        o[2 * D + d] = mu[d];
        o[3 * D + d] = sd[d];
    }
}

char g_msg[512];
int cs_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    nnest::set_last_error(g_msg);
    return code;
}
#define CS_TRY(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess) return cs_fail(NNEST_E_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

int check_shape(const float *x, int C, int T, int D, long long cs, long long ss, const void *work) {
    if (!x || !work) return cs_fail(NNEST_E_ARG, "chain_stats: NULL x_dev or work_dev");
    if (C < 1 || T < 2 || D < 1) return cs_fail(NNEST_E_ARG, "chain_stats: C=%d T=%d D=%d (C >= 1, T >= 2, D >= 1)", C, T, D);
    if (cs < 0 || ss < 0) return cs_fail(NNEST_E_ARG, "chain_stats: negative stride (chain %lld, step %lld)", cs, ss);
    if (nnest_chain_stats_work_words(C, T, D) < 0) return cs_fail(NNEST_E_ARG, "chain_stats: C=%d D=%d: work exceeds 2^31 words", C, D);
    return NNEST_OK;
}

int lds_bytes(int D) { return (2 * JT + LB) * (D < DT ? D : DT) * (int)sizeof(float); }

}  // namespace

extern "C" {

int nnest_chain_stats_work_words(int C, int T, int D) {
    if (C < 1 || T < 2 || D < 1 || D > (1 << 20)) return -1;
    const size_t w = Layout(C, D).total;
    return w > (size_t)0x7fffffff ? -1 : (int)w;
}

int nnest_chain_stats_chains(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride,
                             const double *affine_dev, const double *center_dev, double *work_dev, double *chain_sums_dev,
                             void *stream) {
    int rc = check_shape(x_dev, C, T, D, chain_stride, step_stride, work_dev);
    if (rc) return rc;
    if (!chain_sums_dev) return cs_fail(NNEST_E_ARG, "chain_stats: NULL chain_sums_dev");
    const Layout L(C, D);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_chain, dim3(C), dim3(256), 0, st, x_dev, T, D, chain_stride, step_stride, affine_dev, work_dev + L.tab);
    CS_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_chain_sum, dim3(D + 1), dim3(256), 0, st, work_dev + L.tab, C, D, center_dev, work_dev + L.center,
                       chain_sums_dev);
    CS_TRY(hipGetLastError());
    return NNEST_OK;
}

int nnest_chain_stats_prepare(const double *chain_sums_dev, int C, int T, int D, const double *mean_dev, const double *std_dev,
                              double *work_dev, void *stream) {
    if (!chain_sums_dev || !work_dev) return cs_fail(NNEST_E_ARG, "chain_stats: NULL chain_sums_dev or work_dev");
    if (nnest_chain_stats_work_words(C, T, D) < 0) return cs_fail(NNEST_E_ARG, "chain_stats: C=%d T=%d D=%d", C, T, D);
    const Layout L(C, D);
    hipLaunchKernelGGL(k_prepare, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, chain_sums_dev, D, mean_dev, std_dev,
                       work_dev + L.center, work_dev + L.mu, work_dev + L.sd, work_dev + L.e, work_dev + L.state);
    CS_TRY(hipGetLastError());
    return NNEST_OK;
}

int nnest_chain_stats_lags(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride,
                           const double *affine_dev, int lag0, int nlags, int flags, double *work_dev, double *lag_sums_dev,
                           void *stream) {
    int rc = check_shape(x_dev, C, T, D, chain_stride, step_stride, work_dev);
    if (rc) return rc;
    if (!lag_sums_dev) return cs_fail(NNEST_E_ARG, "chain_stats: NULL lag_sums_dev");
    if (lag0 < 1 || nlags < 1 || nlags > MMAX * LB || nlags % LB != 0)
        return cs_fail(NNEST_E_ARG, "chain_stats: lags %d + %d (lag0 >= 1, nlags a multiple of %d up to %d)", lag0, nlags, LB, MMAX * LB);
    const Layout L(C, D);
    const int m = nlags / LB;
    const int ncg = (C < NCG ? C : NCG) / m > 0 ? (C < NCG ? C : NCG) / m : 1;
    hipStream_t st = (hipStream_t)stream;
    static bool lds_set[64];   // per device, once
    int dev = 0;
    CS_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !lds_set[dev]) {
        CS_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lags), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes(DT)));
        if (dev >= 0 && dev < 64) lds_set[dev] = true;
    }
    const int all = (flags & NNEST_CHAIN_STATS_ALL_LAGS) ? 1 : 0;
    hipLaunchKernelGGL(k_lags, dim3(ncg, m, (D + DT - 1) / DT), dim3(LAG_THREADS), lds_bytes(D), st, x_dev, C, T, D, chain_stride,
                       step_stride, affine_dev, work_dev + L.mu, lag0, ncg, work_dev + L.state, all, work_dev + L.partial);
    CS_TRY(hipGetLastError());
    const int n = nlags * D;
    hipLaunchKernelGGL(k_lag_reduce, dim3((n + 63) / 64), dim3(1024), 0, st, work_dev + L.partial, ncg, n, work_dev + L.state, all,
                       lag_sums_dev);
    CS_TRY(hipGetLastError());
    return NNEST_OK;
}

int nnest_chain_stats_advance(const double *chain_sums_dev, const double *lag_sums_dev, int C, int T, int D, int lag0, int nlags,
                              int flags, double *work_dev, double *p_dev, void *stream) {
    if (!chain_sums_dev || !lag_sums_dev || !work_dev) return cs_fail(NNEST_E_ARG, "chain_stats: NULL sums or work_dev");
    if (nnest_chain_stats_work_words(C, T, D) < 0) return cs_fail(NNEST_E_ARG, "chain_stats: C=%d T=%d D=%d", C, T, D);
    if (lag0 < 1 || nlags < 1) return cs_fail(NNEST_E_ARG, "chain_stats: lags %d + %d", lag0, nlags);
    const int n = lag0 + nlags - 1 <= T - 1 ? nlags : T - lag0;
    if (n <= 0) return NNEST_OK;
    const Layout L(C, D);
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1024), 0, (hipStream_t)stream, lag_sums_dev, chain_sums_dev, T, D, lag0, n,
                       work_dev + L.sd, work_dev + L.e, work_dev + L.state, (flags & NNEST_CHAIN_STATS_ALL_LAGS) ? 1 : 0, p_dev);
    CS_TRY(hipGetLastError());
    return NNEST_OK;
}

int nnest_chain_stats_finish(const double *chain_sums_dev, int C, int T, int D, int flags, double *work_dev, double *out_dev,
                             void *stream) {
    if (!chain_sums_dev || !work_dev || !out_dev) return cs_fail(NNEST_E_ARG, "chain_stats: NULL sums, work_dev or out_dev");
    if (nnest_chain_stats_work_words(C, T, D) < 0) return cs_fail(NNEST_E_ARG, "chain_stats: C=%d T=%d D=%d", C, T, D);
    const Layout L(C, D);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, chain_sums_dev, T, D, flags, work_dev + L.mu,
                       work_dev + L.center,
                       work_dev + L.sd, work_dev + L.e, work_dev + L.state, out_dev);
    CS_TRY(hipGetLastError());
    return NNEST_OK;
}

int nnest_chain_stats(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride, const double *affine_dev,
                      const double *mean_dev, const double *std_dev, int flags, double *work_dev, double *p_dev, double *out_dev,
                      void *stream) {
    int rc = check_shape(x_dev, C, T, D, chain_stride, step_stride, work_dev);
    if (rc) return rc;
    if (!out_dev) return cs_fail(NNEST_E_ARG, "chain_stats: NULL out_dev");
    if (flags & ~(NNEST_CHAIN_STATS_ALL_LAGS | NNEST_CHAIN_STATS_NO_ESS | NNEST_CHAIN_STATS_RHAT_AT_MEAN))
        return cs_fail(NNEST_E_ARG, "chain_stats: unknown flags 0x%x", flags);
    if ((flags & NNEST_CHAIN_STATS_RHAT_AT_MEAN) && !mean_dev) return cs_fail(NNEST_E_ARG, "chain_stats: RHAT_AT_MEAN without mean_dev");
    const Layout L(C, D);
    double *sums = work_dev + L.sums, *lag_sums = work_dev + L.lag_sums;
    if ((rc = nnest_chain_stats_chains(x_dev, C, T, D, chain_stride, step_stride, affine_dev, mean_dev, work_dev, sums, stream)))
        return rc;
    if ((rc = nnest_chain_stats_prepare(sums, C, T, D, mean_dev, std_dev, work_dev, stream))) return rc;
    if (!(flags & NNEST_CHAIN_STATS_NO_ESS)) {
        // blocks of 1, 1, 2, 4, 8, 8, ... x LB lags; a launch after the stop lag returns at once on the device
        int m = 1, grow = 0;
        for (int lag0 = 1; lag0 <= T - 1;) {
            const int left = (T - 1 - lag0) / LB + 1;
            const int mm = m < left ? m : left;
            if ((rc = nnest_chain_stats_lags(x_dev, C, T, D, chain_stride, step_stride, affine_dev, lag0, mm * LB, flags, work_dev,
                                             lag_sums, stream)))
                return rc;
            if ((rc = nnest_chain_stats_advance(sums, lag_sums, C, T, D, lag0, mm * LB, flags, work_dev, p_dev, stream))) return rc;
            lag0 += mm * LB;
            if (grow++ > 0 && m < MMAX) m *= 2;
        }
    }
    return nnest_chain_stats_finish(sums, C, T, D, flags, work_dev, out_dev, stream);
}

int nnest_chain_autocorr_work_words(int C, int T, int D) {
    if (C < 1 || T < 2 || D < 1 || D > (1 << 20)) return -1;
    const size_t w = AcLayout(C, D).total;
    return w > (size_t)0x7fffffff ? -1 : (int)w;
}

int nnest_chain_autocorr(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride, double *work_dev,
                         double *f_dev, void *stream) {
    if (!x_dev || !work_dev || !f_dev) return cs_fail(NNEST_E_ARG, "chain_autocorr: NULL x_dev, work_dev or f_dev");
    if (C < 1 || T < 2 || D < 1) return cs_fail(NNEST_E_ARG, "chain_autocorr: C=%d T=%d D=%d (C >= 1, T >= 2, D >= 1)", C, T, D);
    if (chain_stride < 0 || step_stride < 0)
        return cs_fail(NNEST_E_ARG, "chain_autocorr: negative stride (chain %lld, step %lld)", chain_stride, step_stride);
    if (nnest_chain_autocorr_work_words(C, T, D) < 0) return cs_fail(NNEST_E_ARG, "chain_autocorr: C=%d D=%d: work exceeds 2^31 words", C, D);
    const AcLayout L(C, D);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ac_moments, dim3(C), dim3(256), 0, st, x_dev, T, D, chain_stride, step_stride, work_dev + L.mom);
    CS_TRY(hipGetLastError());
    const int ncg = C < A_NCG ? C : A_NCG;
    for (int lag0 = 0; lag0 < T; lag0 += A_MMAX * A_LB) {
        const int left = (T - lag0 + A_LB - 1) / A_LB;
        const int m = left < A_MMAX ? left : A_MMAX;
        hipLaunchKernelGGL(k_ac_lags, dim3(ncg, m, (D + A_DT - 1) / A_DT), dim3(A_THREADS), 0, st, x_dev, C, T, D, chain_stride, step_stride,
                           work_dev + L.mom, lag0, ncg, work_dev + L.partial);
        CS_TRY(hipGetLastError());
        const int n = m * A_LB * D;
        hipLaunchKernelGGL(k_lag_reduce, dim3((n + 63) / 64), dim3(1024), 0, st, work_dev + L.partial, ncg, n, work_dev + L.mom, 1,
                           work_dev + L.lag_sums);
        CS_TRY(hipGetLastError());
        const int rows = T - lag0 < m * A_LB ? T - lag0 : m * A_LB;
        CS_TRY(hipMemcpyAsync(f_dev + (size_t)lag0 * D, work_dev + L.lag_sums, (size_t)rows * D * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return NNEST_OK;
}

}  // extern "C"
