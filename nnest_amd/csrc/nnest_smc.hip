// nnest_smc.hip -- the two service kernels of the sequential Monte Carlo sampler (SMCSampler, nnest_amd/smc.py; DESIGN.md 3.12;
// include/nnest_hip.h nnest_smc_reweight, nnest_smc_resample has the definition in full): between two temperatures of the ladder
// L^beta pi the population is REWEIGHTED -- the next beta is the one at which the effective sample size of the incremental weights
// falls to a fraction of N, found by bisection -- and RESAMPLED, systematically, on integer weights.  BUILD-DEFINED: the reference
// has no such sampler.  The moves between are nnest_mcmc_tempered_steps's.
//
// Layout: at these sizes (N <= 2^20 particles) both are service kernels: ONE workgroup of 1024 threads each.  Every sum is float64
// (or int64) and taken in a fixed order -- thread t adds up the elements t, t + 1024, ... in index order, then the 1024 partials go
// through a binary tree in LDS -- with no floating-point atomics: the same call twice returns the same bits.  The bisection's
// decisions are taken on a value every thread reads from the same LDS word, so the workgroup never diverges at a barrier.
//
// Compiled with each float64 operation rounded (fp contract off): the numpy restatement (tests/smc_check.py) follows the same rule.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "nnest_internal.h"

namespace nnest {

enum { NOISE_STREAM_SMC = 8 };
constexpr int SMC_THREADS = 1024;
constexpr int SMC_MAX_N = 1 << 20;

#pragma clang fp contract(off)

// the sum of v over the workgroup, in a fixed order; `red` [SMC_THREADS] in LDS.  Every thread returns the same bits
__device__ __forceinline__ double smc_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();   // (the previous use of `red` is over)
    red[t] = v;
    __syncthreads();
    for (int s = SMC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double smc_block_max(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = SMC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    return red[0];
}

// S1 = sum w, S2 = sum w^2 of w_i = exp(db (logL_i - mx)) over the population
__device__ __forceinline__ void smc_weight_sums(const double *__restrict__ logl, int N, double db, double mx, double *red, double &S1,
                                                double &S2) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < N; i += SMC_THREADS) {
        const double w = exp(db * (logl[i] - mx));
        s1 = s1 + w;
        s2 = s2 + w * w;
    }
    S1 = smc_block_sum(s1, red);
    S2 = smc_block_sum(s2, red);
}

__global__ void __launch_bounds__(SMC_THREADS) smc_reweight_kernel(const double *__restrict__ logl, int N, double beta, double ess_fraction,
                                                                   double *__restrict__ out, long long *__restrict__ m) {
    __shared__ double red[SMC_THREADS];
    double mx = -INFINITY;
    for (int i = threadIdx.x; i < N; i += SMC_THREADS) mx = fmax(mx, logl[i]);
    mx = smc_block_max(mx, red);
    const double target = ess_fraction * (double)N;
    double S1, S2;
    smc_weight_sums(logl, N, 1.0 - beta, mx, red, S1, S2);
    double bn = 1.0;
    if ((S1 * S1) / S2 < target) {
        double lo = beta, hi = 1.0;
        for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (lo + hi);
            smc_weight_sums(logl, N, mid - beta, mx, red, S1, S2);
            if ((S1 * S1) / S2 < target) hi = mid;
            else lo = mid;
        }
        bn = hi > beta ? hi : 1.0;   // (the ladder always advances)
    }
    const double db = bn - beta;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < N; i += SMC_THREADS) {
        const double w = exp(db * (logl[i] - mx));
        s1 = s1 + w;
        s2 = s2 + w * w;
        m[i] = (long long)floor(w * 2147483648.0);
    }
    S1 = smc_block_sum(s1, red);
    S2 = smc_block_sum(s2, red);
    if (threadIdx.x == 0) {
        out[0] = bn;
        out[1] = db * mx + log(S1 / (double)N);
        out[2] = (S1 * S1) / S2;
        out[3] = mx;
    }
}

// the resampling draw of (seed, stage): word 0's top 24 bits of the block (0, stage, 0) of stream NOISE_STREAM_SMC
__host__ __device__ __forceinline__ double smc_uniform(uint64_t seed, uint32_t stage) {
    u32x4 c;
    c.x = 0;
    c.y = stage;
    c.z = 0;
    c.w = (uint32_t)NOISE_STREAM_SMC << 28;
    const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (double)(r.x >> 8) * 5.9604644775390625e-08;
}

// Systematic resampling on the integer weights.  Thread t owns the inputs [t L, (t + 1) L) for the prefix sums and the outputs of
// the same range for the search, L = ceil(N / 1024): cs[t] is the inclusive prefix sum at the end of input chunk t.  An output's
// position p_j grows with j, so a thread finds its first ancestor by bisection over cs and walks forward from there, skipping whole
// chunks of no weight through cs.  A population that cannot be resampled (T <= 0, a negative weight) writes anc[0] = -1 and nothing
// else: the entry reads that word back.
__global__ void __launch_bounds__(SMC_THREADS) smc_resample_kernel(const long long *__restrict__ m, int N, int D, double u,
                                                                   const float *__restrict__ theta_in, const double *__restrict__ logl_in,
                                                                   int *__restrict__ anc, float *__restrict__ theta_out,
                                                                   double *__restrict__ logl_out) {
    __shared__ long long cs[SMC_THREADS];
    __shared__ int bad;
    const int t = threadIdx.x;
    const int L = (N + SMC_THREADS - 1) / SMC_THREADS;
    const int i0 = t * L < N ? t * L : N, i1 = i0 + L < N ? i0 + L : N;
    if (t == 0) bad = 0;
    __syncthreads();
    long long s = 0;
    int neg = 0;
    for (int i = i0; i < i1; ++i) {
        const long long v = m[i];
        neg |= v < 0;
        s += v;
    }
    cs[t] = s;
    if (neg) bad = 1;   // (every writer stores the same value)
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int k = 0; k < SMC_THREADS; ++k) { run += cs[k]; cs[k] = run; }
        if (run <= 0) bad = 1;
    }
    __syncthreads();
    if (bad) {
        if (t == 0) anc[0] = -1;
        return;
    }
    const long long T = cs[SMC_THREADS - 1];
    const int nchunk = (N + L - 1) / L;   // chunks that hold inputs: the others add nothing to cs
    if (i0 < i1) {
        int i = -1;          // the current ancestor, run = the inclusive prefix sum of m at i
        long long run = 0;
        for (int j = i0; j < i1; ++j) {
            // p_j = floor(((j + u) T) / N): every operand exact in float64, each operation rounded
            long long p = (long long)floor((((double)j + u) * (double)T) / (double)N);
            p = p < 0 ? 0 : (p > T - 1 ? T - 1 : p);   // (never taken: (j + u) < N keeps p below T; a guard for the reads below)
            if (i < 0) {     // the thread's first output: the chunk by bisection, the smallest c with cs[c] > p
                int a = 0, b = nchunk - 1;
                while (a < b) {
                    const int c = (a + b) >> 1;
                    if (cs[c] > p) b = c;
                    else a = c + 1;
                }
                i = a * L;
                run = (a ? cs[a - 1] : 0) + m[i];
            }
            while (run <= p && i + 1 < N) {
                ++i;
                if (i % L == 0) {   // a chunk's first input: skip the chunks that end at or below p
                    int c = i / L;
                    while (c + 1 < nchunk && cs[c] <= p) ++c;
                    i = c * L;
                    run = (c ? cs[c - 1] : 0) + m[i];
                } else {
                    run += m[i];
                }
            }
            anc[j] = i;
        }
    }
    __syncthreads();   // (anc is this workgroup's own: visible behind the barrier)
    const long nd = (long)N * D;
    for (long e = t; e < nd; e += SMC_THREADS) {
        const long j = e / D;
        theta_out[e] = theta_in[(long)anc[j] * D + (e - j * D)];
    }
    for (int j = t; j < N; j += SMC_THREADS) logl_out[j] = logl_in[anc[j]];
}
#pragma clang fp contract(fast)

namespace {
char g_smc_msg[512];
int smc_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_smc_msg, sizeof(g_smc_msg), fmt, ap);
    va_end(ap);
    nnest::set_last_error(g_smc_msg);
    return code;
}
}  // namespace

}  // namespace nnest

using namespace nnest;

extern "C" {

// (every check comes before the launch: they answer on a machine without a GPU)
int nnest_smc_reweight(const double *logl_dev, int N, double beta, double ess_fraction, double *out_dev, long long *m_dev, void *stream) {
    if (N < 1 || N > SMC_MAX_N) return smc_fail(NNEST_E_ARG, "smc_reweight: N=%d (1 .. 2^20 particles)", N);
    if (!(ess_fraction > 0.0 && ess_fraction < 1.0)) return smc_fail(NNEST_E_ARG, "smc_reweight: ess_fraction=%g (inside (0, 1))", ess_fraction);
    if (!(beta >= 0.0 && beta < 1.0)) return smc_fail(NNEST_E_ARG, "smc_reweight: beta=%g (0 <= beta < 1: at 1 the ladder has ended)", beta);
    if (!logl_dev || !out_dev || !m_dev) return smc_fail(NNEST_E_ARG, "smc_reweight: NULL logl_dev, out_dev or m_dev");
    hipLaunchKernelGGL(smc_reweight_kernel, dim3(1), dim3(SMC_THREADS), 0, (hipStream_t)stream, logl_dev, N, beta, ess_fraction, out_dev, m_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return smc_fail(NNEST_E_HIP, "smc_reweight_kernel: %s", hipGetErrorString(e));
    return NNEST_OK;
}

int nnest_smc_resample(const long long *m_dev, int N, int D, uint64_t seed, int stage, const float *theta_in_dev, const double *logl_in_dev,
                       int *anc_out_dev, float *theta_out_dev, double *logl_out_dev, void *stream) {
    if (N < 1 || N > SMC_MAX_N || D < 1) return smc_fail(NNEST_E_ARG, "smc_resample: N=%d (1 .. 2^20 particles) D=%d (>= 1)", N, D);
    if (stage < 0) return smc_fail(NNEST_E_ARG, "smc_resample: stage=%d (>= 0)", stage);
    if (!m_dev || !theta_in_dev || !logl_in_dev || !anc_out_dev || !theta_out_dev || !logl_out_dev)
        return smc_fail(NNEST_E_ARG, "smc_resample: NULL device buffer");
    if ((const void *)theta_in_dev == (const void *)theta_out_dev || (const void *)logl_in_dev == (const void *)logl_out_dev)
        return smc_fail(NNEST_E_ARG, "smc_resample: the outputs must not be the inputs (a row is read after others are written)");
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(smc_resample_kernel, dim3(1), dim3(SMC_THREADS), 0, st, m_dev, N, D, smc_uniform(seed, (uint32_t)stage), theta_in_dev,
                       logl_in_dev, anc_out_dev, theta_out_dev, logl_out_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return smc_fail(NNEST_E_HIP, "smc_resample_kernel: %s", hipGetErrorString(e));
    int first = 0;   // (the kernel's verdict on the weights: anc[0] = -1)
    if ((e = hipMemcpyAsync(&first, anc_out_dev, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return smc_fail(NNEST_E_HIP, "smc_resample: %s", hipGetErrorString(e));
    if (first < 0) return smc_fail(NNEST_E_ARG, "smc_resample: the weights sum to 0 or one is negative: nothing to resample (outputs unwritten)");
    return NNEST_OK;
}

}  // extern "C"
