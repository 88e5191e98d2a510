// nnest_glm_psis.hip -- PARETO-SMOOTHED LEAVE-ONE-OUT of the regression likelihoods of user data over a set of posterior draws, and
// the matrix of their terms (include/nnest_hip.h nnest_glm_psis, nnest_glm_terms; glm_psis.h).
//
// PSIS needs, of every data row, the M ~ 3 sqrt(S) largest importance ratios in order, and the [S x n] matrix is never stored.  So
// the draws stream FOUR more times in nnest_glm_pointwise.hip's layout -- a wave owns 16 data rows, the draws come in tiles of 16 through
// v_mfma_f32_16x16x4f32, the accumulator starts from the offsets, tau and j ascend, the grid is over glm_pointwise_groups -- which makes
// eta, and hence l, the bits nnest_glm_pointwise saw, whose b = max -l and cnt the caller hands in:
//   * THREE HISTOGRAM PASSES find the cutoff.  With d = b - (-l) >= 0 and key(d) = the top 24 bits of its pattern, the cutoff is the
//     bin edge c = K << 40 with K the key of the draw of rank M* (from 0) in d: the largest edge with #{d < c} <= M*.  Each pass
//     counts one 8-bit digit of the key, of the draws whose higher digits are the prefix found so far, in a per-wave LDS histogram
//     [16 rows][256] uint32 (16 KB a wave, 64 KB a workgroup: the static limit), flushed with integer atomics into hist [n, 256];
//     a one-thread-per-row kernel then picks the digit and zeroes the row's counts for the next pass.  Counts are integers: the
//     order of the atomics does not reach the result.
//   * THE COLLECT PASS writes d < c into the row's tail buffer [n, Mcap] (slots from a per-row integer counter; a slot >= Mcap is
//     dropped and flagged, never written) and adds the body's N, B = sum e^-d, B2 = sum e^-2d per lane, merged over the 16 lanes of a
//     row by a butterfly of additions (commutative: both sides hold the same bits) into per-group partials.
//   * THE FIT KERNEL, one workgroup per data row, merges the partials in index order, sorts the tail in LDS (bitonic; behind it the
//     array is a function of the multiset alone, whatever order the slots were handed out in), writes it back, and computes Zhang &
//     Stephens' fit, the smoothed sums, elpd_psis and psis_ess in float64 in a fixed order.
//   * nnest_glm_terms is the same loop with a store for an epilogue.
// Rows i >= n are masked (never written), no read goes past [D, ld], no floating-point atomics: the same call twice returns the same bits.
#include <type_traits>

#include "glm_psis.h"

namespace nnest {

#pragma clang fp contract(off)

// the wave's draw loop (glm_pointwise_kernel's, to the operation): f(v, counted, l) for the pair (row 16 rb + 4 g + v, draw 16 tl + m)
template <int NT, int FAM, class F>
__device__ __forceinline__ void psis_stream(const GlmSpec &gl, const float *__restrict__ t, int S, int G, int chunk, int rb, int m, int g, F &&f) {
    const int D = gl.D;
    const int i0 = 16 * rb + 4 * g;
    float a[NT][8];
    pw_load_a<NT>(gl, rb, m, g, a);
    const f32x4 off = *reinterpret_cast<const f32x4 *>(gl.o + i0);
    const f32x4 yv = *reinterpret_cast<const f32x4 *>(gl.y + i0);
    const int ntiles = (S + GLMPW_TILE - 1) / GLMPW_TILE;
    float b[NT][8];
    if (chunk < ntiles) pw_load_tile<NT>(t, (long)GLMPW_TILE * chunk + m, S, D, g, b);
    for (int tl = chunk; tl < ntiles; tl += G) {   // (uniform)
        const long s = (long)GLMPW_TILE * tl + m;
        float bn[NT][8];
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
        for (int v = 0; v < 4; ++v) f(v, s, in, glm_term<FAM>(eta[v], yy[v]));
#pragma unroll
        for (int tau = 0; tau < NT; ++tau)
#pragma unroll
            for (int j = 0; j < 8; ++j) b[tau][j] = bn[tau][j];
    }
}

__device__ __forceinline__ bool psis_live(double l) { return fabs(l) <= 1.79769313486231570e308; }
__device__ __forceinline__ unsigned psis_key(double d) { return (unsigned)((unsigned long long)__double_as_longlong(d) >> GLMPSIS_KEY_SHIFT); }

// ---- the matrix of terms: out [S, n], NaN for a dead pair ----
template <int NT, int FAM>
__global__ void __launch_bounds__(256) glm_terms_kernel(GlmSpec gl, const float *__restrict__ t, double *__restrict__ out, int S, int G) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4, n = gl.n;
    const int rb = 4 * blockIdx.x + wave;
    if (16 * rb >= n) return;   // (uniform in the wave; no barrier follows)
    const int i0 = 16 * rb + 4 * g;
    psis_stream<NT, FAM>(gl, t, S, G, blockIdx.y, rb, m, g, [&](int v, long s, bool in, double l) {
        if (in && i0 + v < n) out[(size_t)s * n + (i0 + v)] = psis_live(l) ? l : __builtin_nan("");   // (masked, not padded)
    });
}

// ---- one digit of the key: pass 0, 1, 2 = bits 23-16, 15-8, 7-0 ----
template <int NT, int FAM>
__global__ void __launch_bounds__(256) glm_psis_hist_kernel(GlmSpec gl, const float *__restrict__ t, const double *__restrict__ stats,
                                                            const unsigned *__restrict__ sel, unsigned *__restrict__ hist, int S, int G, int pass) {
    __shared__ unsigned h[4][16 * 256];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4, n = gl.n;
    for (int k = threadIdx.x; k < 4 * 16 * 256; k += 256) (&h[0][0])[k] = 0u;
    __syncthreads();
    const int rb = 4 * blockIdx.x + wave;
    const bool active = 16 * rb < n;   // (uniform in the wave)
    if (active) {
        const int i0 = 16 * rb + 4 * g;
        double b[4];
        unsigned pre[4];
        bool row[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            row[v] = i0 + v < n;
            b[v] = row[v] ? stats[(size_t)(i0 + v) * 8 + 2] : 0.0;
            pre[v] = row[v] && pass > 0 ? sel[2 * (size_t)(i0 + v)] : 0u;
        }
        const int shift = 16 - 8 * pass;
        unsigned *hw = h[wave];
        psis_stream<NT, FAM>(gl, t, S, G, blockIdx.y, rb, m, g, [&](int v, long s, bool in, double l) {
            if (!(in && row[v] && psis_live(l))) return;
            const unsigned key = psis_key(b[v] - (-l));
            if (pass > 0 && (key >> (shift + 8)) != pre[v]) return;
            atomicAdd(&hw[(4 * g + v) * 256 + ((key >> shift) & 255u)], 1u);
        });
    }
    __syncthreads();
    if (active) {
        const unsigned *hw = h[wave];
        for (int k = lane; k < 16 * 256; k += 64) {
            const unsigned c = hw[k];
            const int i = 16 * rb + (k >> 8);
            if (c != 0u && i < n) atomicAdd(&hist[(size_t)i * 256 + (k & 255)], c);
        }
    }
}

// one thread per row: the digit at which the count of d below the edge would pass M*; the row's counts are zeroed for the next pass
__global__ void __launch_bounds__(256) glm_psis_select_kernel(const double *__restrict__ stats, unsigned *__restrict__ hist,
                                                              unsigned *__restrict__ sel, int n, int pass) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long cnt = (long long)stats[(size_t)i * 8 + 5];
    const long long target = psis_tail_target(cnt);
    const unsigned prefix = pass > 0 ? sel[2 * (size_t)i] : 0u, below = pass > 0 ? sel[2 * (size_t)i + 1] : 0u;
    unsigned *h = hist + (size_t)i * 256;
    unsigned dg = 0u, lo = 0u, cum = 0u;
    bool found = false;
    for (int k = 0; k < 256; ++k) {
        const unsigned c = h[k];
        h[k] = 0u;
        if (!found && (long long)below + cum + c > target) {
            found = true;
            dg = (unsigned)k;
            lo = cum;
        }
        cum += c;
    }
    // (no live draw: the edge 0 and nothing below it)
    sel[2 * (size_t)i] = cnt > 0 && found ? (prefix << 8) | dg : 0u;
    sel[2 * (size_t)i + 1] = cnt > 0 && found ? below + lo : 0u;
}

// ---- the tail into its buffer, the body into sums ----
template <int NT, int FAM>
__global__ void __launch_bounds__(256) glm_psis_collect_kernel(GlmSpec gl, const float *__restrict__ t, const double *__restrict__ stats,
                                                               const unsigned *__restrict__ sel, unsigned *__restrict__ counter,
                                                               double *__restrict__ tail, double *__restrict__ partials, int S, int G, int mcap) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4, n = gl.n;
    const int rb = 4 * blockIdx.x + wave, chunk = blockIdx.y;
    if (16 * rb >= n) return;   // (uniform in the wave; no barrier follows)
    const int i0 = 16 * rb + 4 * g;
    double b[4], nb[4], B[4], B2[4];
    unsigned K[4];
    bool row[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        row[v] = i0 + v < n;
        b[v] = row[v] ? stats[(size_t)(i0 + v) * 8 + 2] : 0.0;
        K[v] = row[v] ? sel[2 * (size_t)(i0 + v)] : 0u;
        nb[v] = B[v] = B2[v] = 0.0;
    }
    psis_stream<NT, FAM>(gl, t, S, G, chunk, rb, m, g, [&](int v, long s, bool in, double l) {
        if (!(in && row[v] && psis_live(l))) return;
        const double d = b[v] - (-l);
        if (psis_key(d) < K[v]) {
            const unsigned slot = atomicAdd(&counter[i0 + v], 1u);
            if (slot < (unsigned)mcap) tail[(size_t)(i0 + v) * mcap + slot] = d;   // (a slot past the row's buffer is dropped)
        } else {
            const double e = exp(-d);
            nb[v] += 1.0;
            B[v] += e;
            B2[v] += e * e;
        }
    });
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int k = 1; k < 16; k <<= 1) {
            nb[v] += __shfl_xor(nb[v], k);
            B[v] += __shfl_xor(B[v], k);
            B2[v] += __shfl_xor(B2[v], k);
        }
    if (m == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (row[v]) {
                double *p = partials + ((size_t)chunk * n + (i0 + v)) * 3;
                p[0] = nb[v];
                p[1] = B[v];
                p[2] = B2[v];
            }
    }
}

// ---- the fit: one workgroup per data row ----
// the sum of v over the 256 threads, the same bits in every thread: a butterfly in the wave, the four waves in order
__device__ __forceinline__ double psis_block_sum(double v, double *red, int lane, int wave) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k);
    __syncthreads();   // (the last sum has been read)
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256) glm_psis_fit_kernel(const double *__restrict__ stats, const unsigned *__restrict__ sel,
                                                           const unsigned *__restrict__ counter, double *__restrict__ tail,
                                                           const double *__restrict__ partials, double *__restrict__ out, int n, int G, int mcap) {
    __shared__ double dd[GLMPSIS_SORT];
    __shared__ double xs[GLMPSIS_SORT * 3 / 4];
    __shared__ double red[4];
    __shared__ double th[96], Lj[96], tw[96];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x;
    if (i >= n) return;   // (uniform in the workgroup)
    const double b = stats[(size_t)i * 8 + 2], cnt = stats[(size_t)i * 8 + 5];
    const unsigned K = sel[2 * (size_t)i], got = counter[i];
    const int M = (int)(got < (unsigned)mcap ? got : (unsigned)mcap);
    int flag = got > (unsigned)mcap ? GLMPSIS_F_DROPPED : 0;
    const double c = __longlong_as_double((long long)((unsigned long long)K << GLMPSIS_KEY_SHIFT));
    // the body: the groups' partials in index order (every thread the same loads, the same bits)
    double nb = 0.0, B = 0.0, B2 = 0.0;
    for (int q = 0; q < G; ++q) {
        const double *p = partials + ((size_t)q * n + i) * 3;
        nb += p[0];
        B += p[1];
        B2 += p[2];
    }
    // the tail, sorted ascending in d (padded with +inf to a power of two)
    double *row = tail + (size_t)i * mcap;
    int P = 1;
    while (P < M) P <<= 1;
    for (int a = tid; a < P; a += 256) dd[a] = a < M ? row[a] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int a = tid; a < P; a += 256) {
                const int l = a ^ j;
                if (l > a) {
                    const double p = dd[a], q = dd[l];
                    if ((p > q) == ((a & k) == 0)) {
                        dd[a] = q;
                        dd[l] = p;
                    }
                }
            }
            __syncthreads();
        }
    for (int a = tid; a < M; a += 256) row[a] = dd[a];
    const double u = exp(-c);
    for (int a = tid; a < M; a += 256) xs[a] = exp(-dd[a]) - u;   // (x_(j) = xs[M - j]: ascending in j)
    __syncthreads();

    const double Md = (double)M;
    double sigma = __builtin_nan(""), khat = INFINITY, thetahat = __builtin_nan("");
    bool fit = false;
    if (M >= 5) {   // (uniform)
        int sq = (int)sqrt(Md);
        while (sq * sq > M) --sq;
        while ((sq + 1) * (sq + 1) <= M) ++sq;
        const int mg = 30 + sq;
        const double xM = xs[0], xstar = xs[M - (int)floor(Md / 4.0 + 0.5)];
        for (int j = 1; j <= mg; ++j) {
            const double theta = 1.0 / xM + (1.0 - sqrt((double)mg / ((double)j - 0.5))) / (3.0 * xstar);
            double s = 0.0;
            for (int a = tid; a < M; a += 256) s += log1p(-theta * xs[a]);
            const double kj = psis_block_sum(s, red, lane, wave) / Md;
            if (tid == 0) {
                th[j - 1] = theta;
                Lj[j - 1] = Md * (log(-theta / kj) - kj - 1.0);
            }
        }
        __syncthreads();
        if (tid < mg) {
            double s = 0.0;
            for (int q = 0; q < mg; ++q) s += exp(Lj[q] - Lj[tid]);
            tw[tid] = th[tid] * (1.0 / s);   // (an overflow to +inf: the weight 0)
        }
        __syncthreads();
        thetahat = 0.0;
        for (int q = 0; q < mg; ++q) thetahat += tw[q];
        double s = 0.0;
        for (int a = tid; a < M; a += 256) s += log1p(-thetahat * xs[a]);
        const double k = psis_block_sum(s, red, lane, wave) / Md;
        if (psis_live(k)) {
            fit = true;
            sigma = -k / thetahat;
            khat = (k * Md + 5.0) / (Md + 10.0);
        } else {
            khat = __builtin_nan("");
            flag |= GLMPSIS_F_BADK;
        }
    } else {
        flag |= GLMPSIS_F_NOFIT;
    }
    // the smoothed tail: q_j for x_(j), j = M - a, against e^(d_(j)); without a fit the raw weights e^-d
    double sq1 = 0.0, sq2 = 0.0, sqe = 0.0;
    for (int a = tid; a < M; a += 256) {
        double q;
        if (fit) {
            const double lp = log1p(-(((double)(M - a) - 0.5) / Md));
            const double tailq = fabs(khat) < 9.094947017729282e-13 ? -sigma * lp : sigma * expm1(-khat * lp) / khat;   // (2^-40)
            q = u + tailq;
            q = q > 1.0 ? 1.0 : q;
            sqe += q * exp(dd[a]);
        } else {
            q = exp(-dd[a]);
        }
        sq1 += q;
        sq2 += q * q;
    }
    sq1 = psis_block_sum(sq1, red, lane, wave);
    sq2 = psis_block_sum(sq2, red, lane, wave);
    sqe = psis_block_sum(sqe, red, lane, wave);
    if (tid == 0) {
        const double num = fit ? nb + sqe : nb + Md, den = B + sq1, den2 = B2 + sq2;
        const double lognum = log(num), logden = log(den);
        double *o = out + (size_t)i * GLMPSIS_SLOTS;
        o[0] = c;
        o[1] = Md;
        o[2] = nb;
        o[3] = B;
        o[4] = B2;
        o[5] = sigma;
        o[6] = khat;
        o[7] = lognum;
        o[8] = logden;
        o[9] = cnt > 0.0 ? (-b + lognum) - logden : __builtin_nan("");
        o[10] = den2 > 0.0 ? den * den / den2 : 0.0;
        o[11] = (double)flag;
        o[12] = (double)psis_tail_target((long long)cnt);
        o[13] = thetahat;
        o[14] = 0.0;
        o[15] = 0.0;
    }
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------
// host side
template <class F>
static hipError_t psis_dispatch(const GlmSpec &gl, F &&f) {
    const int key = 2 * ((gl.D + 31) / 32) + gl.family;   // (NT: the lane's 8 NT columns, 32 NT >= D)
#define NNEST_PSIS_CASE(NT, FAM) \
    case 2 * NT + FAM: f(std::integral_constant<int, NT>{}, std::integral_constant<int, FAM>{}); return hipGetLastError();
    switch (key) {
        NNEST_PSIS_CASE(1, GLM_LOGISTIC) NNEST_PSIS_CASE(1, GLM_POISSON) NNEST_PSIS_CASE(2, GLM_LOGISTIC) NNEST_PSIS_CASE(2, GLM_POISSON)
        NNEST_PSIS_CASE(3, GLM_LOGISTIC) NNEST_PSIS_CASE(3, GLM_POISSON) NNEST_PSIS_CASE(4, GLM_LOGISTIC) NNEST_PSIS_CASE(4, GLM_POISSON)
    }
#undef NNEST_PSIS_CASE
    return hipErrorInvalidConfiguration;
}

hipError_t launch_glm_terms(const GlmSpec &gl, const float *t, double *out, int S, hipStream_t st) {
    const int G = glm_pointwise_groups(S, gl.n);
    if (G <= 0) return hipSuccess;
    if (gl.family != GLM_LOGISTIC && gl.family != GLM_POISSON) return hipErrorInvalidConfiguration;
    const dim3 grid((gl.n + 63) / 64, G);
    return psis_dispatch(gl, [&](auto nt, auto fam) {
        hipLaunchKernelGGL((glm_terms_kernel<decltype(nt)::value, decltype(fam)::value>), grid, dim3(256), 0, st, gl, t, out, S, G);
    });
}

hipError_t launch_glm_psis(const GlmSpec &gl, const float *t, const double *stats, double *out, void *work, int S, hipStream_t st) {
    if (gl.family != GLM_LOGISTIC && gl.family != GLM_POISSON) return hipErrorInvalidConfiguration;
    const int n = gl.n;
    const GlmPsisWork w = glm_psis_work(S, n);
    char *base = static_cast<char *>(work);
    double *tail = reinterpret_cast<double *>(base + w.tail), *partials = reinterpret_cast<double *>(base + w.partials);
    unsigned *hist = reinterpret_cast<unsigned *>(base + w.hist), *sel = reinterpret_cast<unsigned *>(base + w.sel);
    unsigned *counter = reinterpret_cast<unsigned *>(base + w.counter);
    hipError_t e = hipMemsetAsync(base + w.hist, 0, (size_t)(w.bytes - w.hist), st);   // (the counts, the prefixes and the slot counters)
    if (e != hipSuccess) return e;
    const int G = w.G;
    if (G > 0) {
        const dim3 grid((n + 63) / 64, G), rows((n + 255) / 256);
        for (int pass = 0; pass < 3; ++pass) {
            e = psis_dispatch(gl, [&](auto nt, auto fam) {
                hipLaunchKernelGGL((glm_psis_hist_kernel<decltype(nt)::value, decltype(fam)::value>), grid, dim3(256), 0, st, gl, t, stats, sel,
                                   hist, S, G, pass);
            });
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(glm_psis_select_kernel, rows, dim3(256), 0, st, stats, hist, sel, n, pass);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        e = psis_dispatch(gl, [&](auto nt, auto fam) {
            hipLaunchKernelGGL((glm_psis_collect_kernel<decltype(nt)::value, decltype(fam)::value>), grid, dim3(256), 0, st, gl, t, stats, sel,
                               counter, tail, partials, S, G, w.mcap);
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(glm_psis_fit_kernel, dim3(n), dim3(256), 0, st, stats, sel, counter, tail, partials, out, n, G, w.mcap);
    return hipGetLastError();
}

}  // namespace nnest
