// nnest_glm_newton.hip -- GRADIENT, CURVATURE AND NEWTON STEP of the regression likelihoods of user data at one theta (include/nnest_hip.h
// nnest_glm_curv, nnest_glm_newton_solve; glm_newton.h): what a posterior mode, the Laplace approximation and the
// Laplace evidence are made of.  All float64.
//
// THE CURVATURE is a reduction over the n data rows of D + D (D + 1) / 2 sums, H = sum over row blocks of (A_blk^T W)(A_blk), on the
// float64 matrix cores (v_mfma_f64_16x16x4_f64; C/D: col = lane & 15, row = (lane >> 4) + 4 reg; A/B as the f32 16x16x4 form).
//   * A workgroup of four waves takes the row blocks b = group, group + G, ... of 64 rows.  Per block:
//     1. thread (wave p, lane) reads row 64 b + lane of the columns c = p, p + 4, ... from at (the 64 lanes one 256-byte run),
//        stores the float32 value into LDS (0 for a row i >= n: masked, not padded) and adds it into its quarter of eta by fma;
//     2. behind a barrier wave 0 adds o_i and the four quarters in wave order, evaluates l_i, y_i - mu_i and w_i for its lane's row
//        (glm_curv_row) and leaves the residuals and the weights in LDS (0 for a masked row), the term in its running sum;
//     3. behind a barrier every wave walks the block in K-steps of four rows: lane (m, k) reads A[r0 + k, 16 t + m] for the NT
//        column tiles t (bank 4 m + k: no conflict), scales by w, and issues the MFMAs of ITS tiles -- CurvTiles: the tiles on and
//        above the diagonal and the NT gradient tiles (operand r_k in lane m = 0, zero elsewhere: row 0 of the result is the
//        gradient's 16 columns) dealt round robin to the waves, all indices compile-time (one copy of the loop per wave).
//   * After its last block the wave writes its tiles' entries (row <= col < D) into the group's partials; a second kernel, one
//     thread per entry of [1 + D + D D], adds the G partials in index order, applies the safe rule to entry 0 and writes both
//     triangles from the one sum.  No atomics of any kind: the same call twice gives the same bits.
// No read goes past [D, ld] (64 (b + 1) <= ld for every block started; a column past D - 1 reads column D - 1 and is zeroed behind
// the load, so the loads carry no branch and a block's are all in flight together -- the next block's behind this block's MFMAs).
//
// THE SOLVE runs in one workgroup of 128 threads with the matrix in dynamic LDS (D (D + 1) + 3 D doubles: 132 KB at D = 128, the
// limit raised as the other large-LDS kernels do): the prior's terms, a left-looking Cholesky -- thread i owns row i, column j is
// the dot products of rows i >= j with row j (four chains k mod 4 over the multiples of eight, added pairwise, then the rest in the
// order of k), the pivot through one LDS slot, two barriers a column; a pivot that
// is not above (j + 2) 2^-52 H_jj, the bound on its own rounding error, cannot be told from one <= 0 and is refused with it --, the two
// triangular solves (one barrier a step), and thread 0's sums for the decrement, log det and log pi, each in index order.
#include "glm_newton.h"

namespace nnest {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the MFMAs of wave W's tiles J, J + 1, ... for one K-step: a[t] the lane's value of column tile t, wa[t] that times the row's weight,
// ra the row's residual in the lanes m = 0
template <int NT, int W, int J>
__device__ __forceinline__ void curv_step(const double (&a)[NT], const double (&wa)[NT], double ra, f64x4 (&acc)[CurvTiles<NT>::PER]) {
    using T = CurvTiles<NT>;
    constexpr int q = W + 4 * J;
    if constexpr (q < T::NQ) {
        if constexpr (q < T::NH) {
            constexpr int R = T::tr(q), C = T::tc(q);   // (constants: a call in the index would be evaluated at run time)
            acc[J] = mfma_f64(wa[R], a[C], acc[J]);
        } else {
            acc[J] = mfma_f64(ra, a[q - T::NH], acc[J]);
        }
        curv_step<NT, W, J + 1>(a, wa, ra, acc);
    }
}

// the 16 K-steps of one staged block, for wave W
template <int NT, int W>
__device__ __forceinline__ void curv_block(const float (*As)[GLMNW_STRIDE], const double *ws, const double *rs, int lane,
                                           f64x4 (&acc)[CurvTiles<NT>::PER]) {
    const int m = lane & 15, k = lane >> 4;
    const float *Ap = &As[m][k];   // A[r0 + k, 16 t + m] is Ap[16 t GLMNW_STRIDE + r0]
    float af[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) af[t] = Ap[16 * t * GLMNW_STRIDE];
    double wk = ws[k], rk = rs[k];
    for (int r0 = 0; r0 < GLMNW_ROWS; r0 += 4) {
        // the next step's operands in front of this step's MFMAs (past the last step: the first one's again, dropped)
        const int rn = (r0 + 4) & (GLMNW_ROWS - 1);
        float afn[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) afn[t] = Ap[16 * t * GLMNW_STRIDE + rn];
        const double wkn = ws[rn + k], rkn = rs[rn + k];
        double a[NT], wa[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            a[t] = (double)af[t];
            wa[t] = wk * a[t];
        }
        curv_step<NT, W, 0>(a, wa, m == 0 ? rk : 0.0, acc);
#pragma unroll
        for (int t = 0; t < NT; ++t) af[t] = afn[t];
        wk = wkn;
        rk = rkn;
    }
}

// the entries of wave W's tiles J, J + 1, ... into the group's partials P
template <int NT, int W, int J>
__device__ __forceinline__ void curv_store(double *P, int D, int lane, const f64x4 (&acc)[CurvTiles<NT>::PER]) {
    using T = CurvTiles<NT>;
    constexpr int q = W + 4 * J;
    if constexpr (q < T::NQ) {
        const int col = lane & 15;
        if constexpr (q < T::NH) {
            constexpr int TR = T::tr(q), TC = T::tc(q);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int R = 16 * TR + (lane >> 4) + 4 * v, C = 16 * TC + col;
                if (R <= C && C < D) P[glm_curv_packed(D, R, C)] = acc[J][v];
            }
        } else {
            const int C = 16 * (q - T::NH) + col;
            if (lane < 16 && C < D) P[1 + C] = acc[J][0];   // (row 0 of the tile: lanes 0 .. 15, register 0)
        }
        curv_store<NT, W, J + 1>(P, D, lane, acc);
    }
}

template <int NT, int FAM>
__global__ void __launch_bounds__(256) glm_curv_kernel(GlmSpec gl, const double *__restrict__ theta, double *__restrict__ partials, int G) {
    using T = CurvTiles<NT>;
    __shared__ float As[16 * NT][GLMNW_STRIDE];
    __shared__ double etap[4][GLMNW_ROWS];
    __shared__ double ws[GLMNW_ROWS], rs[GLMNW_ROWS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = gl.D, n = gl.n;
    const size_t ld = (size_t)gl.ld;
    __shared__ double ths[16 * NT];
    constexpr int CW = 4 * NT;   // columns a wave stages of a block: c = wave + 4 q
    if (threadIdx.x < 16 * NT) ths[threadIdx.x] = (int)threadIdx.x < D ? theta[threadIdx.x] : 0.0;   // (0 past D - 1: x + 0 a = x)
    f64x4 acc[T::PER];
#pragma unroll
    for (int j = 0; j < T::PER; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double lsum = 0.0;
    const int nblk = (n + GLMNW_ROWS - 1) / GLMNW_ROWS;   // (64 nblk <= ld: no read past the arrays)
    // The loads carry no branch (a column past D - 1 reads column D - 1 and is zeroed behind the load): all CW of them are in flight
    // together, and the NEXT block's are issued before this block's MFMAs, which hide them
    float v[CW];
    {
        const float *p = gl.at + GLMNW_ROWS * blockIdx.x + lane;   // (G <= nblk: every group has a first block)
#pragma unroll
        for (int q = 0; q < CW; ++q) v[q] = p[(size_t)min(wave + 4 * q, D - 1) * ld];
    }
    __syncthreads();   // (ths)
    for (int b = blockIdx.x; b < nblk; b += G) {          // (uniform in the workgroup)
        const int i = GLMNW_ROWS * b + lane;
        const bool live = i < n;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            const int c = wave + 4 * q;
            const float vm = live && c < D ? v[q] : 0.f;   // (masked, not padded)
            As[c][lane] = vm;
            s = fma((double)vm, ths[c], s);
        }
        etap[wave][lane] = s;
        __syncthreads();
        if (wave == 0) {
            const double eta = ((((double)gl.o[i] + etap[0][lane]) + etap[1][lane]) + etap[2][lane]) + etap[3][lane];
            double l, r, w;
            glm_curv_row<FAM>(eta, (double)gl.y[i], l, r, w);
            lsum += live ? l : 0.0;
            ws[lane] = live ? w : 0.0;
            rs[lane] = live ? r : 0.0;
        }
        __syncthreads();
        if (b + G < nblk) {   // (uniform)
            const float *p = gl.at + GLMNW_ROWS * (b + G) + lane;
#pragma unroll
            for (int q = 0; q < CW; ++q) v[q] = p[(size_t)min(wave + 4 * q, D - 1) * ld];
        }
        switch (wave) {
            case 0: curv_block<NT, 0>(As, ws, rs, lane, acc); break;
            case 1: curv_block<NT, 1>(As, ws, rs, lane, acc); break;
            case 2: curv_block<NT, 2>(As, ws, rs, lane, acc); break;
            default: curv_block<NT, 3>(As, ws, rs, lane, acc); break;
        }
        __syncthreads();   // (the block is free for the next one)
    }
    double *P = partials + (size_t)blockIdx.x * glm_curv_slots(D);
    if (wave == 0) {
        lsum += __shfl_xor(lsum, 1);
        lsum += __shfl_xor(lsum, 2);
        lsum += __shfl_xor(lsum, 4);
        lsum += __shfl_xor(lsum, 8);
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        if (lane == 0) P[0] = lsum;
    }
    switch (wave) {
        case 0: curv_store<NT, 0, 0>(P, D, lane, acc); break;
        case 1: curv_store<NT, 1, 0>(P, D, lane, acc); break;
        case 2: curv_store<NT, 2, 0>(P, D, lane, acc); break;
        default: curv_store<NT, 3, 0>(P, D, lane, acc); break;
    }
}

// the second stage: one thread per entry of out [1 + D + D D] adds the G partials in index order; a thread on or above the
// diagonal writes both triangles
__global__ void __launch_bounds__(256) glm_curv_merge_kernel(const double *__restrict__ partials, double *__restrict__ out, double logl0, int D, int G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 1 + D + D * D) return;
    int slot = e, R = 0, C = 0;
    if (e >= 1 + D) {
        R = (e - 1 - D) / D;
        C = (e - 1 - D) % D;
        if (R > C) return;
        slot = glm_curv_packed(D, R, C);
    }
    const size_t stride = (size_t)glm_curv_slots(D);
    double s = 0.0;
    const double *p = partials + slot;
    int g = 0;
    for (; g + 8 <= G; g += 8) {   // (eight loads in flight; the additions in index order)
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = p[(size_t)(g + j) * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += t[j];
    }
    for (; g < G; ++g) s += p[(size_t)g * stride];
    if (e == 0) out[0] = glm_finish(logl0, s);
    else if (e < 1 + D) out[e] = s;
    else {
        out[1 + D + R * D + C] = s;
        out[1 + D + C * D + R] = s;
    }
}

#pragma clang fp contract(off)
__global__ void __launch_bounds__(GLMNW_SOLVE_THREADS) glm_newton_solve_kernel(const double *__restrict__ curv, GaussPriorSpec pr, int has_prior,
                                                                               const double *__restrict__ theta, double *__restrict__ step,
                                                                               double *__restrict__ chol, double *__restrict__ info, int D) {
    extern __shared__ double sm[];
    const int S = D + 1, t = threadIdx.x;
    double *L = sm;                    // [D][D + 1]: the negative Hessian of the log posterior, then its lower factor
    double *ys = sm + (size_t)D * S;   // [D]: the squares of the prior's u, then y of L y = g
    double *dl = ys + D;               // [D]: delta
    double *gs = dl + D;               // [D]: g
    __shared__ double pivot_s, floor_s, logpi_s;
    // (thread t takes column t, sixteen rows' loads in flight; a row past D - 1 reads row D - 1 and is dropped)
    for (int r0 = 0; r0 < D; r0 += 16) {
        double h[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) h[q] = curv[1 + D + min(r0 + q, D - 1) * D + min(t, D - 1)];
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (r0 + q < D && t < D) L[(r0 + q) * S + t] = h[q];
    }
    double r2 = 0.0;
    if (t < D) {
        double g = curv[1 + t], u = 0.0;
        if (has_prior) {
            const double r = (double)pr.r[t], d = theta[t] - (double)pr.m[t];
            u = d * r;
            r2 = r * r;
            g = g - d * r2;
        }
        gs[t] = g;
        ys[t] = u * u;
    }
    __syncthreads();
    if (t < D) L[t * S + t] = L[t * S + t] + r2;
    if (t == 0) {
        double ss = 0.0;
        for (int c = 0; c < D; ++c) ss += ys[c];
        logpi_s = has_prior ? gauss_prior_finish(pr.logc, ss) : 0.0;
    }
    __syncthreads();
    const double logl = curv[0], logpi = logpi_s;
    int status = (logl == -1e100 || !(fabs(logpi) <= 1.79769313486231570e308)) ? 2 : 0;
    double b = 0.0;
    if (status == 0) {
        for (int j = 0; j < D; ++j) {   // (every branch on j, status or the pivot is uniform in the workgroup)
            double s = 0.0;
            if (t >= j && t < D) {
                s = L[t * S + j];
                const double *rt = L + t * S, *rj = L + j * S;
                int k = 0;
                double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;   // (four chains: k mod 4; one chain of j dependent fmas is the kernel's time)
                for (; k + 8 <= j; k += 8) {   // (sixteen reads in flight)
                    double a[8], c[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        a[q] = rt[k + q];
                        c[q] = rj[k + q];
                    }
                    p0 = fma(a[0], c[0], p0); p1 = fma(a[1], c[1], p1); p2 = fma(a[2], c[2], p2); p3 = fma(a[3], c[3], p3);
                    p0 = fma(a[4], c[4], p0); p1 = fma(a[5], c[5], p1); p2 = fma(a[6], c[6], p2); p3 = fma(a[7], c[7], p3);
                }
                s = s - ((p0 + p1) + (p2 + p3));
                for (; k < j; ++k) s = fma(-rt[k], rj[k], s);
            }
            if (t == j) {
                pivot_s = s;
                floor_s = (double)(j + 2) * 2.220446049250313e-16 * L[t * S + j];   // ((j + 2) 2^-52 H_jj: the pivot's own rounding error)
            }
            __syncthreads();
            const double p = pivot_s;
            if (!(p > floor_s && p <= 1.79769313486231570e308)) {
                status = 1;
                break;
            }
            const double ljj = sqrt(p);
            if (t == j) L[t * S + j] = ljj;
            else if (t > j && t < D) L[t * S + j] = s / ljj;
            __syncthreads();
        }
    }
    if (status == 0) {
        b = t < D ? gs[t] : 0.0;
        for (int j = 0; j < D; ++j) {   // L y = g
            if (t == j) ys[j] = b / L[j * S + j];
            __syncthreads();
            if (t > j && t < D) b = fma(-L[t * S + j], ys[j], b);
        }
        b = t < D ? ys[t] : 0.0;        // (its own slot)
        for (int j = D - 1; j >= 0; --j) {   // L^T delta = y
            if (t == j) dl[j] = b / L[j * S + j];
            __syncthreads();
            if (t < j) b = fma(-L[j * S + t], dl[j], b);
        }
        __syncthreads();
    }
    const bool ok = status == 0;
    if (t < D) step[t] = ok ? dl[t] : 0.0;
    for (int idx = t; idx < D * D; idx += GLMNW_SOLVE_THREADS) {
        const int r = idx / D, c = idx % D;
        chol[idx] = ok && c <= r ? L[r * S + c] : 0.0;
    }
    if (t == 0) {
        double lp = logl + logpi;
        if (!(fabs(lp) <= 1.79769313486231570e308)) lp = -1e100;
        double dec = 0.0, ldet = 0.0;
        if (ok) {
            for (int c = 0; c < D; ++c) dec = fma(gs[c], dl[c], dec);
            for (int c = 0; c < D; ++c) ldet += log(L[c * S + c]);
            ldet = 2.0 * ldet;
        }
        info[0] = lp;
        info[1] = dec;
        info[2] = ldet;
        info[3] = (double)status;
    }
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------
// host side
int glm_curv_groups(int n, int D) {
    (void)D;
    const int nblk = (n + GLMNW_ROWS - 1) / GLMNW_ROWS;
    return nblk < GLMNW_MAX_GROUPS ? nblk : GLMNW_MAX_GROUPS;
}

template <int NT>
static hipError_t glm_curv_launch_k(const GlmSpec &gl, const double *theta, double *partials, int G, hipStream_t st) {
    if (gl.family == GLM_LOGISTIC) hipLaunchKernelGGL((glm_curv_kernel<NT, GLM_LOGISTIC>), dim3(G), dim3(256), 0, st, gl, theta, partials, G);
    else if (gl.family == GLM_POISSON) hipLaunchKernelGGL((glm_curv_kernel<NT, GLM_POISSON>), dim3(G), dim3(256), 0, st, gl, theta, partials, G);
    else return hipErrorInvalidConfiguration;
    return hipGetLastError();
}

hipError_t launch_glm_curv(const GlmSpec &gl, const double *theta, double *out, double *partials, hipStream_t st) {
    const int G = glm_curv_groups(gl.n, gl.D), D = gl.D;
    hipError_t e = hipErrorInvalidConfiguration;
    switch ((D + 15) / 16) {   // (NT: 16 NT >= D)
        case 1: e = glm_curv_launch_k<1>(gl, theta, partials, G, st); break;
        case 2: e = glm_curv_launch_k<2>(gl, theta, partials, G, st); break;
        case 3: e = glm_curv_launch_k<3>(gl, theta, partials, G, st); break;
        case 4: e = glm_curv_launch_k<4>(gl, theta, partials, G, st); break;
        case 5: e = glm_curv_launch_k<5>(gl, theta, partials, G, st); break;
        case 6: e = glm_curv_launch_k<6>(gl, theta, partials, G, st); break;
        case 7: e = glm_curv_launch_k<7>(gl, theta, partials, G, st); break;
        case 8: e = glm_curv_launch_k<8>(gl, theta, partials, G, st); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(glm_curv_merge_kernel, dim3((1 + D + D * D + 255) / 256), dim3(256), 0, st, partials, out, gl.logl0, D, G);
    return hipGetLastError();
}

hipError_t launch_glm_newton_solve(const double *curv, const GaussPriorSpec *prior, const double *theta, double *step, double *chol,
                                   double *info, int D, hipStream_t st) {
    const size_t lds = glm_newton_solve_lds(D);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(glm_newton_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)glm_newton_solve_lds(128));
    if (e != hipSuccess) return e;
    GaussPriorSpec p;
    p.m = nullptr; p.r = nullptr; p.logc = 0.0; p.D = D;
    if (prior) p = *prior;
    hipLaunchKernelGGL(glm_newton_solve_kernel, dim3(1), dim3(GLMNW_SOLVE_THREADS), lds, st, curv, p, prior ? 1 : 0, theta, step, chol, info, D);
    return hipGetLastError();
}

}  // namespace nnest
