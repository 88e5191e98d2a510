// solo_latent.h -- the LATENT TARGET in the solo layout (nnest_solo.hip's: one walker per wave, lane = 32 n + 16 h + p holds dims
// 2U p + 2u + c, the four (n, h) rows hold copies), stated once for the fused kernels that evaluate it: ensemble_x_kernel
// (nnest_ensemble.hip) and the walks of nnest_mcmc.hip and its five siblings.  (ensemble_kernel and importance_kernel
// each keep a written-out copy of this text, for a measured reason: see the comment above each.  Their launchers use the LDS size
// and the shape table below.)
//   z -> x = f^-1(z), ld = log|det dx/dz|;  T(x) = x std + mean per dimension (float32, no contraction: ens_T);  the box on T(x), a NaN
//   coordinate counting as inside;  logL = safe_loglike(T(x)) at scale 1.
// Two halves.  SoloFlow is f^-1: the weights' staging in LDS, the lane's share of the three blocks, the inverse.  SoloBox is
// everything behind it: T and the box (map), or both and the likelihood (eval).  The x-space kernel uses the box half alone; the walks on
// a data likelihood use the map and bring their own likelihood.  What a kernel makes of (logL, ld, in_prior) -- ens_target with its
// loglstar, mcmc_target_tempered -- is its own last line: the `combine` it hands over.
// Beside them: the rows' load and store, the lane's normals of a Philox-drawn row, and the table of instantiated shapes.
#pragma once
#include "ensemble_common.h"
#include "flow_tile.h"
#include "nnest_internal.h"
#include "solo_loglike.h"
#include "solo_tile.h"

namespace nnest {

// ---- rows: this lane's 2U dims of a [D] row (padded dims read 0 and are not written) ----
template <int U>
__device__ __forceinline__ void solo_load_row(const float *base, int D, int pos, float (&v)[2][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = 2 * U * pos + 2 * u + c;
            v[c][u] = d < D ? base[d] : 0.f;
        }
}
template <int U>
__device__ __forceinline__ void solo_store_row(float *base, int D, int pos, const float (&v)[2][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = 2 * U * pos + 2 * u + c;
            if (d < D) base[d] = v[c][u];
        }
}

// the float64 sum of squares of a row (padded dims hold 0), the same bits on every lane of the wave: importance_kernel's order (the
// lane's dims in order, then a butterfly over the row's 16 positions).  The global step of the mixed walk and its heirs weighs
// with it (nnest_mcmc_mixed.hip, _adapt, _gdata, _glm, _glm_prior)
template <int U>
__device__ __forceinline__ double solo_row_zz(const float (&v)[2][U]) {
    double zz = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) zz += (double)v[c][u] * (double)v[c][u];   // (the product of two float32 is exact in float64)
    zz += __shfl_xor(zz, 1);
    zz += __shfl_xor(zz, 2);
    zz += __shfl_xor(zz, 4);
    zz += __shfl_xor(zz, 8);
    return zz;
}

// ---- the flow half: NormalizingFlow.inverse (networks.py:34-42) of the default NVP shape ----
// dynamic LDS of a kernel that holds a SoloFlow: the packed nets (x_dim <= 64: gathered into registers behind the barrier), or the
// three blocks' gathered fields (x_dim > 64: the weights stay in LDS; solo_lds_weights<U, 4>)
template <int U>
inline size_t solo_flow_lds_bytes(const FlowShape &s) {
    return U >= 3 ? (size_t)3 * SOLO4_NF * 64 * sizeof(float) : (size_t)s.nets_params() * sizeof(float);
}

template <int U>
struct SoloFlow {
    static constexpr bool LDSW = U >= 3;
    SoloNet<U> net[LDSW ? 1 : 3];
    const float *wlds;
    unsigned sel;
    bool h1;
    int lane;

    // the whole workgroup (256 threads), in front of its barrier
    static __device__ __forceinline__ void stage(float *wlds, const FlowShape &s, const float *packed, int lane, int wave) {
        if constexpr (!LDSW) {
            const int n = s.nets_params();
            for (int i = threadIdx.x; i < n; i += blockDim.x) wlds[i] = packed[i];
        } else if (wave < 3) {
            SoloNet<U> nb;
            solo_gather<U>(nb, packed + (size_t)(wave * 2 + (lane >= 32 ? 1 : 0)) * s.net_params, s.D, (wave + 1) & 1, wave & 1, lane);
            solo4_store<U>(wlds, wave, nb, lane);
        }
    }
    // behind the barrier: the lane's share of the three blocks
    __device__ __forceinline__ void init(const float *wlds_, const FlowShape &s, int lane_) {
        wlds = wlds_;
        lane = lane_;
        const bool translate_half = lane >= 32;
        if constexpr (!LDSW) {
#pragma unroll
            for (int b = 0; b < 3; ++b)
                solo_gather<U>(net[b], wlds + (size_t)(b * 2 + (translate_half ? 1 : 0)) * s.net_params, s.D, (b + 1) & 1, b & 1, lane);
        }
        sel = translate_half ? 0xffffffffu : 0u;
        h1 = (lane & 16) != 0;
    }
    // x <- f^-1(x) in place, blocks 2, 1, 0; returns the lane's log-det partial (solo_logdet_total sums it)
    __device__ __forceinline__ float inverse(float (&xs)[2][U]) const {
        if constexpr (LDSW) {
            float ld = solo_coupling_inverse4<U>(Solo4Lds{wlds + (size_t)2 * SOLO4_NF * 64, lane}, sel, h1, xs[1], xs[0]);
            ld += solo_coupling_inverse4<U>(Solo4Lds{wlds + (size_t)1 * SOLO4_NF * 64, lane}, sel, h1, xs[0], xs[1]);
            ld += solo_coupling_inverse4<U>(Solo4Lds{wlds, lane}, sel, h1, xs[1], xs[0]);
            return ld;
        } else {
            float ld;
            solo_coupling_inverse<U, true>(net[2], sel, h1, xs[1], xs[0], ld);
            solo_coupling_inverse<U, false>(net[1], sel, h1, xs[0], xs[1], ld);
            solo_coupling_inverse<U, false>(net[0], sel, h1, xs[1], xs[0], ld);
            return ld;
        }
    }
};

// ---- the box half: T, the box on T(x), the likelihood at scale 1 ----
template <int U, int LK>
struct SoloBox {
    float sd[2][U], mu[2][U], blo[2][U], bhi[2][U];
    bool live[2][U];   // the lane's dims below D
    LikeSpec like;
    int D, lane;

    // a: the kernel's arguments (EnsArgs, McmcArgs, ImpArgs: like, t_std, t_mean, lo, hi); pos = lane & 15, the kernel's own value.
    // t_std / t_mean NULL: T = identity (x * 1 + 0 in float32); lo / hi NULL: no box.  Padded dims: T = 0, always inside.
    // (Read from `a` and indexed by the kernel's `pos`, not handed over pointer by pointer and indexed by a lane & 15 of its own:
    // that form spilled 27 SGPRs for 8 in importance_kernel<4, 0>, then still on this header, and cost it 2.5 % of a launch, 7.57 ->
    // 7.76 ms at x_dim 100 (profiles/latent_target/timing.txt, section 2); mcmc_kernel's spills follow the same pattern.)
    template <class Args>
    __device__ __forceinline__ void init(const Args &a, int D_, int lane_, int pos) {
        D = D_;
        lane = lane_;
        like = a.like;
        like.scale = 1.0f;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int d = 2 * U * pos + 2 * u + c;
                const bool v = d < D;
                live[c][u] = v;
                sd[c][u] = v ? (a.t_std ? a.t_std[d] : 1.f) : 0.f;
                mu[c][u] = v && a.t_mean ? a.t_mean[d] : 0.f;
                blo[c][u] = v && a.lo ? a.lo[d] : -INFINITY;
                bhi[c][u] = v && a.hi ? a.hi[d] : INFINITY;
            }
    }
    // tx = T(xs); returns in_prior: the whole row inside the box.
    // tx may BE xs (ensemble_x_kernel maps its row in place): element (c, u) of xs is read once, before element (c, u) of tx is
    // written, and xs is not read again behind the loop.
    __device__ __forceinline__ bool map(const float (&xs)[2][U], float (&tx)[2][U]) const {
        int ok = 1;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                tx[c][u] = ens_T(xs[c][u], sd[c][u], mu[c][u]);
                ok &= !(tx[c][u] < blo[c][u] || tx[c][u] > bhi[c][u]);   // (NaN counts as inside: UniformPrior, priors.py)
            }
        return __ballot(ok != 0) == ~0ull;
    }
    // tx = T(xs), then the likelihood: returns combine(safe logL(tx), ld, in_prior) -- the kernel's own last line.  tx may BE xs, as
    // in map.  A kernel with a likelihood of its own (the data likelihoods of nnest_mcmc_gdata.hip, _glm, _glm_prior) calls map and
    // goes on from tx itself.
    // (map's loop written out, not called: with the call, ensemble_x_kernel and every LK = -1 walk kernel at U >= 2 compiled to
    // another schedule and other SGPR spills -- profiles/mcmc_shared_walk/resources.txt -- and each would have wanted its timing.)
    // (Handed on, not given back through references: out-parameters change hipcc's code for the surrounding kernel; spline_latent.h)
    template <class Combine>
    __device__ __forceinline__ double eval(const float (&xs)[2][U], float (&tx)[2][U], float ld, Combine &&combine) const {
        int ok = 1;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                tx[c][u] = ens_T(xs[c][u], sd[c][u], mu[c][u]);
                ok &= !(tx[c][u] < blo[c][u] || tx[c][u] > bhi[c][u]);   // (NaN counts as inside: UniformPrior, priors.py)
            }
        const bool in_prior = __ballot(ok != 0) == ~0ull;
        const double logl = solo_loglike<U, LK>(like, D, lane, tx);
        return combine(logl, ld, in_prior);
    }
};

// the two halves in a row: x <- f^-1(x) in place; returns combine(logL(T(x)), log|det|, in_prior)
template <int U, int LK, class Combine>
__device__ __forceinline__ double solo_latent_eval(const SoloFlow<U> &flow, const SoloBox<U, LK> &box, float (&xs)[2][U], Combine &&combine) {
    const float ld = solo_logdet_total(flow.inverse(xs));
    float tx[2][U];
    return box.eval(xs, tx, ld, combine);
}

// ---- the lane's normals of a row drawn four dims to a Philox block: draw(g) -> the f32x4 of dims 4g .. 4g + 3.  The lane's 2U
// consecutive dims start at dim 2U pos: component 0 or 2 of block g0, in one block (U = 1: half of one; U = 2: exactly one) or in
// two (U = 3, 4); every (n, h) row draws the same blocks, so the copies stay copies ----
template <int U, class Draw>
__device__ __forceinline__ void solo_lane_normals(int pos, Draw &&draw, float (&e)[2][U]) {
    constexpr int NB = U <= 2 ? 1 : 2;
    const uint32_t g0 = (uint32_t)(2 * U * pos) >> 2;
    const uint32_t offm = ((2 * U * pos) & 3) != 0 ? 0xffffffffu : 0u;
    float n[4 * NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const f32x4 v = draw(g0 + (uint32_t)b);
        n[4 * b] = v.x; n[4 * b + 1] = v.y; n[4 * b + 2] = v.z; n[4 * b + 3] = v.w;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int k = 2 * u + c;
            e[c][u] = n[k];
            // (a lane whose dims start at component 2; a mask, as the coupling code selects: as `off2 ? n[k + 2] : n[k]` the
            // compiler selects the address and keeps n in scratch)
            if constexpr ((U & 1) != 0)
                e[c][u] = __uint_as_float((__float_as_uint(n[k]) & ~offm) | (__float_as_uint(n[k + 2]) & offm));
        }
}

// ---- the instantiated shapes: U = NT in 1 .. 4, the likelihood compiled in (Rosenbrock) or read at run time (LK = -1).
// f(SoloShape<U, LK>{}) launches, or sizes, that instantiation ----
template <int U_, int LK_>
struct SoloShape { static constexpr int U = U_, LK = LK_; };
template <class F>
inline hipError_t solo_for_shape(int NT, int like_id, F &&f) {
    const bool rosen = like_id == NNEST_LIKE_ROSENBROCK;
    switch (NT) {
        case 1: return rosen ? f(SoloShape<1, NNEST_LIKE_ROSENBROCK>{}) : f(SoloShape<1, -1>{});
        case 2: return rosen ? f(SoloShape<2, NNEST_LIKE_ROSENBROCK>{}) : f(SoloShape<2, -1>{});
        case 3: return rosen ? f(SoloShape<3, NNEST_LIKE_ROSENBROCK>{}) : f(SoloShape<3, -1>{});
        case 4: return rosen ? f(SoloShape<4, NNEST_LIKE_ROSENBROCK>{}) : f(SoloShape<4, -1>{});
    }
    return hipErrorInvalidConfiguration;
}
// ... of the kernels with no likelihood to select: f(SoloU<U>{}) for U in 1 .. 4 (the walks on data: U = NT; the kernels on rows
// that are already T(x): U = (D + 31) / 32, the lane's 2U dims with 32 U >= D)
template <int U_>
struct SoloU { static constexpr int U = U_; };
template <class F>
inline hipError_t solo_for_U(int U, F &&f) {
    switch (U) {
        case 1: return f(SoloU<1>{});
        case 2: return f(SoloU<2>{});
        case 3: return f(SoloU<3>{});
        case 4: return f(SoloU<4>{});
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
