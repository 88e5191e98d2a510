// spline_latent.h -- the LATENT TARGET on the spline flow's TEAM tile (16 walkers per workgroup, four waves per tile: every wave
// carries the same 16 walkers in the parity-class tiles of flow_tile.h, the spline evaluations of the inverse are divided between
// the waves by SplineInverseTeam), stated once for the fused kernels that evaluate it: spline_ensemble_kernel_team
// (nnest_spline_ensemble.hip), the walks of nnest_spline_mcmc.hip and its five siblings, spline_importance_kernel_team
// (nnest_spline_importance.hip).  The definition is solo_latent.h's with the spline's inverse for the coupling stack:
//   z -> x = f^-1(z), ld = log|det dx/dz|;  T(x) = x std + mean per element (float32, no contraction: ens_T);  the box on T(x) as a tile
//   reduction, a NaN coordinate counting as inside;  logL = loglike_tile(T(x)) at scale 1.
// The log-det (summed through LDS in the same order on every wave, then over the four lane groups by group_sum) and the likelihood
// come out bit-identical on the four lane groups of a walker and on the four waves.  What a kernel makes of (logL, ld, in_prior) is
// its own last line, the `combine` it hands to spl_tile_eval.  Beside the evaluation: the workgroup's LDS layout, T and the box in
// it, the lane's normals of a tile column and the table of instantiated shapes.
#pragma once
#include "ensemble_common.h"
#include "flow_tile.h"
#include "mh_common.h"
#include "nnest_internal.h"
#include "spline_train_tile.h"

namespace nnest {

#include "spline_inverse.h"

constexpr int SPL_TILE_WALKERS = 16;   // walkers per workgroup

// class c of the lane's eight consecutive values v0 (dims 0..3 of its block pair) and v1 (4..7): load_tile's layout
__device__ __forceinline__ f32x4 tile_class(const f32x4 &v0, const f32x4 &v1, int c) {
    return c ? (f32x4){v0.y, v0.w, v1.y, v1.w} : (f32x4){v0.x, v0.z, v1.x, v1.z};
}

// the float64 sum of squares of a walker's row (padded dims hold 0), the same bits on its four lane groups and on the four waves:
// spline_importance_kernel_team's order (the lane's eight dims of a tile column, column by column, then group_sum).  The global step
// of the mixed walk and its heirs weighs with it (nnest_spline_mcmc_mixed.hip, _adapt, _gdata, _glm, _glm_prior)
template <int NT>
__device__ __forceinline__ double tile_row_zz(const f32x4 (&v)[2][NT]) {
    double zz = 0.0;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 zc = v[c][tau];
            zz += (double)zc.x * (double)zc.x + (double)zc.y * (double)zc.y + (double)zc.z * (double)zc.z + (double)zc.w * (double)zc.w;
        }
    return group_sum(zz);
}

// ---- the workgroup's dynamic LDS, in floats: the waves' layout-exchange buffers [4][16][D + 1], the spline exchange [4][NT][64]
// f32x4, the log-det reduction [4][16] (spline_mh_kernel_team's three), then tpar [4][32 NT]: std, mean, lo, hi ----
__host__ __device__ inline int spl_tile_lds_tpar(int D, int NT) { return ((4 * 16 * (D + 1) + 3) & ~3) + 4 * NT * 64 * 4 + 4 * 16; }
__host__ __device__ inline int spl_tile_lds_floats(int D, int NT) { return spl_tile_lds_tpar(D, NT) + 4 * 32 * NT; }

// this wave's view of it: its inverse on the carved-up buffer, and tpar
template <int NT, int NH>
struct SplTile {
    SplineInverseTeam<NT, NH, 4> inv;
    const float *tpar;
};
// The whole workgroup (256 threads): fills tpar (t_std / t_mean NULL: T = identity, x * 1 + 0 in float32; lo / hi NULL: no box;
// padded dims: 0, 0, -inf, +inf) and meets at the barrier
template <int NT, int NH>
__device__ __forceinline__ SplTile<NT, NH> spl_tile_setup(float *lds_buf, const SplArgs &q, const float *t_std, const float *t_mean,
                                                          const float *lo, const float *hi, int lane, int wv) {
    const int D = q.sp.D;
    float *bufs = lds_buf;
    f32x4 *xch = reinterpret_cast<f32x4 *>(lds_buf + ((4 * 16 * (D + 1) + 3) & ~3));
    float *ldred = reinterpret_cast<float *>(xch + 4 * NT * 64);
    float *tpar = lds_buf + spl_tile_lds_tpar(D, NT);
    for (int d = threadIdx.x; d < 32 * NT; d += 256) {
        const bool v = d < D;
        tpar[d] = v ? (t_std ? t_std[d] : 1.f) : 0.f;
        tpar[32 * NT + d] = v && t_mean ? t_mean[d] : 0.f;
        tpar[2 * 32 * NT + d] = v && lo ? lo[d] : -INFINITY;
        tpar[3 * 32 * NT + d] = v && hi ? hi[d] : INFINITY;
    }
    __syncthreads();
    return SplTile<NT, NH>{{q.img, q.sp, bufs + (size_t)wv * 16 * (D + 1), xch, ldred, lane, wv}, tpar};
}

// tx = T(xs) of the tile; returns in_prior: the walker's row inside the box.  tpar: [4][32 NT] in LDS -- std, mean, lo, hi
template <int NT>
__device__ __forceinline__ bool spl_tile_map(const float *tpar, int lane, const f32x4 (&xs)[2][NT], f32x4 (&tx)[2][NT]) {
    const int g = lane >> 4;
    int inside = 1;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(tpar + 32 * tau + 8 * g);
        constexpr int PW = 8 * NT;   // f32x4 per parameter
        const f32x4 s0 = p[0], s1 = p[1], m0 = p[PW], m1 = p[PW + 1], l0 = p[2 * PW], l1 = p[2 * PW + 1], h0 = p[3 * PW], h1 = p[3 * PW + 1];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 sd = tile_class(s0, s1, c), mu = tile_class(m0, m1, c), lo = tile_class(l0, l1, c), hi = tile_class(h0, h1, c);
            f32x4 t;
            t.x = ens_T(xs[c][tau].x, sd.x, mu.x); t.y = ens_T(xs[c][tau].y, sd.y, mu.y);
            t.z = ens_T(xs[c][tau].z, sd.z, mu.z); t.w = ens_T(xs[c][tau].w, sd.w, mu.w);
            // (NaN counts as inside: UniformPrior, priors.py)
            inside &= !(t.x < lo.x || t.x > hi.x) & !(t.y < lo.y || t.y > hi.y) & !(t.z < lo.z || t.z > hi.z) & !(t.w < lo.w || t.w > hi.w);
            tx[c][tau] = t;
        }
    }
    return group_all(inside != 0, lane) != 0;
}

// x <- f^-1(x) in place, T and the box, then the likelihood: returns combine(logL(T(x)), ld, in_prior) -- the kernel's own last
// line -- with `like` at scale 1, ld = log|det| and in_prior as above.  A kernel with a likelihood of its own (the data likelihoods
// of nnest_spline_mcmc_gdata.hip, _glm, _glm_prior) takes the inverse and spl_tile_map and goes on from tx itself.
// (The map's loop written out, not called: with the call every kernel on this evaluation -- ensemble, walk, importance -- compiled
// to another instruction order: profiles/mcmc_shared_walk/resources.txt.  Handed on, not given back through references:
// out-parameters cost spline_importance_kernel_team<1, 1> 3 % of its launch, 12.76 -> 13.15 ms at x_dim 20:
// profiles/latent_target/timing.txt, section 2.)
template <int NT, class Inv, class Combine>
__device__ __forceinline__ double spl_tile_eval(const Inv &inv, const float *tpar, const LikeSpec &like, int D, int lane, f32x4 (&xs)[2][NT],
                                                Combine &&combine) {
    const int g = lane >> 4;
    const float ld = group_sum(inv(xs));
    f32x4 tx[2][NT];
    int inside = 1;
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(tpar + 32 * tau + 8 * g);
        constexpr int PW = 8 * NT;   // f32x4 per parameter
        const f32x4 s0 = p[0], s1 = p[1], m0 = p[PW], m1 = p[PW + 1], l0 = p[2 * PW], l1 = p[2 * PW + 1], h0 = p[3 * PW], h1 = p[3 * PW + 1];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 sd = tile_class(s0, s1, c), mu = tile_class(m0, m1, c), lo = tile_class(l0, l1, c), hi = tile_class(h0, h1, c);
            f32x4 t;
            t.x = ens_T(xs[c][tau].x, sd.x, mu.x); t.y = ens_T(xs[c][tau].y, sd.y, mu.y);
            t.z = ens_T(xs[c][tau].z, sd.z, mu.z); t.w = ens_T(xs[c][tau].w, sd.w, mu.w);
            // (NaN counts as inside: UniformPrior, priors.py)
            inside &= !(t.x < lo.x || t.x > hi.x) & !(t.y < lo.y || t.y > hi.y) & !(t.z < lo.z || t.z > hi.z) & !(t.w < lo.w || t.w > hi.w);
            tx[c][tau] = t;
        }
    }
    const bool in_prior = group_all(inside != 0, lane) != 0;
    const double logl = loglike_tile<NT>(like, D, lane, tx);
    return combine(logl, ld, in_prior);
}

// ---- the lane's normals of tile column tau of a row drawn four dims to a Philox block: draw(b) -> the f32x4 of dims 4b .. 4b + 3.
// The lane's eight dims 32 tau + 8 g .. + 7 are exactly blocks 8 tau + 2 g and 8 tau + 2 g + 1; the four lane groups of a walker draw
// different blocks, the four waves the same ones.  e[c]: class c; live[c][r]: component r of class c, dim 32 tau + 8 g + c + 2 r, is
// below D (a padded dim stays what it is) ----
template <class Draw>
__device__ __forceinline__ void tile_lane_normals(int tau, int g, int D, Draw &&draw, f32x4 (&e)[2], bool (&live)[2][4]) {
    const uint32_t b0 = (uint32_t)(8 * tau + 2 * g);
    const f32x4 n0 = draw(b0), n1 = draw(b0 + 1u);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        e[c] = tile_class(n0, n1, c);
        const int d0 = 32 * tau + 8 * g + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) live[c][r] = d0 + 2 * r < D;
    }
}

// ---- the instantiated shapes of the team tile: (NTh, NH).  f(TileShape<NT, NH>{}) launches, or sizes, that instantiation ----
template <int NT_, int NH_>
struct TileShape { static constexpr int NT = NT_, NH = NH_; };
template <class F>
inline hipError_t spl_tile_for_shape(const SplineShape &sp, F &&f) {
    if (!spline_shape_supported(sp)) return hipErrorInvalidConfiguration;
    switch (sp.NTh * 10 + sp.NH) {
        case 11: return f(TileShape<1, 1>{});
        case 21: return f(TileShape<2, 1>{});
        case 31: return f(TileShape<3, 1>{});
        case 41: return f(TileShape<4, 1>{});
        case 12: return f(TileShape<1, 2>{});
        case 22: return f(TileShape<2, 2>{});
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
