// spline_inverse.h -- the flow-inverse functors of the spline proposal kernels: `inv(xs)` inverts the spline flow on a tile of
// walkers in the parity-class layout of flow_tile.h (load_tile / store_tile) and returns the lane's log-det partial.  Shared by the
// Metropolis kernels (spline_kernels.h; nnest_spline_mh.hip) and the slice kernel (nnest_spline_slice.hip).  Included inside
// namespace nnest, behind spline_train_tile.h.
#pragma once

// one wave per 16 walkers (spline_mh_kernel)
template <int NT, int NH>
struct SplineInverse {
    const float *img;
    SplineShape sp;
    float *buf;
    int lane;
#ifdef NNEST_STAMP
    unsigned long long t_mlp = 0, t_xch = 0, t_upd = 0;
#endif
    __device__ __forceinline__ float operator()(f32x4 (&xs)[2][NT]) const {
        f32x4 t[2][NT];
        spl_from_parity<NT>(buf, sp.D, sp.nl, lane, xs, t);
        const float ld = spline_inverse_tile<NT, NH>(img, sp, lane, t);
        spl_to_parity<NT>(buf, sp.D, sp.nl, lane, t, xs);
        return ld;
    }
};

// four waves per 16 walkers (spline_mh_kernel_team): every wave carries the same walkers; the spline evaluations of the inverse are
// divided (spl_coupling TEAM = 4), and the log-det partials are summed through LDS
template <int NT, int NH, int TEAM>
struct SplineInverseTeam {
    const float *img;
    SplineShape sp;
    float *buf;     // this wave's 16 x (D+1) layout-exchange buffer
    f32x4 *xch;     // [TEAM][NT][64]
    float *ldred;   // [TEAM][16]
    int lane, wv;
#ifdef NNEST_STAMP
    unsigned long long t_mlp = 0, t_xch = 0, t_upd = 0;
#endif
    __device__ __forceinline__ float operator()(f32x4 (&xs)[2][NT]) const {
        f32x4 t[2][NT];
        spl_from_parity<NT>(buf, sp.D, sp.nl, lane, xs, t);
        float ld = group_sum(spline_inverse_tile<NT, NH, TEAM>(img, sp, lane, t, wv, xch));
        if (lane < 16) ldred[wv * 16 + lane] = ld;
        spl_team_barrier();
        const int w = lane & 15;
        ld = 0.f;
#pragma unroll
        for (int k = 0; k < TEAM; ++k) ld += ldred[k * 16 + w];
        spl_team_barrier();
        spl_to_parity<NT>(buf, sp.D, sp.nl, lane, t, xs);
        return 0.25f * ld;  // the caller sums the four lanes of a walker
    }
};

// four waves per 8 walkers, each walker held in both halves of the matrix-core columns (spline_mh_kernel_pair): the halves run the
// spline stage on different dimensions (spline_inverse_tile_halves)
template <int NT, int NH>
struct SplineInverseHalves {
    const float *img;
    SplineShape sp;
    float *buf;     // this wave's 16 x (D+1) layout-exchange buffer
    f32x4 *xch;     // 2 x [4][NT][64]: the exchanges alternate between the two (one barrier each, round 6)
    float *ldred;   // 2 x [4][16], likewise
    const float *trunks;   // the conditioners' hidden parts in LDS (spline_stage_trunks)
    int lane, wv;
    mutable int xsel = 0, lsel = 0;
#ifdef NNEST_STAMP
    unsigned long long t_mlp = 0, t_xch = 0, t_upd = 0;
#endif
    __device__ __forceinline__ float operator()(f32x4 (&xs)[2][NT]) const {
        f32x4 t[2][NT];
        spl_from_parity<NT>(buf, sp.D, sp.nl, lane, xs, t);
        float ld = group_sum(spline_inverse_tile_halves<NT, NH>(img, sp, lane, t, wv, xch, xsel, trunks));
        float *lr = ldred + ((lsel & 1) ? 64 : 0);
        lsel ^= 1;
        if (lane < 16) lr[wv * 16 + lane] = ld;
        spl_team_barrier();
        const int w = lane & 15;
        ld = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) ld += lr[k * 16 + w];
        spl_to_parity<NT>(buf, sp.D, sp.nl, lane, t, xs);
        return 0.25f * ld;  // the caller sums the four lanes of a walker
    }
};

