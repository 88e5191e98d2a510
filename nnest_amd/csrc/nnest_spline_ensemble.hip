// nnest_spline_ensemble.hip -- emcee's STRETCH MOVE in the latent space of the neural-spline flow, every step of a chunk in ONE launch
// (include/nnest_hip.h nnest_spline_ensemble_steps).  BUILD-DEFINED STREAM, EMCEE'S MOVE.  The definition is nnest_ensemble_steps's
// (nnest_ensemble.hip has it in full), with the same split table, the same draws and the same arithmetic (ensemble_common.h): only
// the flow differs -- the spline's inverse (spline_inverse.h) replaces the coupling stack -- and with it the layout.
//
// Layout: the TEAM tile of the spline proposal kernels (spline_latent.h, which also states the target): 16 walkers per workgroup,
// four waves per tile.  Every wave carries the same 16 walkers in the parity-class tiles of flow_tile.h (z, x and lp stay in
// registers for the launch) and takes the same decisions; only the spline evaluations of the inverse are divided between the waves
// (SplineInverseTeam).  Wave 0 stores.  T's scale and offset and the box sit in LDS ([4][32 NT] floats: spl_tile_setup), read per
// evaluation as the lane's eight dimensions.
//
// A step is two half-steps, each ONE tile evaluation.  In half h the lanes whose walker is in set h propose against their partner's
// row; the other lanes, and rows >= C, evaluate their own point and the result is discarded (as slice_body treats idle walkers).
// T(x) per lane element (float32, no contraction), the box as a tile reduction (one ballot), the likelihood loglike_tile at scale 1
// on T(x).  The log-det (summed through LDS in the same order on every wave, then over the four lane groups by group_sum) and the
// likelihood (group_sum_wide) come out bit-identical on the four lane groups of a walker and on the four waves, so the decision
// does: the waves never exchange it.
//
// Hand-off: the protocol of ens_walk (nnest_ensemble.hip), through the same two functions (ensemble_common.h ens_wait /
// ens_publish): per-walker step counts in the work buffer's tags, history rows as the channel, a relaxed agent-scope poll with
// s_sleep, ONE acquire, ONE release fence before the tag store.  Every wave loads partner rows, so every wave polls and acquires
// for itself: lanes 0-15 poll their own walker's partner tag and the loop ends on a ballot.
//
// TWO PUBLISHES PER STEP, and why the launch completes.  A tile holds walkers of both sets.  After half 0 of step t it publishes
// the history rows and the tags (t + 1) of its set-0 walkers, after half 1 those of its set-1 walkers.  Half 0 of step t waits for
// set-1 partners at tag t: their half 1 of step t - 1, or their half 0 if they were in set 0 then.  Half 1 of step t waits for
// set-0 partners at tag t + 1: their half 0 of step t.  So every wait points to an earlier (step, half) -- partners in the same tile
// included: wave 0 publishes half 0 before it polls for half 1, and no workgroup barrier lies between the end of an evaluation and
// the publish.  By induction over (step, half) every wait is met whenever every workgroup is resident.  (With ONE publish at the
// end of a step, half 1 of step t in tile A could wait for a set-0 walker of tile B whose tag only moves after B's half 1, which
// could wait for a set-0 walker of A: a cycle.)  History rows are never overwritten in a launch, so a reader that is behind still
// finds its row.  The launcher refuses populations beyond the resident grid; it never launches a grid it has not proven resident.
// Every poll keeps the wall-clock bound (ENS_SPIN_TICKS) and the error word: a wait that runs out ends every wave -- a wave that has
// ended no longer counts at the workgroup's barriers, so its team mates go on to their next poll, see the word and leave -- and the
// call returns NNEST_E_HIP.
//
// Compiled with -mllvm -disable-machine-licm, as nnest_spline_mh.hip is: a step loop around the same inverse.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ensemble_common.h"
#include "spline_latent.h"

namespace nnest {

// The walk of one tile (16 walkers, this wave's copy) through the S steps of a launch.  tpar: [4][32 NT] in LDS -- std, mean, lo, hi
// (padded dims: 0, 0, -inf, +inf).  `writer`: the wave that stores and publishes.
template <int NT, class Inv>
__device__ __forceinline__ void ens_tile_walk(const EnsArgs &a, int D, int tile, int lane, const Inv &inv, const float *tpar, bool writer) {
    const int S = a.S, C = a.C;
    const int row = tile * SPL_TILE_WALKERS + (lane & 15);
    const bool ok = row < C;
    const bool store = writer && ok;
    int *err = a.work;
    unsigned *tags = reinterpret_cast<unsigned *>(a.work + ENS_CTRL_WORDS);
    const int *inds = a.work + ens_split_off(C);
    const int *members = inds + (size_t)S * C;
    const int n0 = (C + 1) / 2;
    LikeSpec like = a.like;
    like.scale = 1.0f;
    const int constrained = a.constrained;
    const double loglstar = a.loglstar;

    // x <- f^-1(x) in place; returns lp
    auto target = [&](f32x4 (&xs)[2][NT]) -> double {
        return spl_tile_eval<NT>(inv, tpar, like, D, lane, xs, [&](double logl, float ld, bool in_prior) {
            return ens_target(logl, ld, in_prior, constrained, loglstar);
        });
    };

    // ONE loop over the launch's evaluations, so that the inverse is inlined once: hs = -1 is the initial evaluation (nobody moves,
    // every walker takes its own point's x and lp), then the half-steps hs = 2 i + half
    f32x4 z[2][NT], x[2][NT];
    load_tile<NT>(a.z_in, row, ok, D, lane, z);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < NT; ++t) x[c][t] = z[c][t];
    double lp = 0.0;
    int n_acc = 0, set = -1, j = 0;
    float zz = 1.f, u3 = 1.f;
#pragma unroll 1
    for (int hs = -1; hs < 2 * S; ++hs) {
        const bool init = hs < 0;
        const int i = hs >> 1, half = hs & 1;
        if (!init && half == 0) {   // the step's draws: the walker's set, its partner in the other set, zz, u3
            set = ok ? inds[(size_t)i * C + row] : -1;
            const int Nc = set ? n0 : C - n0, cbase = set ? 0 : n0;
            const EnsU u = ens_uniforms(a.seed, (uint64_t)row, a.step0 + (uint32_t)i);
            const int jr = (int)(((uint64_t)u.m2 * (uint64_t)Nc) >> 24);
            j = ok ? members[(size_t)i * C + cbase + jr] : 0;
            zz = ens_zz(u.u1);
            u3 = u.u3;
        }
        const bool moving = !init && set == half;
        const unsigned need = init ? 0u : (half ? (unsigned)i + 1u : (unsigned)i);   // the partner's position after step t - 1 (set 0) or t (set 1)
        if (need > 0 && !ens_wait(tags, err, j, need, moving && lane < 16)) return;   // a hand-off wait ran out: the call reports it
        f32x4 q[2][NT], xq[2][NT];
        load_tile<NT>(need == 0 ? a.z_in + (size_t)j * D : a.hist_z + ((size_t)j * S + (need - 1)) * D, 0, moving, D, lane, q);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {   // the proposal; a walker that does not move in this half: its own point
                q[c][t].x = moving ? ens_propose(q[c][t].x, z[c][t].x, zz) : z[c][t].x;
                q[c][t].y = moving ? ens_propose(q[c][t].y, z[c][t].y, zz) : z[c][t].y;
                q[c][t].z = moving ? ens_propose(q[c][t].z, z[c][t].z, zz) : z[c][t].z;
                q[c][t].w = moving ? ens_propose(q[c][t].w, z[c][t].w, zz) : z[c][t].w;
                xq[c][t] = q[c][t];
            }
        const double lpq = target(xq);
        const bool acc = moving && ens_accept(lpq, lp, zz, u3, D);
        const bool take = acc || init;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                z[c][t].x = take ? q[c][t].x : z[c][t].x; z[c][t].y = take ? q[c][t].y : z[c][t].y;
                z[c][t].z = take ? q[c][t].z : z[c][t].z; z[c][t].w = take ? q[c][t].w : z[c][t].w;
                x[c][t].x = take ? xq[c][t].x : x[c][t].x; x[c][t].y = take ? xq[c][t].y : x[c][t].y;
                x[c][t].z = take ? xq[c][t].z : x[c][t].z; x[c][t].w = take ? xq[c][t].w : x[c][t].w;
            }
        lp = take ? lpq : lp;
        if (init && a.lp_in && ok) lp = a.lp_in[row];
        n_acc += acc ? 1 : 0;
        if (writer && !init) {   // publish this half's walkers: their history rows, then their step counts
            const bool mine = store && moving;
            const long hr = (long)row * S + i;
            store_tile<NT>(a.hist_z, hr, mine, D, lane, z);
            store_tile<NT>(a.hist_x, hr, mine, D, lane, x);
            if (mine && lane < 16) a.hist_lp[hr] = lp;
            ens_publish(tags, row, (unsigned)i + 1u, mine && lane < 16);
        }
    }
    if (!store) return;
    store_tile<NT>(a.z_out, row, true, D, lane, z);
    store_tile<NT>(a.x_out, row, true, D, lane, x);
    if (lane < 16) {
        a.lp_out[row] = lp;
        if (a.n_accept) a.n_accept[row] = n_acc;
    }
}

template <int NT, int NH>
__global__ void __launch_bounds__(256) spline_ensemble_kernel_team(EnsArgs a, SplArgs q) {
    extern __shared__ __attribute__((aligned(16))) float lds_buf[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const SplTile<NT, NH> t = spl_tile_setup<NT, NH>(lds_buf, q, a.t_std, a.t_mean, a.lo, a.hi, lane, wv);
    ens_tile_walk<NT>(a, q.sp.D, blockIdx.x, lane, t.inv, t.tpar, wv == 0);
}

// ------------------------------------------------------------------------------------------------
// host side
template <int NT, int NH>
static hipError_t spl_ens_launch_t(const EnsArgs &a, const SplArgs &q, int num_cu, bool launch, int *max_walkers, hipStream_t st) {
    const void *fn = reinterpret_cast<const void *>(spline_ensemble_kernel_team<NT, NH>);
    const size_t lds = (size_t)spl_tile_lds_floats(q.sp.D, NT) * sizeof(float);
    int per_cu = 0;
    hipError_t e = ens_blocks_per_cu(fn, lds, &per_cu);
    if (e != hipSuccess) return e;
    *max_walkers = SPL_TILE_WALKERS * per_cu * num_cu;
    if (!launch) return hipSuccess;
    if (a.C > *max_walkers) return hipErrorInvalidConfiguration;   // (never a grid that is not proven resident)
    hipLaunchKernelGGL((spline_ensemble_kernel_team<NT, NH>), dim3((a.C + SPL_TILE_WALKERS - 1) / SPL_TILE_WALKERS), dim3(256), lds, st, a, q);
    return hipGetLastError();
}

// launch (when `launch` and C fits) or only size: *max_walkers = the resident population of the instantiation the call would run
static hipError_t spl_ens_dispatch(const EnsArgs &a, const SplArgs &q, int num_cu, bool launch, int *max_walkers, hipStream_t st) {
    return spl_tile_for_shape(q.sp, [&](auto sh) {
        return spl_ens_launch_t<decltype(sh)::NT, decltype(sh)::NH>(a, q, num_cu, launch, max_walkers, st);
    });
}

hipError_t spline_ensemble_max_walkers(const SplArgs &q, int num_cu, int *out) {
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    return spl_ens_dispatch(a, q, num_cu, false, out, 0);
}

// the size query, the residency refusal, the split, the launch and the error word (ens_run of nnest_ensemble.hip, for this kernel)
int launch_spline_ensemble(const SplArgs &q, const EnsArgs &a, int num_cu, hipStream_t st, char *msg, size_t msg_len) {
    const char *name = "spline_ensemble_kernel_team";
    int max_walkers = 0;
    hipError_t e = spl_ens_dispatch(a, q, num_cu, false, &max_walkers, st);
    if (e == hipErrorInvalidConfiguration) {
        snprintf(msg, msg_len, "spline ensemble: x_dim=%d hidden_dim=%d not instantiated", q.sp.D, q.sp.H);
        return NNEST_E_UNSUPPORTED;
    }
    if (e != hipSuccess) { snprintf(msg, msg_len, "occupancy query: %s", hipGetErrorString(e)); return NNEST_E_HIP; }
    if (a.C > max_walkers) {
        snprintf(msg, msg_len, "spline ensemble: %d walkers > %d resident (%d walkers per workgroup, every workgroup resident); the round route takes it",
                 a.C, max_walkers, SPL_TILE_WALKERS);
        return NNEST_E_UNSUPPORTED;
    }
    if ((e = launch_ensemble_split(a.work, nullptr, a.C, a.S, a.step0, a.seed, st)) != hipSuccess) {
        snprintf(msg, msg_len, "split: %s", hipGetErrorString(e));
        return NNEST_E_HIP;
    }
    if ((e = spl_ens_dispatch(a, q, num_cu, true, &max_walkers, st)) != hipSuccess) {
        snprintf(msg, msg_len, "%s: %s", name, hipGetErrorString(e));
        return NNEST_E_HIP;
    }
    return ens_finish(a.work, name, st, msg, msg_len);
}

}  // namespace nnest
