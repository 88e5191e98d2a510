// nnest_ensemble.hip -- emcee's affine-invariant STRETCH MOVE (Goodman & Weare 2010; emcee 3 EnsembleSampler with its default
// StretchMove: RedBlueMove, a = 2, nsplits = 2, randomize_split = True) in the latent space of the trained flow, as the reference's
// Sampler._ensemble_sample runs it through emcee (nnest/sampler.py:632-724).  BUILD-DEFINED STREAM, EMCEE'S MOVE: the draws are
// Philox4x32-10 words of this library, so parity with emcee is statistical (its random streams cannot be reproduced).
//
// Definition (include/nnest_hip.h has it in full).  N walkers z_k in R^D, step t (global index, 0-based):
//   split:    inds = arange(N) % 2 shuffled by Fisher-Yates from i = N - 1 down to 1, j = (m_i (i + 1)) >> 24 with m_i the top 24 bits
//             of word (i & 3) of Philox(seed; i >> 2, t, 0, stream 4): set 0 = {k : inds_k = 0} (ceil(N/2) walkers), set 1 the rest,
//             each listed in ascending walker index;
//   half 0:   every walker k of set 0 against the current positions of set 1, then half 1: set 1 against the updated set 0;
//             u1, u2, u3 = the top 24 bits of words x, y, z of Philox(seed; 0, k, t, stream 3 | k >> 32) / 2^24;
//             zz = ((a - 1) u1 + 1)^2 / a;  j = member (m2 Nc) >> 24 (= floor(u2 Nc)) of the other set;  q = z_j - (z_j - z_k) zz
//             (float32, no contraction);  lnpdiff = (D - 1) log zz + lp(q) - lp(z_k) (float64);  accept iff lnpdiff > log u3.
//   lp(z):    x = f^-1(z), ld = log|det dx/dz|, T(x) = x std + mean per dimension (float32, no contraction), logL = safe_loglike(T(x))
//             (non-finite -> -1e100), prior = 0 inside the box on T(x) (or no box), -inf outside;
//             loglstar unset: lp = (logL + ld) + prior;  set: lp = -inf if logL < loglstar, else ld + prior (sampler.py:674-689).
//
// Two routes run that definition with the same draws:
//   FUSED (ensemble_kernel): the default NVP shape of the solo layout (nnest_solo.hip: one walker per wave, the coupling inverse and
//     the likelihood in the wave's registers), every step of a chunk in ONE launch.  A walker of the moving half reads its partner's
//     position from the partner's history row: the partner publishes each finished step with an agent-scope release (its stores,
//     one release fence, one relaxed sc1 store of its step count) and the reader polls that count from one lane, relaxed, with
//     s_sleep, then takes one agent-scope acquire before reading the row (cdna_hip_programming.md Guideline 16, handoff-flag).  A
//     set-0 walker of step t needs its partner's position after step t - 1, a set-1 walker its partner's after step t, which only
//     waits on steps before t: every dependency points to an earlier (step, half), so the launch completes when every workgroup is
//     resident -- the launcher refuses populations beyond the resident grid.  History rows are never overwritten in a launch, so
//     there is no write-after-read hazard.  Every poll is bounded in wall-clock time; one that runs out sets the error word, and
//     every waiting wave then leaves.
//   ROUNDS (ensemble_propose_kernel / ensemble_accept_kernel): any flow, any likelihood.  Per half-step the propose kernel writes the
//     moving set's proposals (rows in ascending walker order), the caller maps them through the flow's inverse and the likelihood,
//     and the accept kernel applies the rule and writes the history.
// Both read the split from one table (ensemble_split_kernel), built per chunk for its steps: a run is a function of the seed, not of
// its chunking or its route.  The draws, the move's arithmetic, the work buffer's layout and the two ends of the hand-off live in
// ensemble_common.h, shared with the spline flow's fused kernel (nnest_spline_ensemble.hip: a third route, 16-walker tiles).
//
// The same move in X SPACE (ensemble_x_kernel; DESIGN.md 3.9: the emcee run EnsembleSampler.bootstrap starts from) is that definition
// with f = identity and ld = 0.  It is a third caller of the same pieces, not a second protocol: the walk through the steps of a
// launch -- partner, hand-off, proposal, accept, history, publish -- is ens_walk, which the two fused kernels call with their
// position -> lp functor; the round kernels run it with an identity map for the flow.
//
// MOVE MIXTURES (include/nnest_hip.h nnest_ensemble_moves_steps): with weights on emcee's differential-evolution move
// a step is either a stretch step or a DE step, q = z_k + (z_b - z_a) gamma with two partners of the other set and no factor in
// lnpdiff; the move of a step is a draw of (seed, t).  The fused kernels know it in their MIX instantiations only (the others are
// the stretch move's code as it was), the round kernels through the EnsMoves block of their arguments.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ensemble_common.h"
#include "flow_tile.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

// ---- the split of each step of a chunk: one wave per step, the population shuffled in LDS, one byte per walker (hence at most
// 65536 walkers: nnest_abi.hip) ----
__global__ void __launch_bounds__(64) ensemble_split_kernel(int *__restrict__ work, int C, int S, uint32_t step0, uint64_t seed) {
    extern __shared__ unsigned char inds_lds[];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= S) return;
    const uint32_t t = step0 + (uint32_t)i;
    __shared__ uint32_t words[256];
    for (int k = lane; k < C; k += 64) inds_lds[k] = (unsigned char)(k & 1);
    // Fisher-Yates, i = C - 1 .. 1, in windows of 256 indices [256 w, 256 w + 255]: the wave draws the window's 64 Philox blocks
    // (256 words) at once, lane 0 swaps
    for (int w = (C - 1) >> 8; w >= 0; --w) {
        const int lo = 256 * w > 1 ? 256 * w : 1, hi = 256 * w + 255 < C - 1 ? 256 * w + 255 : C - 1;
        const int b0 = 64 * w;
        const int b = b0 + lane;
        if (4 * b <= hi) {
            u32x4 c;
            c.x = (uint32_t)b;
            c.y = t;
            c.z = 0;
            c.w = (uint32_t)NOISE_STREAM_ENSEMBLE_SPLIT << 28;
            const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
            words[4 * lane + 0] = r.x;
            words[4 * lane + 1] = r.y;
            words[4 * lane + 2] = r.z;
            words[4 * lane + 3] = r.w;
        }
        __syncthreads();
        if (lane == 0) {
            for (int ii = hi; ii >= lo; --ii) {
                const uint32_t m = words[ii - 4 * b0] >> 8;
                const int j = (int)(((uint64_t)m * (uint64_t)(ii + 1)) >> 24);
                const unsigned char a = inds_lds[ii];
                inds_lds[ii] = inds_lds[j];
                inds_lds[j] = a;
            }
        }
        __syncthreads();
    }
    // the sets in ascending walker order: set 0 at members[0 .. n0), set 1 at members[n0 .. C)
    int *inds = work + ens_split_off(C) + (size_t)i * C;
    int *members = work + ens_split_off(C) + (size_t)S * C + (size_t)i * C;
    const int n0 = (C + 1) / 2;
    int c0 = 0, c1 = 0;   // wave-uniform
    for (int k0 = 0; k0 < C; k0 += 64) {
        const int k = k0 + lane;
        const int s = k < C ? inds_lds[k] : -1;
        const unsigned long long m0 = __ballot(s == 0), m1 = __ballot(s == 1);
        const uint32_t below0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
        const uint32_t below1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
        if (k < C) {
            inds[k] = s;
            if (s == 0) members[c0 + below0] = k;
            else members[n0 + c1 + below1] = k;
        }
        c0 += __popcll(m0);
        c1 += __popcll(m1);
    }
}

// the uniforms, exported for the checker: u [S][C][3]
__global__ void ensemble_fill_u_kernel(float *__restrict__ u, int C, int S, uint32_t step0, uint64_t seed) {
    const long n = (long)S * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int k = (int)(e % C), i = (int)(e / C);
        const EnsU v = ens_uniforms(seed, (uint64_t)k, step0 + (uint32_t)i);
        u[3 * e + 0] = v.u1;
        u[3 * e + 1] = v.u2;
        u[3 * e + 2] = v.u3;
    }
}

// the moves' draws, exported for the checker through the kernels' own functions: move [S] (ENS_MOVE_*), jb [S][C] (the DE step's
// second partner: its index in the other set's member list, after the shift past ja) and gamma [S][C].  work: the split of these steps
__global__ void ensemble_fill_moves_kernel(const int *__restrict__ work, int *__restrict__ move, int *__restrict__ jb,
                                           float *__restrict__ gamma, int C, int S, uint32_t step0, uint64_t seed, EnsMoves mv) {
    const long n = (long)S * C;
    const int n0 = (C + 1) / 2;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int k = (int)(e % C), i = (int)(e / C);
        const uint32_t t = step0 + (uint32_t)i;
        if (k == 0 && move) move[i] = ens_move_of_step(seed, t, mv.thr);
        const int set = work[ens_split_off(C) + e];
        const EnsDe de = ens_de_draws(seed, (uint64_t)k, t, ens_uniforms(seed, (uint64_t)k, t), set ? n0 : C - n0, mv);
        if (jb) jb[e] = de.jb;
        if (gamma) gamma[e] = de.gamma;
    }
}

// ------------------------------------------------------------------------------------------------
// FUSED route: one walker per wave, four walkers per workgroup, in the solo layout; the latent target -- the flow's inverse, T, the
// box, the likelihood -- is solo_latent.h's for ensemble_x_kernel (its box half); ensemble_kernel states it itself, see there.
// (struct EnsArgs: ensemble_common.h)

// The walk of one walker (one wave) through the S steps of a launch, shared by the two fused kernels: `target` maps a position in
// place to what the kernel reports beside it (the latent kernel: x = f^-1(z); the x-space kernel: T(x)) and returns lp.  This is the
// only hand-off protocol in the file.  XH: the mapped rows have a history of their own (hist_x); without it the positions' history
// (hist_z) is the run's, and x_out may be NULL.  MIX: the run mixes the stretch move with the DE move (a.mv; the move of a step is
// wave-uniform): a DE step waits for two partners instead of one, through the same ens_wait, at the same `need`; without MIX the
// code is the stretch move's alone.
template <int U, bool XH, bool MIX, class Target>
__device__ __forceinline__ void ens_walk(const EnsArgs &a, const int row, const int lane, Target &&target) {
    const int D = a.s.D, S = a.S, C = a.C;
    const int pos = lane & 15;
    const bool writer_lane = lane < 16;
    auto load_row = [&](const float *base, float (&v)[2][U]) { solo_load_row<U>(base, D, pos, v); };
    auto store_row = [&](float *base, const float (&v)[2][U]) { solo_store_row<U>(base, D, pos, v); };
    int *err = a.work;
    unsigned *tags = reinterpret_cast<unsigned *>(a.work + ENS_CTRL_WORDS);
    const int *inds = a.work + ens_split_off(C);
    const int *members = inds + (size_t)S * C;
    const int n0 = (C + 1) / 2;

    float z[2][U], x[2][U];
    load_row(a.z_in + (size_t)row * D, z);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c][u] = z[c][u];
    double lp = target(x);
    if (a.lp_in) lp = a.lp_in[row];
    int n_acc = 0;
    for (int i = 0; i < S; ++i) {
        const uint32_t t = a.step0 + (uint32_t)i;
        const int set = __builtin_amdgcn_readfirstlane(inds[(size_t)i * C + row]);
        const int Nc = set ? n0 : C - n0, cbase = set ? 0 : n0;
        const EnsU u = ens_uniforms(a.seed, (uint64_t)row, t);
        const int jr = (int)(((uint64_t)u.m2 * (uint64_t)Nc) >> 24);
        const int j = __builtin_amdgcn_readfirstlane(members[(size_t)i * C + cbase + jr]);
        const unsigned need = set ? (unsigned)i + 1u : (unsigned)i;   // the partner's position after step t - 1 (set 0) or t (set 1)
        int move = ENS_MOVE_STRETCH;
        if constexpr (MIX) move = __builtin_amdgcn_readfirstlane(ens_move_of_step(a.seed, t, a.mv.thr));
        // (the partner's row is written out at each load: behind a lambda or a helper the compiler spills more SGPRs in the MIX = false
        // instantiations than it did before there was a MIX)
        float zj[2][U], q[2][U], xq[2][U];
        float zz = 1.0f;
        if (MIX && move == ENS_MOVE_DE) {
            // partners a = j and b: lanes 0 and 1 poll one tag each, one acquire, then the two rows (the difference as b's is loaded)
            const EnsDe de = ens_de_draws(a.seed, (uint64_t)row, t, u, Nc, a.mv);
            const int jb = __builtin_amdgcn_readfirstlane(members[(size_t)i * C + cbase + de.jb]);
            if (need > 0 && !ens_wait(tags, err, lane == 0 ? j : jb, need, lane < 2)) return;
            load_row(need == 0 ? a.z_in + (size_t)j * D : a.hist_z + ((size_t)j * S + (need - 1)) * D, zj);
            load_row(need == 0 ? a.z_in + (size_t)jb * D : a.hist_z + ((size_t)jb * S + (need - 1)) * D, q);
#pragma unroll
            for (int uu = 0; uu < U; ++uu)
#pragma unroll
                for (int c = 0; c < 2; ++c) q[c][uu] = ens_de_propose(z[c][uu], zj[c][uu], q[c][uu], de.gamma);
        } else {
            if (need > 0 && !ens_wait(tags, err, j, need, lane == 0)) return;   // a hand-off wait ran out: the call reports it
            load_row(need == 0 ? a.z_in + (size_t)j * D : a.hist_z + ((size_t)j * S + (need - 1)) * D, zj);
            zz = ens_zz(u.u1);
#pragma unroll
            for (int uu = 0; uu < U; ++uu)
#pragma unroll
                for (int c = 0; c < 2; ++c) q[c][uu] = ens_propose(zj[c][uu], z[c][uu], zz);
        }
#pragma unroll
        for (int uu = 0; uu < U; ++uu)
#pragma unroll
            for (int c = 0; c < 2; ++c) xq[c][uu] = q[c][uu];
        const double lpq = target(xq);
        // (the stretch factor (D - 1) log zz; a DE step has none)
        if ((MIX && move == ENS_MOVE_DE) ? ens_accept_factor(lpq, lp, 0.0, u.u3) : ens_accept(lpq, lp, zz, u.u3, D)) {
#pragma unroll
            for (int uu = 0; uu < U; ++uu)
#pragma unroll
                for (int c = 0; c < 2; ++c) { z[c][uu] = q[c][uu]; x[c][uu] = xq[c][uu]; }
            lp = lpq;
            n_acc += 1;
        }
        const size_t hr = (size_t)row * S + i;
        if (writer_lane) {
            store_row(a.hist_z + hr * D, z);
            if constexpr (XH) store_row(a.hist_x + hr * D, x);
            if (pos == 0) a.hist_lp[hr] = lp;
        }
        // publish: the wave's stores, then its step count (release: one fence for the whole wave, one relaxed sc1 store)
        ens_publish(tags, row, (unsigned)i + 1u, lane == 0);
    }
    if (writer_lane) {
        store_row(a.z_out + (size_t)row * D, z);
        if (XH || a.x_out) store_row(a.x_out + (size_t)row * D, x);
        if (pos == 0) {
            a.lp_out[row] = lp;
            if (a.n_accept) a.n_accept[row] = n_acc;
        }
    }
}

// This kernel keeps its target WRITTEN OUT (the text solo_latent.h states for the other three kernels of the layout): its register
// allocation reacts to how the target is wrapped.  Sharing the header moved its SGPR spills (<3, -1, false> 39 -> 62, <2, -1, false>
// 37 -> 59, <1, -1, false> 39 -> 54) and tools/time_ensemble.py then measured it above the parent by more than the parent's spread at
// the wide shapes: x_dim 70 GaussianMix 7.978 -> 8.039 ms (spread 0.058), x_dim 100 GaussianMix 9.410 -> 9.487 ms (0.056), x_dim 100
// Rosenbrock 9.419 -> 9.471 ms (0.035) (profiles/latent_target/timing.txt, section 3).  As written here every instantiation is the
// parent's, instruction for instruction.
template <int U, int LK, bool MIX>
__global__ void __launch_bounds__(256) ensemble_kernel(EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = a.s.D, C = a.C;
    constexpr bool LDSW = U >= 3;   // (solo_lds_weights<U, 4>: x_dim > 64 keeps the weights in LDS)
    {
        if constexpr (!LDSW) {
            const int n = a.s.nets_params();
            for (int i = threadIdx.x; i < n; i += blockDim.x) wlds[i] = a.packed[i];
        } else if (wave < 3) {
            SoloNet<U> nb;
            solo_gather<U>(nb, a.packed + (size_t)(wave * 2 + (lane >= 32 ? 1 : 0)) * a.s.net_params, D, (wave + 1) & 1, wave & 1, lane);
            solo4_store<U>(wlds, wave, nb, lane);
        }
    }
    __syncthreads();
    const int pos = lane & 15;
    const bool translate_half = lane >= 32;
    const int row = blockIdx.x * 4 + wave;
    if (row >= C) return;   // (no barrier behind this point)
    SoloNet<U> net[LDSW ? 1 : 3];
    if constexpr (!LDSW) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
            solo_gather<U>(net[b], wlds + (size_t)(b * 2 + (translate_half ? 1 : 0)) * a.s.net_params, D, (b + 1) & 1, b & 1, lane);
    }
    const unsigned sel = translate_half ? 0xffffffffu : 0u;
    const bool h1 = (lane & 16) != 0;
    auto inverse = [&](float (&xs)[2][U]) {   // NormalizingFlow.inverse (networks.py:34-42), blocks 2, 1, 0
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
    };
    // this lane's dims: T, the box
    float sd[2][U], mu[2][U], blo[2][U], bhi[2][U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int d = 2 * U * pos + 2 * u + c;
            const bool v = d < D;
            sd[c][u] = v ? a.t_std[d] : 0.f;
            mu[c][u] = v ? a.t_mean[d] : 0.f;
            blo[c][u] = v && a.lo ? a.lo[d] : -INFINITY;
            bhi[c][u] = v && a.hi ? a.hi[d] : INFINITY;
        }
    LikeSpec like = a.like;
    like.scale = 1.0f;
    // x <- f^-1(x) in place; returns lp
    auto target = [&](float (&xs)[2][U]) -> double {
        const float ld = solo_logdet_total(inverse(xs));
        float tx[2][U];
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
        return ens_target(logl, ld, in_prior, a.constrained, a.loglstar);
    };
    ens_walk<U, true, MIX>(a, row, lane, target);
}

// The x-space run: the same walk with f = identity and ld = 0, so lp(x) = safe logL(T(x)) + prior: the box half of
// solo_latent.h alone.  No flow, hence no weights and no LDS.  The mapped row is T(x): x_out (optional) receives it.
template <int U, int LK, bool MIX>
__global__ void __launch_bounds__(256) ensemble_x_kernel(EnsArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.x * 4 + wave;
    if (row >= a.C) return;
    SoloBox<U, LK> box;
    box.init(a, a.s.D, lane, lane & 15);
    // x <- T(x) in place; returns lp
    auto target = [&](float (&xs)[2][U]) -> double {
        return box.eval(xs, xs, 0.f, [&](double logl, float ld, bool in_prior) {
            return ens_target(logl, ld, in_prior, a.constrained, a.loglstar);
        });
    };
    ens_walk<U, false, MIX>(a, row, lane, target);
}

// ------------------------------------------------------------------------------------------------
// ROUND route: one wave per moving row, each lane the dims lane, lane + 64, ...
struct EnsRoundArgs {
    const int *work;
    int C, S, D, i, half;   // chunk step i (global step step0 + i); half 0 / 1 (-1: the initial evaluation, rows = walkers)
    uint32_t step0;
    uint64_t seed;
    EnsMoves mv;
};

__device__ __forceinline__ int ens_row_walker(const EnsRoundArgs &a, int r) {
    if (a.half < 0) return r;
    const int *members = a.work + ens_split_off(a.C) + (size_t)a.S * a.C + (size_t)a.i * a.C;
    return members[(a.half ? (a.C + 1) / 2 : 0) + r];
}

__global__ void __launch_bounds__(256) ensemble_propose_kernel(EnsRoundArgs a, const float *__restrict__ z_cur, float *__restrict__ q, int rows) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int C = a.C, D = a.D, n0 = (C + 1) / 2;
    const int k = ens_row_walker(a, r);
    const int Nc = a.half ? n0 : C - n0, cbase = a.half ? 0 : n0;
    const EnsU u = ens_uniforms(a.seed, (uint64_t)k, a.step0 + (uint32_t)a.i);
    const int jr = (int)(((uint64_t)u.m2 * (uint64_t)Nc) >> 24);
    const int *others = a.work + ens_split_off(C) + (size_t)a.S * C + (size_t)a.i * C + cbase;
    const int j = others[jr];
    const uint32_t t = a.step0 + (uint32_t)a.i;
    if (ens_move_of_step(a.seed, t, a.mv.thr) == ENS_MOVE_DE) {
        const EnsDe de = ens_de_draws(a.seed, (uint64_t)k, t, u, Nc, a.mv);
        const int jb = others[de.jb];
        for (int d = lane; d < D; d += 64)
            q[(size_t)r * D + d] = ens_de_propose(z_cur[(size_t)k * D + d], z_cur[(size_t)j * D + d], z_cur[(size_t)jb * D + d], de.gamma);
        return;
    }
    const float zz = ens_zz(u.u1);
    for (int d = lane; d < D; d += 64) q[(size_t)r * D + d] = ens_propose(z_cur[(size_t)j * D + d], z_cur[(size_t)k * D + d], zz);
}

struct EnsAcceptArgs {
    const float *q, *x, *ld;        // the rows: proposals, f^-1, log|det|
    const double *logl;             // safe logL of the rows
    const double *lprior;           // log prior of the rows (the caller's), or NULL: the box below
    const float *t_std, *t_mean, *lo, *hi;   // the box on T(x) (lo / hi NULL: no prior)
    float *z_cur, *x_cur;
    double *lp_cur;
    float *hist_z, *hist_x;         // [C][S][D]
    double *hist_lp;                // [C][S]
    int *n_accept;                  // [C]
    int *acc_rows;                  // [rows] or NULL: 1 where the row's walker moved
    int constrained;
    double loglstar;
};

__global__ void __launch_bounds__(256) ensemble_accept_kernel(EnsRoundArgs a, EnsAcceptArgs b, int rows) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int D = a.D;
    const int k = ens_row_walker(a, r);
    const float *xr = b.x + (size_t)r * D;
    bool in_prior = true;
    if (b.lprior) {
        in_prior = !(b.lprior[r] == -INFINITY);
    } else if (b.lo) {
        int ok = 1;
        for (int d = lane; d < D; d += 64) {
            const float tx = ens_T(xr[d], b.t_std[d], b.t_mean[d]);
            ok &= !(tx < b.lo[d] || tx > b.hi[d]);
        }
        in_prior = __ballot(ok != 0) == ~0ull;
    }
    double lp_new = ens_target(b.logl[r], b.ld[r], in_prior, b.constrained, b.loglstar);
    if (b.lprior && in_prior) lp_new = lp_new + b.lprior[r];   // (a prior density other than 0 / -inf: sampler.py:687-689 adds it)
    bool moved;
    if (a.half < 0) {
        moved = true;
    } else {
        const EnsU u = ens_uniforms(a.seed, (uint64_t)k, a.step0 + (uint32_t)a.i);
        moved = ens_move_of_step(a.seed, a.step0 + (uint32_t)a.i, a.mv.thr) == ENS_MOVE_DE
                    ? ens_accept_factor(lp_new, b.lp_cur[k], 0.0, u.u3)
                    : ens_accept(lp_new, b.lp_cur[k], ens_zz(u.u1), u.u3, D);
    }
    const float *qr = b.q + (size_t)r * D;
    if (moved) {
        for (int d = lane; d < D; d += 64) {
            b.z_cur[(size_t)k * D + d] = qr[d];
            b.x_cur[(size_t)k * D + d] = xr[d];
        }
    }
    if (a.half >= 0) {
        const size_t hr = (size_t)k * a.S + a.i;
        for (int d = lane; d < D; d += 64) {
            b.hist_z[hr * D + d] = moved ? qr[d] : b.z_cur[(size_t)k * D + d];
            b.hist_x[hr * D + d] = moved ? xr[d] : b.x_cur[(size_t)k * D + d];
        }
    }
    if (lane == 0) {
        const double lp = moved ? lp_new : b.lp_cur[k];
        b.lp_cur[k] = lp;
        if (a.half >= 0) {
            b.hist_lp[(size_t)k * a.S + a.i] = lp;
            if (b.n_accept) b.n_accept[k] += moved ? 1 : 0;
        } else if (b.n_accept) {
            b.n_accept[k] = 0;
        }
        if (b.acc_rows) b.acc_rows[r] = moved ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// host side
size_t ensemble_work_words(int C, int S) { return ens_split_off(C) + 2 * (size_t)S * C; }

hipError_t launch_ensemble_split(int *work, float *u, int C, int S, uint32_t step0, uint64_t seed, hipStream_t st) {
    hipError_t e = hipMemsetAsync(work, 0, ens_split_off(C) * sizeof(int), st);   // the error word and the tags
    if (e != hipSuccess) return e;
    if (S > 0) {
        hipLaunchKernelGGL(ensemble_split_kernel, dim3(S), dim3(64), (size_t)C, st, work, C, S, step0, seed);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (u && S > 0) {
        hipLaunchKernelGGL(ensemble_fill_u_kernel, dim3(256), dim3(256), 0, st, u, C, S, step0, seed);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_ensemble_fill_moves(const int *work, int *move, int *jb, float *gamma, int C, int S, uint32_t step0, uint64_t seed,
                                      const EnsMoves &mv, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    hipLaunchKernelGGL(ensemble_fill_moves_kernel, dim3(256), dim3(256), 0, st, work, move, jb, gamma, C, S, step0, seed, mv);
    return hipGetLastError();
}

bool ensemble_form_eligible(const FlowShape &s) { return slice_form_eligible(s); }

// X: the x-space kernel (no flow: a.s carries D and NT only, no LDS); MIX: the instantiation that knows the DE move
template <int U, int LK, bool X, bool MIX>
static hipError_t ens_launch_k(const EnsArgs &a, int num_cu, bool launch, int *max_walkers, hipStream_t st) {
    const void *fn = X ? reinterpret_cast<const void *>(ensemble_x_kernel<U, LK, MIX>) : reinterpret_cast<const void *>(ensemble_kernel<U, LK, MIX>);
    const size_t lds = X ? 0 : solo_flow_lds_bytes<U>(a.s);
    int per_cu = 0;
    hipError_t e = ens_blocks_per_cu(fn, lds, &per_cu);
    if (e != hipSuccess) return e;
    *max_walkers = 4 * per_cu * num_cu;
    if (!launch) return hipSuccess;
    if constexpr (X) hipLaunchKernelGGL((ensemble_x_kernel<U, LK, MIX>), dim3((a.C + 3) / 4), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ensemble_kernel<U, LK, MIX>), dim3((a.C + 3) / 4), dim3(256), lds, st, a);
    return hipGetLastError();
}

// launch (when `launch` and C fits) or only size: *max_walkers = the resident population of the instantiation the call would run
template <bool X, bool MIX>
static hipError_t ens_dispatch_m(const EnsArgs &a, int num_cu, bool launch, int *max_walkers, hipStream_t st) {
    return solo_for_shape(a.s.NT, a.like.id, [&](auto sh) {
        return ens_launch_k<decltype(sh)::U, decltype(sh)::LK, X, MIX>(a, num_cu, launch, max_walkers, st);
    });
}

// a run with a DE step in it (a.mv.thr < 2^24) takes the MIX instantiation; every other run the stretch move's own, as before
template <bool X>
static hipError_t ens_dispatch(const EnsArgs &a, int num_cu, bool launch, int *max_walkers, hipStream_t st) {
    return a.mv.thr < ENS_THR_ALWAYS ? ens_dispatch_m<X, true>(a, num_cu, launch, max_walkers, st)
                                     : ens_dispatch_m<X, false>(a, num_cu, launch, max_walkers, st);
}

// the shape the x-space kernel reads: D and the solo layout's U = NT
static FlowShape ens_x_shape(int D) {
    FlowShape s;
    memset(&s, 0, sizeof(s));
    s.D = D;
    s.NT = ((D + 1) / 2 + 15) / 16;
    return s;
}

hipError_t ensemble_max_walkers(const FlowShape &s, int like_id, const EnsMoves &mv, int num_cu, int *out) {
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    a.mv = mv;
    a.s = s;
    a.like.id = like_id;
    return ens_dispatch<false>(a, num_cu, false, out, 0);
}

hipError_t ensemble_x_max_walkers(int D, int like_id, const EnsMoves &mv, int num_cu, int *out) {
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    a.mv = mv;
    a.s = ens_x_shape(D);
    a.like.id = like_id;
    return ens_dispatch<true>(a, num_cu, false, out, 0);
}

// the size query, the residency refusal, the split, the launch and the error word, for either fused kernel
template <bool X>
static int ens_run(const EnsArgs &a, int num_cu, hipStream_t st, char *msg, size_t msg_len) {
    const char *name = X ? "ensemble_x_kernel" : "ensemble_kernel";
    int max_walkers = 0;
    hipError_t e = ens_dispatch<X>(a, num_cu, false, &max_walkers, st);
    if (e != hipSuccess) { snprintf(msg, msg_len, "occupancy query: %s", hipGetErrorString(e)); return NNEST_E_HIP; }
    if (a.C > max_walkers) {
        snprintf(msg, msg_len, "ensemble: %d walkers > %d resident (one walker per wave, every workgroup resident); the round route takes it",
                 a.C, max_walkers);
        return NNEST_E_UNSUPPORTED;
    }
    if ((e = launch_ensemble_split(a.work, nullptr, a.C, a.S, a.step0, a.seed, st)) != hipSuccess) {
        snprintf(msg, msg_len, "split: %s", hipGetErrorString(e));
        return NNEST_E_HIP;
    }
    if ((e = ens_dispatch<X>(a, num_cu, true, &max_walkers, st)) != hipSuccess) {
        snprintf(msg, msg_len, "%s: %s", name, hipGetErrorString(e));
        return NNEST_E_HIP;
    }
    return ens_finish(a.work, name, st, msg, msg_len);
}

int launch_ensemble(const FlowShape &s, const float *packed, const LikeSpec &like, const float *t_std, const float *t_mean, const float *lo,
                    const float *hi, const float *z_in, const double *lp_in, float *z_out, float *x_out, double *lp_out, float *hist_z,
                    float *hist_x, double *hist_lp, int *n_accept, int *work, int C, int S, uint32_t step0, uint64_t seed, int constrained,
                    double loglstar, const EnsMoves &mv, int num_cu, hipStream_t st, char *msg, size_t msg_len) {
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    a.mv = mv;
    a.s = s; a.packed = packed; a.like = like; a.t_std = t_std; a.t_mean = t_mean; a.lo = lo; a.hi = hi;
    a.z_in = z_in; a.lp_in = lp_in; a.z_out = z_out; a.x_out = x_out; a.lp_out = lp_out;
    a.hist_z = hist_z; a.hist_x = hist_x; a.hist_lp = hist_lp; a.n_accept = n_accept; a.work = work;
    a.C = C; a.S = S; a.constrained = constrained; a.step0 = step0; a.seed = seed; a.loglstar = loglstar;
    return ens_run<false>(a, num_cu, st, msg, msg_len);
}

// the x-space run: the positions are x (EnsArgs' z slots), the mapped row is T(x) (tx_out, optional)
int launch_ensemble_x(int D, const LikeSpec &like, const float *t_std, const float *t_mean, const float *lo, const float *hi,
                      const float *x_in, const double *lp_in, float *x_out, float *tx_out, double *lp_out, float *hist_x, double *hist_lp,
                      int *n_accept, int *work, int C, int S, uint32_t step0, uint64_t seed, int constrained, double loglstar,
                      const EnsMoves &mv, int num_cu, hipStream_t st, char *msg, size_t msg_len) {
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    a.mv = mv;
    a.s = ens_x_shape(D); a.like = like; a.t_std = t_std; a.t_mean = t_mean; a.lo = lo; a.hi = hi;
    a.z_in = x_in; a.lp_in = lp_in; a.z_out = x_out; a.x_out = tx_out; a.lp_out = lp_out;
    a.hist_z = hist_x; a.hist_lp = hist_lp; a.n_accept = n_accept; a.work = work;
    a.C = C; a.S = S; a.constrained = constrained; a.step0 = step0; a.seed = seed; a.loglstar = loglstar;
    return ens_run<true>(a, num_cu, st, msg, msg_len);
}

hipError_t launch_ensemble_propose(const int *work, int C, int S, int D, int i, int half, uint32_t step0, uint64_t seed, const EnsMoves &mv,
                                   const float *z_cur, float *q, int rows, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    EnsRoundArgs a = {work, C, S, D, i, half, step0, seed, mv};
    hipLaunchKernelGGL(ensemble_propose_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a, z_cur, q, rows);
    return hipGetLastError();
}

hipError_t launch_ensemble_accept(const int *work, int C, int S, int D, int i, int half, uint32_t step0, uint64_t seed, const EnsMoves &mv,
                                  const float *q, const float *x, const float *ld, const double *logl, const double *lprior, const float *t_std,
                                  const float *t_mean, const float *lo, const float *hi, float *z_cur, float *x_cur, double *lp_cur,
                                  float *hist_z, float *hist_x, double *hist_lp, int *n_accept, int *acc_rows, int constrained,
                                  double loglstar, int rows, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    EnsRoundArgs a = {work, C, S, D, i, half, step0, seed, mv};
    EnsAcceptArgs b = {q, x, ld, logl, lprior, t_std, t_mean, lo, hi, z_cur, x_cur, lp_cur, hist_z, hist_x, hist_lp, n_accept, acc_rows,
                       constrained, loglstar};
    hipLaunchKernelGGL(ensemble_accept_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a, b, rows);
    return hipGetLastError();
}

}  // namespace nnest
