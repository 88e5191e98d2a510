// nnest_mh_glm.hip -- the constrained METROPOLIS proposal in latent space of the trained NVP on a GENERALISED LINEAR MODEL of the
// user's data (logistic or Poisson regression): K4's hard-constraint step (mh_body.h; reference sampler.py:229-463), operation for
// operation --
//   fs = (float)scale;  z' = z + eps * fs (float32);  x' = f^-1(z');  log_ratio = inbox(x') ? ld' - ld : -inf;
//   ratio = fminf(__expf(log_ratio), 1), a NaN stays a NaN;  pre = u < ratio;  acc = pre && logL' > L*;
//   n_call counts pre, n_accept counts acc (NNEST_MH_ALL_MOVED in bit 30)
// -- with
//   logL(x) := GLM(T(x)),  T(x)_d = ens_T(x_d, t_std[d], t_mean[d])  (SoloBox::map; NULL t_std / t_mean: the identity)
// and the likelihood of glm_data.h (float32 eta in the solo layout's order, float64 terms, rows >= n masked, the safe rule -1e100) in
// place of the analytic likelihoods.  include/nnest_hip.h nnest_mh_glm_steps; DESIGN.md 3.23.
// The box is on x (!(x < -1 || x > 1), a NaN coordinate inside), as in slice_glm_kernel -- NOT on T(x): the map gets no lo / hi.
// Draws: eps = noise_normal4(seed, walker, it, g, NOISE_STREAM_DZ), padded dims exactly 0; u = noise_uniform(seed, walker, it); or
// the recorded ones.  A chain is a function of seed, walker and step -- and, under the step rule, of the batch's votes.
//
// Layout: slice_glm_kernel's, the solo layout, one walker per wave, four walkers per workgroup; the flow half is solo_latent.h's
// SoloFlow, T is SoloBox::map, in front of glm_solo_loglike (data rows over the wave's 64 lanes).
//
// THE LIKELIHOOD IS SKIPPED where nothing reads it: a proposal with pre == false is rejected whatever its logL, and neither counter
// reads the value.  `pre` is the same on all 64 lanes -- the box's verdict is a ballot over the wave, the log-det is the wave's total
// read into a scalar register, u is one draw per walker -- so the skip is a scalar branch around glm_solo_loglike, whose readlanes
// and butterfly always see the whole wave.  No output shows it.
//
// THE STEP RULE (NNEST_MH_DYNAMIC_BATCH, sampler.py:422-431 over all C walkers): mh_common.h's counters, used in mh_body's order --
// the shard words of step it - lag are requested at the top of the step and consumed behind the decision, BEFORE this step's post
// (memory operations retire in order, and an atomic stays outstanding for microseconds); at lag 0 read and total come after the post.
// The workgroup's count is the sum of its four waves' acc, through LDS behind ONE workgroup barrier a step -- the only place where
// the four waves meet; the two count arrays alternate by step, so that a wave one step ahead does not overwrite what a slower wave
// has yet to read (a wave writes array it & 1 behind the barrier of step it - 1, which every wave reaches after reading the counts
// of step it - 2).  A wave whose row is >= C runs the loop and meets the barrier: it proposes nothing and counts 0.  Every wave of
// the grid reads the total itself and applies the same vote, in double: the scale is the same number on every wave.
// The waits are mh_common.h's bounded ones, and the launcher refuses a grid that is not proven resident (below).
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "glm_data.h"
#include "mh_glm.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

template <int U, int FAM>
__global__ void __launch_bounds__(256) mh_glm_kernel(FlowShape s, const float *__restrict__ packed, MhGlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    __shared__ __attribute__((aligned(16))) float x0buf[4][16][2 * U];   // the chains' first x (the usable-chain test at the end)
    __shared__ int wave_acc[2][4];                                        // the waves' acc of a step, alternating by step
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, S = a.steps, C = a.C;
    SoloFlow<U>::stage(wlds, s, packed, lane, wave);
    __syncthreads();
    const int pos = lane & 15;
    const bool writer_lane = lane < 16;
    const int row = blockIdx.x * 4 + wave;
    const bool ok = row < C;   // (scalar)
    const bool batch = (a.flags & NNEST_MH_DYNAMIC_BATCH) != 0;
    const int lag = mh_flag_lag(a.flags);
    const int nwg = gridDim.x;
    if (!ok && !batch) return;   // (fixed step: no barrier behind this point)
    SoloFlow<U> flow;
    flow.init(wlds, s, lane);
    SoloBox<U, NNEST_LIKE_GAUSSIAN> box;   // (T alone: lo / hi are NULL, its likelihood is not called)
    box.init(a, D, lane, pos);
    const double loglstar = a.loglstar;
    // x <- f^-1(x) in place; the walker's log-det as a scalar (the same bits on every lane)
    auto inverse = [&](float (&xs)[2][U]) -> float {
        const float ld = solo_logdet_total(flow.inverse(xs));
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ld)));
    };
    auto store_row = [&](float *base, size_t r, const float (&v)[2][U]) { solo_store_row<U>(base + r * D, D, pos, v); };

    float z[2][U], x[2][U];
    float ld = 0.f;
    double logl = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) z[c][u] = x[c][u] = 0.f;
    if (ok) {
        solo_load_row<U>(a.z + (size_t)row * D, D, pos, z);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) x[c][u] = z[c][u];
        ld = inverse(x);
        logl = a.logl[row];
        if (writer_lane && a.x) {   // the chain's first x waits in LDS (usable-chain test at the end, nested.py:432; a lane reads back its own)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) x0buf[wave][pos][2 * u + c] = x[c][u];
        }
        if (writer_lane && a.hist_x) store_row(a.hist_x, (size_t)row * (S + 1), x);
        if (lane == 0 && a.hist_logl) a.hist_logl[(size_t)row * (S + 1)] = logl;
    }
    const uint64_t walker = a.walker_offset + (uint64_t)row;
    double scale = (double)a.step_size;   // python float in the reference (sampler.py:255, :428-431)
    MhGlmVotes votes;
    int n_acc = 0, n_call = 0;
#pragma unroll 1
    for (int it = 1; it <= S; ++it) {
        // the batch rule: the counts of step it - lag are requested now and consumed behind the decision
        unsigned long long early = 0;
        const bool have_total = batch && it - lag >= 1;
        if (have_total && lag > 0) early = mh_sync_read(a.sync, it - lag);
        bool acc = false;
        if (ok) {
            const float fs = (float)scale;
            float e[2][U], zp[2][U], xp[2][U];
            float uacc;
            if (a.noise_dz) {
                solo_load_row<U>(a.noise_dz + ((size_t)(it - 1) * C + row) * D, D, pos, e);
                uacc = a.noise_u[(size_t)(it - 1) * C + row];
            } else {
                solo_lane_normals<U>(pos, [&](uint32_t g) { return noise_normal4(a.seed, walker, (uint32_t)it, g, NOISE_STREAM_DZ); }, e);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < 2; ++c) e[c][u] = box.live[c][u] ? e[c][u] : 0.f;   // (padded dims stay 0)
                uacc = noise_uniform(a.seed, walker, (uint32_t)it);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) {   // z' = z + eps * fs: a product and a sum, as torch rounds them (no contraction)
                    zp[c][u] = __fadd_rn(z[c][u], __fmul_rn(e[c][u], fs));
                    xp[c][u] = zp[c][u];
                }
            const float ldp = inverse(xp);
            int okl = 1;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int u = 0; u < U; ++u) okl &= !(xp[c][u] < -1.f || xp[c][u] > 1.f);   // UniformPrior(D, -1, 1): priors.py:39-43
            const bool inb = __ballot(okl != 0) == ~0ull;
            const float log_ratio = inb ? (ldp - ld) : -INFINITY;
            float ratio = fminf(__expf(log_ratio), 1.0f);
            if (log_ratio != log_ratio) ratio = log_ratio;   // NaN stays NaN (u < NaN is false, as in torch)
            const bool pre = __builtin_amdgcn_readfirstlane((int)(uacc < ratio)) != 0;   // (every lane holds the same u and ratio)
            n_call += pre ? 1 : 0;
            if (pre) {   // else the likelihood is skipped: its value decides nothing (see the top)
                float tx[2][U];
                box.map(xp, tx);
                const double lp = glm_solo_loglike<U, FAM>(a.gl, lane, tx);
                acc = lp > loglstar;
                if (acc) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int u = 0; u < U; ++u) { z[c][u] = zp[c][u]; x[c][u] = xp[c][u]; }
                    ld = ldp; logl = lp; n_acc += 1;
                }
            }
            if (writer_lane && a.hist_x) store_row(a.hist_x, (size_t)row * (S + 1) + it, x);
            if (lane == 0 && a.hist_logl) a.hist_logl[(size_t)row * (S + 1) + it] = logl;
        }
        if (batch) {
            if (lane == 0) wave_acc[it & 1][wave] = acc ? 1 : 0;
            __syncthreads();   // the only barrier of the step: all four waves are here, rows >= C included
            const int wg_accepted = wave_acc[it & 1][0] + wave_acc[it & 1][1] + wave_acc[it & 1][2] + wave_acc[it & 1][3];
            int num_accepted = 0;
            if (have_total && lag > 0) num_accepted = mh_sync_total(a.sync, it - lag, nwg, early, a.sync_err);
            if (wave == 0 && lane == 0) mh_sync_post(a.sync, it, blockIdx.x, wg_accepted);
            if (have_total && lag == 0) num_accepted = mh_sync_total(a.sync, it, nwg, mh_sync_read(a.sync, it), a.sync_err);
            if (have_total) votes.vote(scale, num_accepted, C);
        }
    }
    if (a.scale_out && wave == 0 && lane == 0) a.scale_out[blockIdx.x] = (float)scale;
    if (!ok) return;
    bool all_moved = n_acc > 0;
    if (a.x) {
        bool mine = true;
        if (writer_lane) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int d = 2 * U * pos + 2 * u + c;
                    const float x0 = x0buf[wave][pos][2 * u + c];
                    mine = mine && (d >= D || x[c][u] != x0);
                }
        }
        all_moved = (__ballot(mine) & 0xffffull) == 0xffffull;
    }
    if (writer_lane) {
        store_row(a.z, (size_t)row, z);
        if (a.x) store_row(a.x, (size_t)row, x);
        if (pos == 0) {
            a.logl[row] = logl;
            if (a.n_call) a.n_call[row] = n_call;
            if (a.n_accept) a.n_accept[row] = n_acc | (all_moved ? NNEST_MH_ALL_MOVED : 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
template <int U, int FAM>
static hipError_t mh_glm_launch_k(const FlowShape &s, const float *packed, const MhGlmArgs &a, int num_cu, int *max_grid, hipStream_t st) {
    const size_t lds = solo_flow_lds_bytes<U>(s);
    const int grid = (a.C + 3) / 4;
    if (max_grid || (a.flags & NNEST_MH_DYNAMIC_BATCH)) {   // the batch rule's waits span the grid: every workgroup must be resident
        int per_cu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(mh_glm_kernel<U, FAM>), 256, lds);
        if (e != hipSuccess) return e;
        const int cap = (per_cu > 0 ? per_cu : 0) * num_cu;
        if (max_grid) { *max_grid = cap; return hipSuccess; }
        if (grid > cap) return hipErrorLaunchOutOfResources;
    }
    if (a.C <= 0) return hipSuccess;
    hipLaunchKernelGGL((mh_glm_kernel<U, FAM>), dim3(grid), dim3(256), lds, st, s, packed, a);
    return hipGetLastError();
}

template <int FAM>
static hipError_t mh_glm_launch_f(const FlowShape &s, const float *packed, const MhGlmArgs &a, int num_cu, int *max_grid, hipStream_t st) {
    return solo_for_U(s.NT, [&](auto sh) { return mh_glm_launch_k<decltype(sh)::U, FAM>(s, packed, a, num_cu, max_grid, st); });
}

hipError_t launch_mh_glm(const FlowShape &s, const float *packed, const MhGlmArgs &a, int num_cu, int *max_grid, hipStream_t st) {
    if (!slice_form_eligible(s)) return hipErrorInvalidConfiguration;
    switch (a.gl.family) {
        case GLM_LOGISTIC: return mh_glm_launch_f<GLM_LOGISTIC>(s, packed, a, num_cu, max_grid, st);
        case GLM_POISSON: return mh_glm_launch_f<GLM_POISSON>(s, packed, a, num_cu, max_grid, st);
    }
    return hipErrorInvalidConfiguration;
}

}  // namespace nnest
