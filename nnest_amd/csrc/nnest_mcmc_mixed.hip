// nnest_mcmc_mixed.hip -- the MIXED WALK in the latent space of the trained flow: nnest_mcmc_tempered_steps's random-walk Metropolis
// steps with a flow-INDEPENDENCE ("global") step at every global_every-th step of the run, every step of a launch inside the kernel
// (include/nnest_hip.h nnest_mcmc_mixed_steps has the definition in full).  BUILD-DEFINED: the reference has no
// such step.  Walker k of the launch is walker w = walker_offset + k of the run; step t is a global index; with k = global_every:
//   kind:    global iff k > 0 and (t + 1) % k == 0, for all walkers alike; local otherwise;
//   draws:   eps = mcmc_normal4(seed, w, t, g), u = mcmc_uniform(seed, w, t): nnest_mcmc_steps's (a draw is used by one kind);
//   target:  lp = mcmc_target_tempered(logL, log|det|, in_prior, beta) on solo_latent.h's latent target;
//   local:   q = z + step_size * eps; the walker moves iff lp(q) - lp(z) > log u -- mcmc_kernel's step;
//   global:  q = eps; the walker moves iff lw(q) - lw(z) > log u, lw(z) = lp(z) - logb(zz(z)) the log importance weight under the
//            N(0, I) base, zz the float64 sum of squares of the float32 row in importance_kernel's order (the lane's dims in order,
//            then a butterfly over the row's 16 positions).  lw is a function of the row and its lp alone.
//
// Layout: mcmc_kernel's (nnest_mcmc.hip): the solo layout, one walker per wave, four per workgroup, the weights in registers
// (x_dim <= 64) or in LDS.  ONE loop, ONE target evaluation per step: the kind is uniform over the wave and selects only q and the
// two sides of the accept rule; i = -1 is the start.  A run cut into launches is the same run, bit for bit; global_every = 0 is
// nnest_mcmc_tempered_steps's run, bit for bit.
#include <stdio.h>
#include <string.h>

#include "flow_tile.h"
#include "mcmc_mixed.h"
#include "nnest_internal.h"
#include "solo_latent.h"

namespace nnest {

template <int U, int LK>
__global__ void __launch_bounds__(256) mcmc_mixed_kernel(FlowShape s, const float *__restrict__ packed, McmcMixedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = s.D, C = a.C, S = a.S;
    SoloFlow<U>::stage(wlds, s, packed, lane, wave);
    __syncthreads();
    const int pos = lane & 15;
    const int row = blockIdx.x * 4 + wave;
    if (row >= C) return;   // (no barrier behind this point)
    SoloFlow<U> flow;
    flow.init(wlds, s, lane);
    SoloBox<U, LK> box;
    box.init(a, D, lane, pos);
    // x <- f^-1(x) in place; returns lp, and logL(T(x)) through `logl`
    auto target = [&](float (&xs)[2][U], double &logl) -> double {
        return solo_latent_eval(flow, box, xs, [&](double l, float ld, bool in_prior) {
            logl = l;
            return mcmc_target_tempered(l, ld, in_prior, a.beta);
        });
    };

    const bool writer_lane = lane < 16;
    auto store_row = [&](float *base, const float (&v)[2][U]) { solo_store_row<U>(base, D, pos, v); };
    const uint64_t w = a.walker_offset + (uint64_t)row;
    const float step = a.step;
    MixedPhase phase;
    phase.init(a.step0, a.global_every);

    float z[2][U], x[2][U];
    solo_load_row<U>(a.z_in + (size_t)row * D, D, pos, z);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c][u] = z[c][u];
    double lp = 0.0, logl = 0.0;
    int n_acc = 0, n_acc_g = 0;
    const bool hist = a.hist_z != nullptr;
#pragma unroll 1
    for (int i = -1; i < S; ++i) {
        const bool init = i < 0;
        const uint32_t t = a.step0 + (uint32_t)i;
        const bool glob = !init && phase.next_is_global();
        float q[2][U], xq[2][U];
        float uacc = 1.f;
        if (!init) {
            float e[2][U];
            solo_lane_normals<U>(pos, [&](uint32_t g) { return mcmc_normal4(a.seed, w, t, g); }, e);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) {   // (padded dims stay 0)
                    const float ql = mcmc_propose(z[c][u], step, e[c][u]);
                    q[c][u] = box.live[c][u] ? (glob ? e[c][u] : ql) : 0.f;
                }
            uacc = mcmc_uniform(a.seed, w, t);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) q[c][u] = z[c][u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < 2; ++c) xq[c][u] = q[c][u];
        double loglq;
        const double lpq = target(xq, loglq);
        // the two sides of the accept rule: lp on a local step, the log importance weight on a global one
        double lnew = lpq, lold = lp;
        if (glob) {
            lnew = mixed_logw(lpq, solo_row_zz<U>(q), D);
            lold = mixed_logw(lp, solo_row_zz<U>(z), D);
        }
        const bool acc = !init && ens_accept_factor(lnew, lold, 0.0, uacc);
        if (acc || init) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) { z[c][u] = q[c][u]; x[c][u] = xq[c][u]; }
            lp = lpq;
            logl = loglq;
        }
        if (init && a.lp_in) { lp = a.lp_in[row]; logl = a.logl_in[row]; }
        n_acc += acc ? 1 : 0;
        n_acc_g += acc && glob ? 1 : 0;
        if (!init && hist && writer_lane) {
            const size_t hr = (size_t)row * S + i;
            store_row(a.hist_z + hr * D, z);
            store_row(a.hist_x + hr * D, x);
            if (pos == 0) a.hist_logl[hr] = logl;
        }
    }
    if (writer_lane) {
        if (S > 0) store_row(a.z_out + (size_t)row * D, z);   // (steps = 0 evaluates the start: x, lp and logL only)
        store_row(a.x_out + (size_t)row * D, x);
        if (pos == 0) {
            a.lp_out[row] = lp;
            a.logl_out[row] = logl;
            if (S > 0 && a.n_accept) a.n_accept[row] = n_acc;
            if (S > 0 && a.n_accept_global) a.n_accept_global[row] = n_acc_g;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
template <int U, int LK>
static hipError_t mcmc_mixed_launch_k(const FlowShape &s, const float *packed, const McmcMixedArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((mcmc_mixed_kernel<U, LK>), dim3((a.C + 3) / 4), dim3(256), solo_flow_lds_bytes<U>(s), st, s, packed, a);
    return hipGetLastError();
}

hipError_t launch_mcmc_mixed(const FlowShape &s, const float *packed, const McmcMixedArgs &a, hipStream_t st) {
    if (a.C <= 0) return hipSuccess;
    return solo_for_shape(s.NT, a.like.id, [&](auto sh) { return mcmc_mixed_launch_k<decltype(sh)::U, decltype(sh)::LK>(s, packed, a, st); });
}

}  // namespace nnest
