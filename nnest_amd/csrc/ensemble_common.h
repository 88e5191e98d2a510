// ensemble_common.h -- what the kernels of the ensemble sampler share (nnest_ensemble.hip: the NVP's one-walker-per-wave kernel, the
// x-space kernel and the round kernels; nnest_spline_ensemble.hip: the spline flow's tile kernel): the draws, the move's arithmetic,
// (the stretch move's and the differential-evolution move's, and which of the two a step takes),
// the layout of the work buffer, the two ends of the hand-off and the residency bound.  One definition of each: a run is a function
// of the seed, not of its route, because every route computes with these.  (The split table itself is built by
// ensemble_split_kernel, nnest_ensemble.hip, which every route reaches through launch_ensemble_split.)
#pragma once
#include "flow_tile.h"
#include "nnest_internal.h"

namespace nnest {

enum { NOISE_STREAM_ENSEMBLE = 3, NOISE_STREAM_ENSEMBLE_SPLIT = 4 };
constexpr float ENS_A = 2.0f;                  // the stretch scale a (emcee's default)
constexpr long long ENS_SPIN_TICKS = 200000000;   // a hand-off wait gives up after ~2 s of the 100 MHz wall clock
constexpr int ENS_CTRL_WORDS = 4;              // work: [error word, pad x 3][tags, padded to 4 words][inds S x N][members S x N]

__host__ __device__ inline int ens_tags_words(int C) { return (C + 3) & ~3; }
__host__ __device__ inline size_t ens_split_off(int C) { return (size_t)ENS_CTRL_WORDS + ens_tags_words(C); }

// the moves of a run (include/nnest_hip.h nnest_ensemble_moves_steps): step t is a stretch step iff its draw m_t < thr (thr = 2^24:
// always; 0: never), else a differential-evolution (DE) step of scale g0 (1 + sigma n).  Resolved on the host (ens_resolve_moves,
// nnest_abi.hip) and handed to every route as it is
enum { ENS_MOVE_STRETCH = 0, ENS_MOVE_DE = 1 };
constexpr uint32_t ENS_THR_ALWAYS = 1u << 24;
struct EnsMoves { uint32_t thr; float g0, sigma; };

// the walker's three uniforms of step t (24-bit fractions: exact in float32); mw: the fourth word's 24 bits (the DE step's second
// partner)
struct EnsU { float u1, u2, u3; uint32_t m2, mw; };
__device__ __forceinline__ EnsU ens_uniforms(uint64_t seed, uint64_t walker, uint32_t t) {
    u32x4 c;
    c.x = 0;
    c.y = (uint32_t)walker;
    c.z = t;
    c.w = ((uint32_t)(walker >> 32) & 0x0fffffffu) | ((uint32_t)NOISE_STREAM_ENSEMBLE << 28);
    const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    EnsU u;
    u.u1 = (float)(r.x >> 8) * 5.9604644775390625e-08f;
    u.m2 = r.y >> 8;
    u.u2 = (float)u.m2 * 5.9604644775390625e-08f;
    u.u3 = (float)(r.z >> 8) * 5.9604644775390625e-08f;
    u.mw = r.w >> 8;
    return u;
}

// the move of step t, the same for every walker: word x of the split stream's block (0, t, 1) (the split itself draws from z = 0)
__device__ __forceinline__ int ens_move_of_step(uint64_t seed, uint32_t t, uint32_t thr) {
    u32x4 c;
    c.x = 0;
    c.y = t;
    c.z = 1;
    c.w = (uint32_t)NOISE_STREAM_ENSEMBLE_SPLIT << 28;
    const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (r.x >> 8) < thr ? ENS_MOVE_STRETCH : ENS_MOVE_DE;
}

#pragma clang fp contract(off)
// a DE step's own draws: the second partner, member jb != ja of the other set (Nc >= 2 members; ja = (u.m2 Nc) >> 24 is the stretch
// partner's draw), and the scale gamma = g0 (1 + sigma n), n a Box-Muller normal (float64) from a second block of the walker's stream
struct EnsDe { int jb; float gamma; };
__device__ __forceinline__ EnsDe ens_de_draws(uint64_t seed, uint64_t walker, uint32_t t, const EnsU &u, int Nc, const EnsMoves &mv) {
    const int ja = (int)(((uint64_t)u.m2 * (uint64_t)Nc) >> 24);
    int jb = (int)(((uint64_t)u.mw * (uint64_t)(Nc - 1)) >> 24);
    jb += jb >= ja ? 1 : 0;
    u32x4 c;
    c.x = 1;
    c.y = (uint32_t)walker;
    c.z = t;
    c.w = ((uint32_t)(walker >> 32) & 0x0fffffffu) | ((uint32_t)NOISE_STREAM_ENSEMBLE << 28);
    const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double r2 = -2.0 * log((double)((r.x >> 8) + 1u) * 5.9604644775390625e-08);
    const double n = sqrt(r2) * cos(6.283185307179586476925 * ((double)(r.y >> 8) * 5.9604644775390625e-08));
    EnsDe d;
    d.jb = jb;
    d.gamma = (float)((double)mv.g0 * (1.0 + (double)mv.sigma * n));
    return d;
}

__device__ __forceinline__ float ens_zz(float u1) {
    const float s = (ENS_A - 1.0f) * u1 + 1.0f;
    return s * s / ENS_A;
}
__device__ __forceinline__ float ens_propose(float zj, float zk, float zz) { return zj - (zj - zk) * zz; }
__device__ __forceinline__ float ens_de_propose(float zk, float za, float zb, float gamma) { return zk + (zb - za) * gamma; }
__device__ __forceinline__ float ens_T(float x, float sd, float mu) { return x * sd + mu; }
// the latent log target from logL (already safe), the log-det and the prior's verdict
__device__ __forceinline__ double ens_target(double logl, float ld, bool in_prior, int constrained, double loglstar) {
    const double prior = in_prior ? 0.0 : -INFINITY;
    if (constrained) return logl < loglstar ? -INFINITY : (double)ld + prior;
    return (logl + (double)ld) + prior;
}
// the Metropolis rule with the move's factor: (D - 1) log zz for a stretch step, 0 for a DE step
__device__ __forceinline__ bool ens_accept_factor(double lp_new, double lp_old, double factor, float u3) {
    const double lnpdiff = factor + lp_new - lp_old;
    return lnpdiff > log((double)u3);
}
__device__ __forceinline__ bool ens_accept(double lp_new, double lp_old, float zz, float u3, int D) {
    return ens_accept_factor(lp_new, lp_old, (double)(D - 1) * log((double)zz), u3);
}
#pragma clang fp contract(fast)

// the arguments of a fused launch (nnest_ensemble_steps, nnest_ensemble_x_steps, nnest_spline_ensemble_steps).  The flow goes with
// them: FlowShape + packed weights here for the NVP, SplArgs beside them for the spline
struct EnsArgs {
    FlowShape s;
    const float *packed;
    LikeSpec like;                  // scale 1: the likelihood sees T(x)
    const float *t_std, *t_mean;    // [D]
    const float *lo, *hi;           // the prior box on T(x) [D], or NULL (no prior)
    const float *z_in;              // [C][D], read only (a partner may still read it after this walker has finished)
    const double *lp_in;            // [C] or NULL: evaluate lp(z_in)
    float *z_out, *x_out;           // [C][D]
    double *lp_out;                 // [C]
    float *hist_z, *hist_x;         // [C][S][D]
    double *hist_lp;                // [C][S]
    int *n_accept;                  // [C]
    int *work;
    int C, S, constrained;
    uint32_t step0;
    uint64_t seed;
    double loglstar;
    EnsMoves mv;                    // read by the MIX instantiations only (the others run the stretch move alone)
};

// ---- the hand-off (cdna_hip_programming.md Guideline 16, handoff-flag): a walker's finished steps are its history rows, its step
// count in tags[] says how many there are.
// The reading end: the lanes with `waits` poll tags[j] (relaxed, agent scope, s_sleep between polls) until it reaches `need`; the
// loop ends when a ballot finds no lane waiting, then the wave takes ONE acquire before it reads the rows.  Every poll is bounded in
// wall-clock time: a wait that runs out, or that sees the error word set by another wave's, sets the error word and returns false on
// every lane -- the wave leaves, and the call reports it.
__device__ __forceinline__ bool ens_wait(const unsigned *tags, int *err, int j, unsigned need, bool waits) {
    unsigned polls = 0;
    const long long t0 = wall_clock64();
    bool pending = waits;
    for (;;) {
        if (pending) pending = __hip_atomic_load(&tags[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need;
        if (__ballot(pending) == 0ull) break;
        __builtin_amdgcn_s_sleep(1);
        if ((++polls & 63) == 0) {
            const int bad = wall_clock64() - t0 > ENS_SPIN_TICKS || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_readfirstlane(bad)) {
                if (pending) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}
// The writing end, called by the whole wave behind its history stores: one release fence for the wave, a drained wait, then the lanes with `owns`
// store their walker's step count (relaxed sc1 vector stores)
__device__ __forceinline__ void ens_publish(unsigned *tags, int row, unsigned count, bool owns) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the fence's own wait can be dropped by the compiler: Guideline 16, Pitfall 12)
    if (owns) __hip_atomic_store(&tags[row], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- residency: resident 256-thread workgroups per CU: min(the occupancy API, 8, floor(800 / (SGPR granules + 16)))
// (MI355X_MICROARCH.md, "Residency and cooperative launch").  The runtime does not report a kernel's SGPRs, so the SGPR term is taken
// at the ceiling a wave can allocate (102 -> 112 in granules of 16): 6 per CU; the kernels use far fewer and their VGPRs bind first
// (DESIGN.md 3.7).
constexpr int ENS_SGPR_CEIL = 112;
inline hipError_t ens_blocks_per_cu(const void *fn, size_t lds, int *out) {
    hipError_t e = lds ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
    if (e != hipSuccess) return e;
    int n = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, lds);
    if (e != hipSuccess) return e;
    const int sg = 800 / (ENS_SGPR_CEIL + 16);
    *out = n < 8 ? (n < sg ? n : sg) : (8 < sg ? 8 : sg);
    return hipSuccess;
}

// what follows a fused launch on the stream: the error word comes back, and a set one is reported (`name`: the kernel)
inline int ens_finish(const int *work, const char *name, hipStream_t st, char *msg, size_t msg_len) {
    int host_err = 0;
    hipError_t e;
    if ((e = hipMemcpyAsync(&host_err, work, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess) {
        snprintf(msg, msg_len, "%s: %s", name, hipGetErrorString(e));
        return NNEST_E_HIP;
    }
    if (host_err) {
        snprintf(msg, msg_len, "%s: a hand-off wait ran out (a workgroup was not resident?); the outputs are incomplete", name);
        return NNEST_E_HIP;
    }
    return NNEST_OK;
}

}  // namespace nnest
