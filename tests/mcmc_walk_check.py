"""A numpy restatement of the fused random-walk Metropolis move (include/nnest_hip.h nnest_mcmc_steps): the reference's latent-space
Metropolis step with the likelihood, the prior and the Jacobian in the ratio (nnest/sampler.py:372-416) on recorded draws -- the
normals `eps` [N, D] and the uniform `u` [N] of each step, as nnest_mcmc_fill_noise exports them, or any other draws.  Proposals are
float32 with every operation rounded (the kernels' fp contract off), the ratio float64.  The target is the ensemble sampler's
(tests/ensemble_check.latent_target): lp(z) = (logL(T(f^-1(z))) + log|det|) + prior.

`rw_step` records what the GPU replay compares: the proposals, lp(q), the margin lp(q) - lp(z) - log u and the decision.
`mcmc_draws` restates the kernels' own Philox streams (the uniforms to the bit, the normals to rounding): what the exported draws are
checked against, and what seeds are chosen with on the CPU.
"""
import numpy as np

from tests.ensemble_check import latent_target   # noqa: F401  (the target both restatements share; re-exported for the tests)


def rw_step(z, lp, eps, u, step_size, lp_fn, record=None):
    """one step of every walker.  z [N, D] float32, lp [N] float64 (updated copies are returned); eps [N, D] float32, u [N] float32;
    lp_fn(q [n, D] float32) -> lp [n] float64.  record: a dict that receives q, lp_q, margin and accept."""
    z = np.array(z, dtype=np.float32)
    lp = np.array(lp, dtype=np.float64)
    q = z + np.float32(step_size) * np.asarray(eps, np.float32)   # (two rounded float32 operations)
    assert q.dtype == np.float32
    lpq = np.asarray(lp_fn(q), np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):   # (-inf - -inf: NaN, never accepted; log 0 = -inf)
        lnpdiff = 0.0 + lpq - lp
        logu = np.log(np.asarray(u, np.float32).astype(np.float64))
        margin = lnpdiff - logu
    acc = lnpdiff > logu
    if record is not None:
        record.update(q=q.copy(), lp_q=lpq, margin=margin, accept=acc)
    z[acc] = q[acc]
    lp[acc] = lpq[acc]
    return z, lp


def rw_run(z, lp, draws, step_size, lp_fn):
    """steps of rw_step on draws = [(eps, u), ...]; returns z, lp, the history of z [N, S, D] and lp [N, S], and how often each
    walker moved [N]"""
    hz, hl = [], []
    n_acc = np.zeros(len(z), np.int64)
    for eps, u in draws:
        rec = {}
        z, lp = rw_step(z, lp, eps, u, step_size, lp_fn, record=rec)
        n_acc += rec['accept']
        hz.append(z)
        hl.append(lp)
    return z, lp, np.stack(hz, 1), np.stack(hl, 1), n_acc


def numpy_draws(rng, N, D, S):
    """draws with the kernels' structure from a numpy generator: float32 normals, 24-bit uniforms"""
    return [(rng.standard_normal((N, D)).astype(np.float32),
             (np.floor(rng.uniform(size=N) * (1 << 24)) / (1 << 24)).astype(np.float32)) for _ in range(S)]


# ---- the kernels' own draws, restated (include/nnest_hip.h nnest_mcmc_steps): Philox4x32-10, streams 5 (normals) and 6 (uniform) ----
_M32 = np.uint64(0xffffffff)


def philox4x32_10(ctr, seed):
    """Philox4x32-10 blocks: ctr [..., 4] (uint32 values), key = the two halves of `seed` -> [..., 4] uint64 holding 32-bit words"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & _M32 for i in range(4)]
    k0, k1 = np.uint64(int(seed) & 0xffffffff), np.uint64((int(seed) >> 32) & 0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(c, -1)


def _counters(x, walkers, t, stream):
    walkers = np.asarray(walkers, np.uint64)
    w_hi = ((walkers >> np.uint64(32)) & np.uint64(0x0fffffff)) | np.uint64(stream << 28)
    return np.stack(np.broadcast_arrays(np.asarray(x, np.uint64), walkers & _M32, np.uint64(int(t) & 0xffffffff), w_hi), -1)


def mcmc_draws(seed, walker_offset, C, step0, S, D):
    """what nnest_mcmc_fill_noise exports: eps [S, C, D] and u [S, C] float32.  u is exact (24 bits).  eps is Box-Muller in float32 with
    numpy's log / sin / cos where the kernels use the hardware's approximations: equal to rounding, not to the bit"""
    walkers = int(walker_offset) + np.arange(C, dtype=np.uint64)
    G = (D + 3) // 4
    eps, u = np.empty((S, C, 4 * G), np.float32), np.empty((S, C), np.float32)
    for i in range(S):
        t = int(step0) + i
        r = philox4x32_10(_counters(np.arange(G, dtype=np.uint64)[None, :], walkers[:, None], t, 5), seed)   # [C, G, 4]
        f = r.astype(np.float32).astype(np.float64)   # (float)r: uint32 -> float32, rounded to nearest
        u1 = (f[..., 0::2] * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)   # fmaf: one rounding
        ang = (f[..., 1::2] * 2.0 ** -32).astype(np.float32)               # revolutions
        rad = np.sqrt(np.float32(-2.0) * np.log(u1)).astype(np.float32)
        n = np.stack([rad * np.cos(2 * np.pi * ang.astype(np.float64)), rad * np.sin(2 * np.pi * ang.astype(np.float64))], -1)   # [C, G, 2, 2]
        eps[i] = n.reshape(C, 4 * G).astype(np.float32)
        ru = philox4x32_10(_counters(0, walkers, t, 6), seed)
        u[i] = ((ru[..., 0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return eps[:, :, :D], u
