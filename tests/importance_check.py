"""A numpy restatement of the importance-sampled evidence (include/nnest_hip.h nnest_importance_evidence): Z = E_q[L pi / q] with the flow
as the proposal q.  Sample m draws z_m from N(0, I) -- the kernels' Philox stream 7 restated (`importance_draws`), or any other draws
--, the weight is logw = lp(z) - logb(z) in float64 with lp the latent target of the ensemble and random-walk kernels
(tests/ensemble_check.latent_target) and logb the base's log density in float64 from the float32 z; a sample is live when logw is
neither NaN nor -inf; the sums are a = max logw over the live samples, S1 = sum e^(logw - a), S2 = sum e^(2 (logw - a)) and n_live.
`merge` and `result` restate nnest_amd._lib.merge_importance / importance_result."""
import numpy as np

from tests.ensemble_check import latent_target   # noqa: F401  (the target; re-exported for the tests)
from tests.mcmc_walk_check import _counters, philox4x32_10

STREAM = 7   # NOISE_STREAM_IMPORTANCE


def importance_draws(seed, sample_offset, M, D):
    """what nnest_importance_fill_noise exports: z [M, D] float32, row k the draws of sample sample_offset + k (step 0 of stream 7).
    Box-Muller in float32 with numpy's log / sin / cos where the kernels use the hardware's approximations: equal to rounding, not to
    the bit (as mcmc_walk_check.mcmc_draws)"""
    m = int(sample_offset) + np.arange(M, dtype=np.uint64)
    G = (D + 3) // 4
    r = philox4x32_10(_counters(np.arange(G, dtype=np.uint64)[None, :], m[:, None], 0, STREAM), seed)   # [M, G, 4]
    f = r.astype(np.float32).astype(np.float64)
    u1 = (f[..., 0::2] * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)
    ang = (f[..., 1::2] * 2.0 ** -32).astype(np.float32)
    rad = np.sqrt(np.float32(-2.0) * np.log(u1)).astype(np.float32)
    n = np.stack([rad * np.cos(2 * np.pi * ang.astype(np.float64)), rad * np.sin(2 * np.pi * ang.astype(np.float64))], -1)
    return n.reshape(M, 4 * G).astype(np.float32)[:, :D]


def logb(z):
    """log N(z; 0, I) in float64 from the float32 z"""
    z = np.asarray(z, np.float32).astype(np.float64)
    return -0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * np.log(2.0 * np.pi)


def logw_of(z, lp_fn):
    """logw [M] float64 of the draws z [M, D] float32 under the latent target lp_fn"""
    with np.errstate(invalid='ignore'):
        return np.asarray(lp_fn(np.asarray(z, np.float32)), np.float64) - logb(z)


def is_live(logw):
    logw = np.asarray(logw, np.float64)
    return ~(np.isnan(logw) | (logw == -np.inf))


def sums(logw):
    """(a, S1, S2, n_live) of a set of log weights"""
    logw = np.asarray(logw, np.float64)
    lw = logw[is_live(logw)]
    if lw.size == 0:
        return -np.inf, 0.0, 0.0, 0.0
    a = float(lw.max())
    e = np.exp(lw - a)
    return a, float(e.sum()), float((e * e).sum()), float(lw.size)


def merge(parts):
    """the sums of the union from the sums of the parts"""
    parts = list(parts)
    a = max([p[0] for p in parts] + [-np.inf])
    s1 = s2 = n = 0.0
    for ai, s1i, s2i, ni in parts:
        if ai == -np.inf:
            continue
        s1 += s1i * np.exp(ai - a)
        s2 += s2i * np.exp(2.0 * (ai - a))
        n += ni
    return a, s1, s2, n


def result(a, S1, S2, n_live, M):
    """logz (over x), ess, logzerr, max_weight_share"""
    if not (n_live > 0 and S1 > 0):
        return dict(logz_x=-np.inf, ess=0.0, logzerr=np.inf, max_weight_share=np.nan)
    ess = S1 * S1 / S2
    return dict(logz_x=a + np.log(S1) - np.log(M), ess=ess, logzerr=np.sqrt(max(M / ess - 1.0, 0.0) / (M - 1)) if M > 1 else np.inf,
                max_weight_share=1.0 / S1)
